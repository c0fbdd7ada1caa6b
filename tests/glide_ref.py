"""The pitch contours' definition (include/vitsmi.h, "pitch contours") in float64 and Python integers: the reference of
tests/test_glide_cpu.py and tests/test_gpu_glide.py.  The table and the tap weights are warp_ref's; nothing here calls the
engine."""
from collections import namedtuple

import numpy as np

import warp_ref
from warp_ref import FB, ONE, Z

# Bound on max s * sum |w| over EVERY step in [ONE / 2, 2 * ONE] and 128 fractional phases, rounded up to two decimals
# (measure_gain() measures 1.9870; tests/test_glide_cpu.py re-measures it).  warp_ref.GAIN = 1.98 was measured at eight cutoffs only.
GAIN = 1.99
MAX_SPAN = 1 << 23

Seg = namedtuple("Seg", "n0 pos0 k step0 step1")


def token(st0, st1):
    """(a, b, rate) of a token gliding from st0 to st1: warp_ref.token's steps, and float32((r0 + r1) / 2)"""
    a, b = warp_ref.token(st0)[0], warp_ref.token(st1)[0]
    r0, r1 = 2.0 ** (float(np.float32(st0)) / 12.0), 2.0 ** (float(np.float32(st1)) / 12.0)
    return a, b, np.float32((r0 + r1) * 0.5)


def cutoff(s):
    """(c, Kh) of an output sample at speed s, in integers"""
    s = int(s)
    c = 55706 if s <= ONE else ((17 << 32) + 10 * s) // (20 * s)
    return c, -(-Z * ONE // c)


def pos_at(g, j):
    """Q16 position of sample j of the record (j == k: where the next token starts); Python integers"""
    j, d = int(j), abs(g.step1 - g.step0)
    q = (d * j * (j - 1)) // (2 * g.k) if g.k else 0
    return g.pos0 + j * g.step0 + (q if g.step1 >= g.step0 else -q)


def step_at(g, j):
    d = abs(g.step1 - g.step0)
    q = (d * int(j)) // g.k
    return g.step0 + (q if g.step1 >= g.step0 else -q)


def samples(g):
    """(pos_j, s_j) for j = 0 .. k - 1 as int64 arrays (exact: object arithmetic where int64 products could overflow)"""
    j = np.arange(g.k, dtype=object if g.k > (1 << 20) else np.int64)
    d = abs(g.step1 - g.step0)
    sgn = 1 if g.step1 >= g.step0 else -1
    pos = g.pos0 + j * g.step0 + sgn * ((d * j * (j - 1)) // (2 * g.k))
    s = g.step0 + sgn * ((d * j) // g.k)
    return pos.astype(np.int64), s.astype(np.int64)


def plan(D, st0, st1, hop):
    """One row: (segments, spans [len(D)], N).  D: the rendered durations in frames; st0 / st1: semitones per token."""
    pos = n = cum = 0
    segs, spans = [], np.zeros(len(D), np.int64)
    for t, d in enumerate(D):
        d = int(d)
        if d == 0:
            continue
        a, b, _ = token(st0[t], st1[t])
        cum += d
        P = (cum * hop) << FB
        k = 0 if P <= pos else -(-2 * (P - pos) // (a + b))
        if k > MAX_SPAN:
            raise ValueError(f"token {t}: {k} output samples")
        g = Seg(n, pos, k, a, b)
        segs.append(g)
        spans[t] = k
        n += k
        pos = pos_at(g, k)
    return segs, spans, n


def identity(segs):
    return all(g.step0 == ONE and g.step1 == ONE for g in segs)


def max_half(segs):
    """the largest Kh the row visits"""
    return max((cutoff(max(g.step0, g.step1))[1] for g in segs if g.k), default=0)


def glide64(x, segs, N):
    """One row's valid samples x [n_b] -> its N output samples, float64 (an identity row: its native samples)."""
    x = np.asarray(x, np.float64)
    y = np.zeros(N, np.float64)
    if identity(segs):
        n = min(N, len(x))
        y[:n] = x[:n]
        return y
    pad = 2 * Z * 3
    for g in segs:
        if g.k == 0:
            continue
        pos, s = samples(g)
        c = np.where(s <= ONE, 55706, ((17 << 32) + 10 * s) // (20 * s))
        # (every sample with the token's longest Kh: the taps beyond a sample's own Kh have weight 0 by the table's end)
        m, w = warp_ref.weights(pos, c[:, None], cutoff(max(g.step0, g.step1))[1])
        hi = int(m.max()) + 1
        lo = max(0, -int(m.min()))
        xp = np.concatenate([np.zeros(pad + lo), x, np.zeros(max(0, hi - len(x)) + pad)])   # x[m] = 0 outside [0, n_b)
        y[g.n0:g.n0 + g.k] = (w * xp[m + pad + lo]).sum(axis=1)
    return y


def tolerance(segs, xmax):
    """warp_ref.tolerance's bound with this module's GAIN and the largest Kh the row visits"""
    return (2 * max_half(segs) + 4) * 2.0 ** -24 * GAIN * float(xmax)


def contour_ids(sizes, value):
    """TTSVoice's pitch_contour restated: a sentence of n phoneme groups, group i of sizes[i] ids; group i glides from
    value(i / n) to value((i + 1) / n) and its m ids split that glide into m equal parts in semitones -> (st0, st1) per id"""
    n = len(sizes)
    st0, st1 = [], []
    for i, m in enumerate(sizes):
        v0, v1 = value(i / n), value((i + 1) / n)
        cuts = [v0] + [v0 + (v1 - v0) * q / m for q in range(1, m)] + [v1]
        st0 += cuts[:m]
        st1 += cuts[1:]
    return st0, st1


def measure_gain(phases=128):
    """max s * sum |w| over every step in [ONE / 2, 2 * ONE] - the weights depend on the step through c alone, so over every
    distinct c - and `phases` fractional phases.  Phase ONE - f has the taps of phase f mirrored (d -> 1 - d), the same
    sum: the first phases / 2 + 1 phases are evaluated."""
    cs = sorted({cutoff(s)[0] for s in range(ONE // 2, 2 * ONE + 1)})
    pos = (np.arange(phases // 2 + 1, dtype=np.int64) * (ONE // phases)) + (100 << FB)
    phases = len(pos)
    best = 0.0
    by_half = {}
    for c in cs:
        by_half.setdefault(-(-Z * ONE // c), []).append(c)
    for Kh, group in by_half.items():
        c = np.repeat(np.asarray(group, np.int64), phases)
        p = np.tile(pos, len(group))
        for i in range(0, len(c), 1 << 16):
            w = warp_ref.weights(p[i:i + (1 << 16)], c[i:i + (1 << 16), None], Kh)[1]
            best = max(best, float(np.abs(w).sum(axis=1).max()))
    return best


def figures(glides=((-12, 12), (12, -12), (-3, 4), (0, 7))):
    """The tone figure the header quotes: a tone at f0 = 0.15 / max(1, r_max) through one long gliding token comes out as
    cos(2 pi f0 pos_j / ONE + phase); the largest deviation away from the row's ends."""
    worst = 0.0
    n_in = 6000
    m = np.arange(n_in, dtype=np.float64)
    for st0, st1 in glides:
        a, b, _ = token(st0, st1)
        k = -(-2 * ((n_in - 200) << FB) // (a + b))
        g = Seg(0, 0, k, a, b)
        pos, _ = samples(g)
        f0 = 0.15 / max(1.0, a / ONE, b / ONE)
        for ph in (0.0, 0.7):
            y = glide64(np.cos(2 * np.pi * f0 * m + ph), [g], k)
            want = np.cos(2 * np.pi * f0 * (pos / ONE) + ph)
            lo = 2 * 38 + 2
            worst = max(worst, float(np.abs(y - want)[lo:k - lo].max()))
    return worst
