"""Pitch at an output rate (include/vitsmi.h, "pitch at an output rate") in float64 and Python integers: the folded token and
the identity-row rule on top of warp_ref, glide_ref and resample_ref - the reference of tests/test_warp_rate_cpu.py and
tests/test_gpu_warp_rate.py.  Nothing here calls the engine."""
import math

import numpy as np

import glide_ref
import resample_ref
import warp_ref
from warp_ref import FB, ONE, RHO, Z

MIN_STEP, MAX_STEP, MAX_HALF = ONE // 8, ONE * 8, 151
MAX_SPAN = 1 << 22   # a gliding token of a folded plan: |b - a| * j * (j - 1) < 2^19 * 2^44 stays inside 64 bits

# Bound on max s * sum |w| over EVERY step of [ONE / 8, 8 ONE] - through its 48 744 distinct cutoffs - and 128 fractional phases,
# rounded up to two decimals: measured 1.98693 (at c = 32743, a step near 1.70 ONE).  On the steps of the listed rate pairs with
# ONE / 8, ONE and 8 ONE it is 1.947, below warp_ref.GAIN = 1.98; a dense grid exceeds that, as glide_ref.GAIN records for
# [ONE / 2, 2 ONE], so this module's tolerance counts with its own bound.
GAIN = 1.99

# the rate pairs the section quotes its figures for
PAIRS = [(22050, 8000), (22050, 11025), (22050, 16000), (22050, 24000), (22050, 44100), (22050, 48000), (16000, 8000), (16000, 48000),
         (24000, 8000), (32000, 8000), (8000, 32000)]


def ratio(fi, fo):
    """(L, M) of the output plan: fo = fi * L / M"""
    g = math.gcd(int(fi), int(fo))
    return int(fo) // g, int(fi) // g


def admitted(L, M):
    return M <= 4 * L and L <= 4 * M


def token(st, L, M):
    """(step, c, Kh) of a token at st semitones delivered at fi * L / M: the rate folded into the step"""
    st = float(np.float32(st))
    if not math.isfinite(st) or abs(st) > 12:
        raise ValueError(f"semitones {st} is not a finite value within [-12, 12]")
    step = int(np.rint(2.0 ** (st / 12.0) * float(M) / float(L) * ONE))
    s = RHO * min(1.0, ONE / step)
    c = int(np.rint(s * ONE))
    return step, c, -(-Z * ONE // c)


def plan(D, st, hop, L, M):
    """warp_ref.plan given the folded steps: P stays a native input position, n0 / k / N are delivered samples"""
    pos = n = cum = 0
    segs, spans = [], np.zeros(len(D), np.int64)
    for t, d in enumerate(D):
        d = int(d)
        if d == 0:
            continue
        step, c, Kh = token(st[t], L, M)
        cum += d
        P = (cum * hop) << FB
        k = 0 if P <= pos else -(-(P - pos) // step)
        segs.append(warp_ref.Seg(n, pos, step, c, Kh, k))
        spans[t] = k
        n += k
        pos += k * step
    return segs, spans, n


def glide_plan(D, st0, st1, hop, L, M):
    """glide_ref.plan given the folded steps"""
    pos = n = cum = 0
    segs, spans = [], np.zeros(len(D), np.int64)
    for t, d in enumerate(D):
        d = int(d)
        if d == 0:
            continue
        a, b = token(st0[t], L, M)[0], token(st1[t], L, M)[0]
        cum += d
        P = (cum * hop) << FB
        k = 0 if P <= pos else -(-2 * (P - pos) // (a + b))
        if k > MAX_SPAN:
            raise ValueError(f"token {t}: {k} output samples")
        g = glide_ref.Seg(n, pos, k, a, b)
        segs.append(g)
        spans[t] = k
        n += k
        pos = glide_ref.pos_at(g, k)
    return segs, spans, n


def identity_spans(D, hop, L, M, n_in):
    """An identity row - every token at 0 semitones - by the resampler's rule: (spans [len(D)], N = ceil(n_in * L / M)), token
    t's span the difference of ceil(cum_t * hop * L / M) clamped to N"""
    N = -(-int(n_in) * L // M)
    cum = prev = 0
    spans = np.zeros(len(D), np.int64)
    for t, d in enumerate(D):
        cum += max(int(d), 0)
        e = min(-(-cum * hop * L // M), N)
        spans[t] = e - prev
        prev = e
    return spans, N


def warp64(x, segs, N):
    """warp_ref.warp64 without its copy branch and with room for 151 half-taps in front of the row: every record is rendered"""
    x = np.asarray(x, np.float64)
    y = np.zeros(N, np.float64)
    pad = MAX_HALF + 1
    for g in segs:
        if g.k == 0:
            continue
        pos = g.pos0 + np.arange(g.k, dtype=np.int64) * g.step
        m, w = warp_ref.weights(pos, g.c, g.Kh)
        hi = int(m.max()) + 1
        xp = np.concatenate([np.zeros(pad), x, np.zeros(max(0, hi - len(x)) + pad)])   # x[m] = 0 outside [0, n_b)
        y[g.n0:g.n0 + g.k] = (w * xp[m + pad]).sum(axis=1)
    return y


def glide64(x, segs, N):
    """glide_ref.glide64 without its copy branch"""
    x = np.asarray(x, np.float64)
    y = np.zeros(N, np.float64)
    pad = MAX_HALF + 1
    for g in segs:
        if g.k == 0:
            continue
        pos, s = glide_ref.samples(g)
        c = np.where(s <= ONE, 55706, ((17 << 32) + 10 * s) // (20 * s))
        m, w = warp_ref.weights(pos, c[:, None], glide_ref.cutoff(max(g.step0, g.step1))[1])
        hi = int(m.max()) + 1
        xp = np.concatenate([np.zeros(pad), x, np.zeros(max(0, hi - len(x)) + pad)])
        y[g.n0:g.n0 + g.k] = (w * xp[m + pad]).sum(axis=1)
    return y


def identity64(x, fi, fo):
    """an identity row: the resampler's definition (its native samples where the rates are equal)"""
    return np.asarray(x, np.float64) if fi == fo else resample_ref.resample64(x, fi, fo)


def max_half(segs):
    """the largest Kh a row of either family's records visits"""
    return max((glide_ref.cutoff(max(g.step0, g.step1))[1] if hasattr(g, "step0") else g.Kh for g in segs if g.k), default=0)


def tolerance(segs, xmax):
    """warp_ref.tolerance's bound - (2 Kh + 4) * 2^-24 * (max s * sum |w|) * max|x| - with this module's GAIN and the largest Kh the
    row visits"""
    return (2 * max_half(segs) + 4) * 2.0 ** -24 * GAIN * float(xmax)


def row_pos(segs, n):
    """Q16 input position of output sample n of a row of warp_ref.Seg or glide_ref.Seg records (Python integers)"""
    g = [q for q in segs if q.n0 <= n][-1]
    return glide_ref.pos_at(g, n - g.n0) if hasattr(g, "step0") else g.pos0 + (n - g.n0) * g.step


def gain(steps, phases=64):
    """max s * sum |w| of the reference over `steps` (through their cutoffs) and `phases` fractional phases"""
    best = 0.0
    pos = (np.arange(phases // 2 + 1, dtype=np.int64) * (ONE // phases)) + (200 << FB)
    for c in sorted({glide_ref.cutoff(s)[0] for s in steps}):
        best = max(best, float(np.abs(warp_ref.weights(pos, c, -(-Z * ONE // c))[1]).sum(axis=1).max()))
    return best


def tone(L, M, sts=(-12, -5, 0, 3, 12)):
    """warp_ref.figures' tone figure with folded tokens: a tone at 0.15 * min(1, 1 / r) cycles per sample through one token of
    step r lands at r times its frequency; the largest deviation away from the row's ends"""
    worst = 0.0
    n_in = 6000
    m = np.arange(n_in, dtype=np.float64)
    for st in sts:
        step, c, Kh = token(st, L, M)
        r = step / ONE
        k = int((n_in - 400) / r)
        n = np.arange(k, dtype=np.float64)
        f0 = 0.15 * min(1.0, 1.0 / r)
        for ph in (0.0, 0.7):
            y = warp64(np.cos(2 * np.pi * f0 * m + ph), [warp_ref.Seg(0, 0, step, c, Kh, k)], k)
            lo = int(2 * Kh / r) + 2
            worst = max(worst, float(np.abs(y - np.cos(2 * np.pi * f0 * r * n + ph))[lo:k - lo].max()))
    return worst
