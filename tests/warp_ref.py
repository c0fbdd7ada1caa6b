"""The per-token time warp's definition (include/vitsmi.h, "intonation") evaluated in float64 with NumPy, from its own
float64 prototype table: the reference of tests/test_warp_cpu.py and tests/test_gpu_warp.py.  Nothing here calls the engine."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

Z, BETA, RHO = 16, 8.555504641634386, 0.85
R, FB = 512, 16
ONE = 1 << FB
GAIN = 1.98   # bound on max s * sum |w| (asserted against this reference in tests/test_warp_cpu.py)

Seg = namedtuple("Seg", "n0 pos0 step c Kh k")


def proto(u):
    """g(u) = sinc(u) * kaiser(u / Z) for 0 <= u < Z, else 0 (float64, u >= 0)"""
    u = np.asarray(u, np.float64)
    t = u / Z
    kaiser = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - t * t))) / np.i0(BETA)
    return np.where(u < Z, np.sinc(u) * kaiser, 0.0)


@lru_cache(maxsize=None)
def table64():
    """G[i] = g(i / R), i = 0 .. Z*R + 1, in float64 (not rounded to fp32)"""
    G = proto(np.arange(Z * R + 2, dtype=np.float64) / R)
    G.setflags(write=False)
    return G


def token(st):
    """(step, c, Kh) of a token at st semitones"""
    st = float(np.float32(st))
    if not math.isfinite(st) or abs(st) > 12:
        raise ValueError(f"semitones {st} is not a finite value within [-12, 12]")
    r = 2.0 ** (st / 12.0)
    step = int(np.rint(r * ONE))
    s = RHO * min(1.0, ONE / step)
    c = int(np.rint(s * ONE))
    return step, c, -(-Z * ONE // c)


def plan(D, st, hop):
    """One row: (segments, spans [len(D)], N).  D: the rendered durations in frames, st: semitones per token."""
    pos = n = cum = 0
    segs, spans = [], np.zeros(len(D), np.int64)
    for t, d in enumerate(D):
        d = int(d)
        if d == 0:
            continue
        step, c, Kh = token(st[t])
        cum += d
        P = (cum * hop) << FB
        k = 0 if P <= pos else -(-(P - pos) // step)
        segs.append(Seg(n, pos, step, c, Kh, k))
        spans[t] = k
        n += k
        pos += k * step
    return segs, spans, n


def identity(segs):
    return all(g.step == ONE for g in segs)


def weights(pos, c, Kh):
    """the taps of the samples at Q16 positions pos [n]: (m [n, 2 Kh], s * w [n, 2 Kh]) in float64"""
    G = table64()
    pos = np.asarray(pos, np.int64)
    m = (pos >> FB)[:, None] + np.arange(1 - Kh, Kh + 1, dtype=np.int64)[None, :]
    v = np.abs((m << FB) - pos[:, None]) * c
    i = v >> 23
    f = (v & 0x7FFFFF).astype(np.float64) * 2.0 ** -23
    ic = np.minimum(i, Z * R)
    w = np.where(i < Z * R, G[ic] + f * (G[ic + 1] - G[ic]), 0.0)
    return m, (c / 65536.0) * w


def warp64(x, segs, N):
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
        pos = g.pos0 + np.arange(g.k, dtype=np.int64) * g.step
        m, w = weights(pos, g.c, g.Kh)
        hi = int(m.max()) + 1
        xp = np.concatenate([np.zeros(pad), x, np.zeros(max(0, hi - len(x)) + pad)])   # x[m] = 0 outside [0, n_b)
        y[g.n0:g.n0 + g.k] = (w * xp[m + pad]).sum(axis=1)
    return y


def tolerance(segs, xmax):
    """Bound on |fp32 engine - float64 definition| for inputs of magnitude <= xmax.  A sample is 2 Kh fused multiply-adds:
    at most 2 Kh roundings of partial sums bounded by sum |w||x|; each weight carries the table's rounding, the rounding of
    the difference G[i+1] - G[i] and of its own fmaf - first-order terms against sum |w| again, counted as three more -, and
    the final product one: (2 Kh + 4) * 2^-24 * (max s * sum |w|) * max|x|, with the largest Kh among the row's segments."""
    Kh = max((g.Kh for g in segs), default=0)
    return (2 * Kh + 4) * 2.0 ** -24 * GAIN * float(xmax)


def figures(sts=(-12, -7, -3, -1, 1, 3, 7, 12)):
    """The figures the header quotes, measured on this reference: (tone_err, interp_err, alias, gain)."""
    tone = gain = alias = 0.0
    n_in = 6000
    m = np.arange(n_in, dtype=np.float64)
    for st in sts:
        step, c, Kh = token(st)
        r = step / ONE
        k = int((n_in - 200) / r)
        seg = [Seg(0, 0, step, c, Kh, k)] if step != ONE else None
        n = np.arange(k, dtype=np.float64)
        f0 = 0.15 * min(1.0, 1.0 / r)
        for ph in (0.0, 0.7):
            y = warp64(np.cos(2 * np.pi * f0 * m + ph), seg, k) if seg else None
            if y is not None:
                lo = int(2 * Kh / r) + 2
                tone = max(tone, float(np.abs(y - np.cos(2 * np.pi * f0 * r * n + ph))[lo:k - lo].max()))
        if r > 1.2:   # a tone that would land at 0.6 of the output rate: above its Nyquist, to be removed
            y = warp64(np.cos(2 * np.pi * (0.6 / r) * m), [Seg(0, 0, step, c, Kh, k)], k)
            lo = int(2 * Kh / r) + 2
            alias = max(alias, float(np.abs(y[lo:k - lo]).max()))
        pos = np.arange(0, ONE, 16, dtype=np.int64) + (100 << FB)
        gain = max(gain, float(np.abs(weights(pos, c, Kh)[1]).sum(axis=1).max()))
    u = np.arange(0, Z * R * 8 + 1, dtype=np.float64) / (R * 8)
    i = np.minimum((u * R).astype(np.int64), Z * R)
    G = table64()
    interp = float(np.abs(G[i] + (u * R - i) * (G[i + 1] - G[i]) - proto(u)).max())
    return tone, interp, alias, gain
