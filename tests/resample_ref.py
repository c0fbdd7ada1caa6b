"""The output-rate resampler's definition (include/vitsmi.h, "output rate") evaluated in float64 with NumPy, from its own
float64 table: the reference of tests/test_resample_cpu.py and tests/test_gpu_resample.py.  Nothing here calls the engine."""
import math
from functools import lru_cache

import numpy as np

Z, BETA, RHO = 16, 8.555504641634386, 0.85


def plan(fi, fo):
    """(L, M, K, s, W) of the definition."""
    g = math.gcd(fi, fo)
    L, M = fo // g, fi // g
    s = RHO * min(1.0, L / M)
    W = Z / s
    return L, M, 2 * math.ceil(W), s, W


@lru_cache(maxsize=None)
def table64(fi, fo):
    """h[p][j] = k(p / L + K / 2 - 1 - j) in float64, [L, K] (not rounded to fp32)."""
    L, M, K, s, W = plan(fi, fo)
    d = np.arange(L, dtype=np.float64)[:, None] / L + (K // 2 - 1 - np.arange(K, dtype=np.float64))[None, :]
    u = d / W
    kaiser = np.where(np.abs(u) < 1.0, np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA), 0.0)
    h = s * np.sinc(s * d) * kaiser
    h.setflags(write=False)
    return h


def count(n, fi, fo):
    """ceil(n * L / M) (integers or integer arrays)"""
    L, M = plan(fi, fo)[:2]
    return -(-np.asarray(n, np.int64) * L // M)


def resample64(x, fi, fo):
    """One row's valid samples x [n] -> its N = ceil(n * L / M) output samples, float64."""
    L, M, K, _, _ = plan(fi, fo)
    h = table64(fi, fo)
    x = np.asarray(x, np.float64)
    N = int(count(len(x), fi, fo))
    n = np.arange(N, dtype=np.int64)
    i, p = n * M // L, n * M % L
    xp = np.concatenate([np.zeros(K), x, np.zeros(K)])   # x[m] = 0 for m < 0 and m >= len(x)
    idx = (i - K // 2 + 1 + K)[:, None] + np.arange(K)[None, :]
    return (h[p] * xp[idx]).sum(axis=1)


def tolerance(fi, fo, xmax):
    """Bound on |fp32 engine - float64 definition| for inputs of magnitude <= xmax: K fused multiply-adds give at most K
    roundings of partial sums bounded by sum |h||x|, the table's own rounding and the final store the other two:
    (K + 2) * 2^-24 * max_p sum_j |h[p][j]| * max|x|."""
    K = plan(fi, fo)[2]
    return (K + 2) * 2.0 ** -24 * float(np.abs(table64(fi, fo)).sum(axis=1).max()) * float(xmax)
