"""Plain NumPy references of the kernels between the token domain and the waveform (csrc/kernels.hip.hpp: duration_kernel,
forced_duration_kernel, expand_prior_strided_kernel, post_conv_tanh_kernel and its blocked form): float64 where values are
compared, int64 where indices are.  Settings (length_scale, noise_scale, rates) are taken at their float32 values, as the
engine receives them."""
import numpy as np


def _f32_as_f64(v):
    return np.asarray(v, np.float32).astype(np.float64)


def durations_ref(logw, lens, length_scale=1.0, rate=None):
    """models.py:702-704.  logw [B, T], lens [B], length_scale a scalar or [B], rate (optional) [B, T] ->
    (w_ceil float32 [B, T] = ceil(exp(logw) * mask * length_scale [* rate]), cum int64 [B, T] its inclusive running sum,
    y_len int64 [B] = max(sum, 1), pre float64 [B, T] the value under the ceil)."""
    logw = np.asarray(logw, np.float64)
    B, T = logw.shape
    lens = np.asarray(lens, np.int64)
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)
    ls = _f32_as_f64(length_scale)
    pre = np.exp(logw) * mask * (ls[:, None] if ls.ndim else ls)
    if rate is not None:
        pre = pre * np.where(mask > 0, _f32_as_f64(rate), 1.0)
    w = np.ceil(pre)
    cum = np.cumsum(w.astype(np.int64), axis=1)
    return w.astype(np.float32), cum, np.maximum(cum[:, -1], 1), pre


def forced_durations_ref(dur, lens):
    """What forced durations leave behind: (w_ceil float32 [B, T] = dur for t < lens[b], 0 behind; cum int64; y_len int64)"""
    dur = np.asarray(dur, np.int64)
    T = dur.shape[1]
    d = np.where(np.arange(T)[None, :] < np.asarray(lens, np.int64)[:, None], dur, 0)
    cum = np.cumsum(d, axis=1)
    return d.astype(np.float32), cum, np.maximum(cum[:, -1], 1)


def regulate_ref(m_p, logs_p, dur, noise, noise_scale, ylen, F=None, parts=False):
    """NumPy length regulator + prior sample (commons.py:116-129, models.py:711-718) over the run's own m_p / logs_p:
    z_p[b, c, f] = m_p[b, c, i(f)] + noise[b, c, f] * exp(logs_p[b, c, i(f)]) * noise_scale, i(f) = the token frame f belongs
    to under `dur`; frames with no token (f >= ylen[b], up to F - the one masked frame of an utterance without any frame among
    them) see m = 0, logs = 0: 0 + noise * exp(0) * noise_scale.  float64 [B, C, F], F = ylen.max() unless given; noise
    [B, C, Fn] reads as 0 behind Fn; noise_scale a scalar or [B].  parts=True: (the gathered m, the noise term) instead of
    their sum."""
    m_p, logs_p = np.asarray(m_p, np.float64), np.asarray(logs_p, np.float64)
    B, C, T = m_p.shape
    F = int(np.max(ylen)) if F is None else int(F)
    nz = np.zeros((B, C, F), np.float64)
    Fn = min(F, noise.shape[2])
    nz[:, :, :Fn] = noise[:, :, :Fn]
    ns = np.broadcast_to(_f32_as_f64(noise_scale), (B,))
    m, e = np.zeros((B, C, F), np.float64), np.zeros((B, C, F), np.float64)
    for b in range(B):
        idx = np.repeat(np.arange(T), np.asarray(dur[b], np.int64))
        n = len(idx)
        assert n <= F and max(n, 1) == int(ylen[b]), (b, n, int(ylen[b]), F)
        m[b, :, :n] = m_p[b][:, idx]
        e[b, :, :n] = nz[b, :, :n] * np.exp(logs_p[b][:, idx]) * ns[b]
        e[b, :, n:] = nz[b, :, n:] * ns[b]
    return (m, e) if parts else m + e


def post_conv_ref(x, w, slope, vlen=None, hop=1, acc=False):
    """models.py:364-366: out[b, t] = tanh(sum_c sum_k w[c, k] * leaky_relu(x, slope)[b, c, t - pad + k]), pad = (K - 1) // 2,
    zeros outside [0, T); zeros at and behind vlen[b] * hop.  x [B, C, T], w [C, K] -> float64 [B, T] (acc=True: the sum under
    the tanh, not zeroed)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, C, T = x.shape
    K = w.shape[1]
    pad = (K - 1) // 2
    a = np.where(x > 0, x, x * np.float64(np.float32(slope)))
    ap = np.zeros((B, C, T + K - 1), np.float64)
    ap[:, :, pad:pad + T] = a
    s = np.zeros((B, T), np.float64)
    for k in range(K):
        s += np.einsum("c,bct->bt", w[:, k], ap[:, :, k:k + T])
    if acc:
        return s
    out = np.tanh(s)
    if vlen is not None:
        for b in range(B):
            out[b, int(vlen[b]) * hop:] = 0
    return out
