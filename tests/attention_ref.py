"""The relative-position self-attention core (attentions.py:215-272, as attention16.hip.hpp and kernels.hip.hpp cite it) in
plain NumPy: the float64 reference of the attention kernel tests, the same formula in float32 (its error against float64 sets
the tests' tolerance), the value of a pair of fp16 operand planes, and the structured inputs whose answers are known in
closed form.

    logits[i, j] = q_i . k_j / sqrt(dk) + q_i . E_k[j - i + w] / sqrt(dk)   (the second term where |j - i| <= w)
    keys j >= len: logit -1e4;  p = softmax over all T keys
    out[:, i]    = sum_j p[i, j] v_j + sum_m p[i, i + m - w] E_v[m]         (m with 0 <= i + m - w < T)
    queries i >= len: zeros (what both kernels write; the graph's values there never reach a valid output)
"""
import numpy as np


def _attention(qkv, n_heads, rel_k, rel_v, lens, dtype):
    qkv = np.asarray(qkv, dtype)
    rel_k = np.asarray(rel_k, dtype)
    rel_v = np.asarray(rel_v, dtype)
    B, C3, T = qkv.shape
    C = C3 // 3
    dk = C // n_heads
    nrel = rel_k.shape[0]
    w = (nrel - 1) // 2
    assert C3 == 3 * C and C == dk * n_heads and rel_k.shape == rel_v.shape == (2 * w + 1, dk)
    out = np.zeros((B, C, T), dtype)
    rsq = dtype(1) / np.sqrt(dtype(dk))
    for b in range(B):
        L = int(min(max(int(lens[b]), 0), T))
        if L == 0:
            continue
        for h in range(n_heads):
            q = qkv[b, h * dk:(h + 1) * dk, :L]            # [dk, L]: valid queries only
            k = qkv[b, C + h * dk:C + (h + 1) * dk]        # [dk, T]
            v = qkv[b, 2 * C + h * dk:2 * C + (h + 1) * dk]
            s = (q.T @ k) * rsq                            # [L, T]
            rq = (q.T @ rel_k.T) * rsq                     # [L, 2 w + 1]
            i = np.arange(L)
            for m in range(nrel):
                j = i + m - w
                ok = (j >= 0) & (j < T)
                s[i[ok], j[ok]] += rq[ok, m]
            s[:, L:] = dtype(-1e4)
            s -= s.max(axis=1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=1, keepdims=True)
            o = p @ v.T                                    # [L, dk]
            for m in range(nrel):
                j = i + m - w
                ok = (j >= 0) & (j < T)
                o[ok] += p[i[ok], j[ok]][:, None] * rel_v[m][None, :]
            out[b, h * dk:(h + 1) * dk, :L] = o.T
    return out


def attention_ref(qkv, n_heads, rel_k, rel_v, lens):
    """float64 reference: qkv [B, 3C, T], rel_k / rel_v [2w+1, dk], lens [B] -> [B, C, T]"""
    return _attention(qkv, n_heads, rel_k, rel_v, lens, np.float64)


def attention_ref_f32(qkv, n_heads, rel_k, rel_v, lens):
    """the same formula with every operation in float32: what plain fp32 arithmetic makes of these inputs"""
    return _attention(qkv, n_heads, rel_k, rel_v, lens, np.float32)


ORDINARY_CEILING = (2e-5, 1e-4)   # (atol, rtol) of the first attention tests: no bound may exceed them
SHARP_CEILING = (1e-4, 1e-4)      # ... for inputs with sharp softmaxes


def tolerance(want, f32, sharp=False):
    """The tests' bound on |kernel - float64|, per element, for one case: 8 x the largest error of the float32 evaluation on
    the same input, at least 2^-22 max|want|, and nowhere above the ceiling atol + rtol |want|.  The 8 covers what the kernels
    do differently from a plain fp32 evaluation: online softmax over 32-key blocks (two halves merged in the fp32 kernel),
    the hardware exp2, and f16x3's 3 * 2^-24 per product against fp32's 2^-24.  Returns (bound array, the scalar before the
    ceiling)."""
    want = np.asarray(want, np.float64)
    e32 = float(np.abs(np.asarray(f32, np.float64) - want).max()) if want.size else 0.0
    scalar = max(8.0 * e32, 2.0 ** -22 * (float(np.abs(want).max()) if want.size else 0.0))
    atol, rtol = SHARP_CEILING if sharp else ORDINARY_CEILING
    return np.minimum(scalar, atol + rtol * np.abs(want)), scalar


def planes_value(pl):
    """fp16 operand planes [B, 3, C/8, T, 8] (f16x3 format: h0, h1 * 2^11) -> the fp32 values they stand for [B, C, T]"""
    h = pl.view(np.float16).astype(np.float64)
    v = h[:, 0] + h[:, 1] / 2048.0
    B, CG, T, _ = v.shape
    return v.transpose(0, 1, 3, 2).reshape(B, CG * 8, T)


def split_planes(x):
    """fp32 [B, C, T] (C % 8 == 0) -> its operand planes uint16 [B, 3, C/8, T, 8] as the device split writes the first two
    slots (h0 = f16(x) clamped to +-65504, h1 = f16((x - h0) * 2^11)); the third slot is zero"""
    x = np.clip(np.asarray(x, np.float32), -65504.0, 65504.0)
    B, C, T = x.shape
    h0 = x.astype(np.float16)
    h1 = ((x - h0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    pl = np.zeros((B, 3, C // 8, T, 8), np.uint16)
    for s, h in enumerate((h0, h1)):
        pl[:, s] = h.reshape(B, C // 8, 8, T).transpose(0, 1, 3, 2).view(np.uint16)
    return pl


# ---- structured inputs with closed-form answers (the band tests)

BAND_LOGIT = 64.0  # the one logit that is not zero: every other key then holds e^-64 of the mass


def band_one_hot(dk, n_heads, window, m_star, L, T, rng, v_zero=False, chan=0):
    """k = 0; q = 8 on channel `chan` of every head; E_k[m_star] on that channel such that the logit of key i + m_star - w is
    BAND_LOGIT (every other logit is 0: the remaining channels of E_k are unit-scale noise that q never meets); unit-scale
    V (or zeros: the relative-value term alone) and E_v.  Returns qkv [1, 3C, T], rel_k, rel_v, lens."""
    C = dk * n_heads
    nrel = 2 * window + 1
    qkv = np.zeros((1, 3 * C, T), np.float32)
    for h in range(n_heads):
        qkv[0, h * dk + chan] = 8.0
    if not v_zero:
        qkv[0, 2 * C:] = rng.standard_normal((C, T)).astype(np.float32)
    rel_k = rng.standard_normal((nrel, dk)).astype(np.float32)
    rel_k[:, chan] = 0.0
    rel_k[m_star, chan] = np.float32(BAND_LOGIT * np.sqrt(dk) / 8.0)
    rel_v = rng.standard_normal((nrel, dk)).astype(np.float32)
    return qkv, rel_k, rel_v, np.asarray([L], np.int64)


def band_one_hot_closed_form(qkv, n_heads, rel_k, rel_v, lens, m_star):
    """what band_one_hot's input gives, without a softmax: V[:, j*] + E_v[m_star] where key j* = i + m_star - w exists
    (0 <= j* < len), else the uniform average of V over the valid keys plus the average of E_v over the band's valid keys
    (both up to the e^-64 that the other keys hold)"""
    qkv = np.asarray(qkv, np.float64)
    B, C3, T = qkv.shape
    C = C3 // 3
    dk = C // n_heads
    w = (rel_k.shape[0] - 1) // 2
    L = int(min(int(lens[0]), T))
    out = np.zeros((B, C, T))
    for h in range(n_heads):
        v = qkv[0, 2 * C + h * dk:2 * C + (h + 1) * dk]
        for i in range(L):
            j = i + m_star - w
            if 0 <= j < L:
                o = v[:, j] + rel_v[m_star]
            else:
                o = v[:, :L].mean(axis=1)
                for m in range(2 * w + 1):
                    if 0 <= i + m - w < L:
                        o = o + rel_v[m].astype(np.float64) / L
            out[0, h * dk:(h + 1) * dk, i] = o
    return out


# ---- the input families of the kernel tests (shared by the CPU test of this reference and the GPU tests)

def random_case(seed, B, n_heads, dk, T, window=4, rel_scale=None):
    """unit-scale q | k | v and E_k, E_v at `rel_scale` (default dk^-0.5, what a trained voice holds; 1.0 = unit scale, at which
    one wrong band entry moves an output by O(1))"""
    rng = np.random.default_rng(seed)
    C = n_heads * dk
    s = dk ** -0.5 if rel_scale is None else rel_scale
    qkv = rng.standard_normal((B, 3 * C, T)).astype(np.float32)
    rel_k = (rng.standard_normal((2 * window + 1, dk)) * s).astype(np.float32)
    rel_v = (rng.standard_normal((2 * window + 1, dk)) * s).astype(np.float32)
    return qkv, rel_k, rel_v


RESCALE_KINDS = ("growing", "falling", "band", "last_block", "jumps_late")


def rescale_case(kind, seed, n_heads, dk, L, T, window=4):
    """Where the running maximum of the online softmax moves: logits growing along the keys by 0.125 a key (it moves in every
    32-key block), falling (never after the first), the maximum inside the band (the relative-key logits carry it), in the
    last, partly masked block (with larger values still behind len, which the mask must hide), and late in the sweep on top of
    sharp logits (the first attention tests' case).  One utterance of length L in T columns."""
    qkv, rel_k, rel_v = random_case(seed, 1, n_heads, dk, T, window, rel_scale=1.0)
    C = n_heads * dk
    rt = np.float32(np.sqrt(dk))
    j = np.arange(T, dtype=np.float32)
    for h in range(n_heads):
        q0, k0 = h * dk, C + h * dk
        if kind in ("growing", "falling"):
            qkv[0, q0] = 1.0
            qkv[0, k0] = (0.125 if kind == "growing" else -0.125) * rt * j
        elif kind == "band":
            qkv[0, q0] = 2.0
            rel_k[:, 0] = rt * np.linspace(2.0, 6.0, 2 * window + 1, dtype=np.float32)
        elif kind == "last_block":
            qkv[0, q0] = 2.0
            qkv[0, k0, max(0, L - 3):L] = 5.0 * rt
            qkv[0, k0, L:] = 50.0 * rt
        elif kind == "jumps_late":
            qkv[0, q0:q0 + dk] *= 6.0
            qkv[0, k0:k0 + dk, (3 * L) // 4:] *= 5.0
        else:
            raise ValueError(kind)
    return qkv, rel_k, rel_v, np.asarray([L], np.int64)
