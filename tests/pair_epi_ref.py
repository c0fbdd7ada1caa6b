"""What one launch of the fused ResBlock step (conv_sx_pair16() of csrc/vitsmi.hip -> conv_sx_pair16_kernel) has to compute,
in float64 numpy: the operation, not the kernel (tests/sx_epi_ref.py states the single-conv engine's launches the same way).

    end_b  = sx_ends(...)                       x is taken as zero at columns >= end_b, whatever it holds there
    c1     = conv(leaky_relu(x, s), w1, dil1) + b1
    PAIR  (a ResBlock1 step, modules.py:301-314):     mid = c1          res = x
    CHAIN (two ResBlock2 steps, modules.py:355-364):  mid = c1 + x      res = mid
    mid is zero at columns >= end_b (and < 0): c2 sees its zero padding there, not c1 evaluated there
    value  = conv(leaky_relu(mid, s), w2, dil2) + b2 + res, then + old_out (acc), then / div (div)
    the raw tensor stores value, the planes store leaky_relu(value, s)
Ownership: the columns < end_b of every row, in the raw tensor (with "raw" only: without it the raw tensor is at most the
accumulate operand and owns nothing) and in the planes (with "planes").

quantized=True evaluates the single-plane arithmetic's roundings (precision "f16"): the input plane is the fp16 of
leaky_relu(x, s) computed in float32, the weights are fp16 after a power-of-two scale that puts their largest magnitude in
[2^14, 2^15), the intermediate is one fp16 plane, the residual is the stored plane with the slope undone.  Products and sums
stay float64 (acc32=True: float32, to size what the kernel's accumulation order may move).
"""
import numpy as np

from conv_epi_ref import conv1d, lrelu
from sx_epi_ref import sx_ends

FLAG_NAMES = ("acc", "div", "raw", "planes")


def f16(v):
    """float32 values as one fp16 plane holds them (clamped to +-65504, as cvt1h_pair_pk clamps), as float64"""
    v = np.asarray(v, np.float32)
    return np.clip(v, np.float32(-65504), np.float32(65504)).astype(np.float16).astype(np.float64)


def f16_weights(w):
    """the single-plane arithmetic's weights (tests/test_gpu_parity.py _f16_operands), as float64"""
    w = np.asarray(w, np.float32)
    _, e = np.frexp(np.float32(np.abs(w).max()))
    mul = np.float32(2.0) ** (15 - int(e))
    return (w * mul).astype(np.float16).astype(np.float64) / float(mul)


def pair_epi_ref(x, w1, b1, w2, b2, flags=("raw",), dil1=1, dil2=1, chain=False, slope=0.1, div=1.0, old_out=None, lens=None,
                 rag_add=0, rag_mul=1, sentinel=0.0, quantized=False, acc32=False, res_x=None, **_launch_only):
    """-> dict(out, planes, own, own_pl, value, mid): the raw tensor and the planes [B, C, T] after the launch (float64; the
    sentinel or the old contents where the launch owns nothing; planes None without "planes"), their ownership masks, the
    value in front of the stores and the intermediate (zero behind the ends).  res_x: the x the residual is taken from, where
    it is not the conv's input itself (the kernel recovers it from the operand planes)."""
    f = set(flags)
    assert f <= set(FLAG_NAMES), flags
    if "div" in f and "acc" not in f:
        raise ValueError("div without acc: no call site forms it, the launcher refuses it")
    if "acc" in f and old_out is None:
        raise ValueError("acc without old_out")
    B, C, T = np.shape(x)
    K = np.shape(w1)[2]
    if K % 2 == 0:
        raise ValueError('even K: no "same" padding')
    ends = sx_ends(B, T, lens, rag_add, rag_mul)
    live = np.broadcast_to((np.arange(T)[None, :] < ends[:, None])[:, None, :], (B, C, T))
    ct = np.float32 if acc32 else np.float64
    bias = lambda b: 0.0 if b is None else np.asarray(b, ct)[None, :, None]

    def conv(xin, w, dil):
        if not acc32:
            return conv1d(xin, w, dil, dil * (K - 1) // 2)
        xp = np.zeros((B, C, T + dil * (K - 1)), np.float32)
        xp[:, :, dil * (K - 1) // 2:dil * (K - 1) // 2 + T] = xin
        y = np.zeros((B, C, T), np.float32)
        for k in range(K):
            y += np.einsum("oc,bct->bot", w[:, :, k].astype(np.float32), xp[:, :, k * dil:k * dil + T])
        return y

    if quantized:
        s32 = np.float32(slope)
        s = float(s32)
        x32 = np.asarray(x, np.float32)
        xa = f16(np.where(live, np.where(x32 >= 0, x32, x32 * s32), np.float32(0)))       # the stored input plane
        xz = np.where(xa >= 0, xa, xa * float(np.float32(1.0) / s32))                     # the residual the kernel recovers
        w1q, w2q = f16_weights(w1), f16_weights(w2)
        act_in = xa
        act_mid = lambda m: f16(lrelu(m, s).astype(np.float32))
    else:
        s = slope
        xz = np.where(live, np.asarray(x, np.float64), 0.0)
        w1q, w2q = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
        act_in = lrelu(xz, s)
        act_mid = lambda m: lrelu(m, s)
    rx = xz if res_x is None else np.where(live, np.asarray(res_x, np.float64), 0.0)
    c1 = conv(act_in.astype(ct), w1q, dil1) + bias(b1)
    mid = np.where(live, c1 + rx.astype(ct) if chain else c1, 0.0).astype(ct)
    res = mid if chain else rx.astype(ct)
    v = conv(act_mid(mid).astype(ct), w2q, dil2) + bias(b2) + res
    prev = np.full((B, C, T), np.float64(np.float32(sentinel)))
    if old_out is not None:
        prev[:] = np.asarray(old_out, np.float64)
    if "acc" in f:
        v = v + prev.astype(ct)
    if "div" in f:
        v = v / ct(div)
    v = v.astype(np.float64)
    own = live.copy() if "raw" in f else np.zeros((B, C, T), bool)
    out = np.where(own, v, prev)
    pl = own_pl = None
    if "planes" in f:
        own_pl = live.copy()
        pl = np.where(own_pl, lrelu(v, s), np.float64(np.float32(sentinel)))
    return {"out": out, "planes": pl, "own": own, "own_pl": own_pl, "value": v, "mid": mid.astype(np.float64)}
