"""What one generator-form launch of the split-operand conv engine has to compute, in float64 numpy: the operation, not the
kernel (conv_sx() of csrc/vitsmi.hip forms these launches; tests/conv_epi_ref.py states the f32 engine's the same way).

    end_b  = T                                           without lens
           = min(T, (len_b + add) * mul) for len_b > 0,  0 for len_b <= 0      (SxRagged: where utterance b's tensors end)
    x      is taken as zero at columns >= end_b, whatever it holds there
    value  = conv(leaky_relu(x, islope)) + bias + bias_b[b]
             then + res, then + old_out, then / div, in that order             (xs = (rb_0 + rb_1 + ..) / n of the generator)
    raw    stores leaky_relu(value, oslope), the planes leaky_relu(value, oslope2)
Ownership: the output columns < end_b * ups of every conv row, in the raw tensor and in the planes alike; nothing else is
owned, and with no_raw_store the raw tensor (then only the accumulate operand) owns nothing.
"""
import numpy as np

from conv_epi_ref import conv1d, conv_transpose1d, lrelu

FLAG_NAMES = ("res", "acc", "div", "no_raw_store")


def sx_ends(B, T, lens=None, rag_add=0, rag_mul=1):
    """-> [B] columns at which each utterance's tensors end"""
    if lens is None:
        return np.full(B, T, np.int64)
    lens = np.asarray(lens, np.int64)
    assert lens.shape == (B,)
    return np.where(lens > 0, np.minimum(T, (lens + rag_add) * rag_mul), 0)


def sx_epi_ref(x, w, bias=None, flags=(), dil=1, pad_l=None, stride=1, res=None, old_out=None, bias_b=None, div=1.0,
               oslope=1.0, oslope2=1.0, islope=1.0, raw=True, planes=False, lens=None, rag_add=0, rag_mul=1, sentinel=0.0,
               **_launch_only):
    """-> dict(out, planes, own, own_pl, value): expected raw tensor and planes [B, Cout, T * stride] (float64; the sentinel or
    the old contents where the launch owns nothing; None where the output does not exist), their ownership masks, and the
    value in front of the output slopes."""
    f = set(flags)
    assert f <= set(FLAG_NAMES), flags
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, Cin, T = x.shape
    Cout, K = (w.shape[1] if stride > 1 else w.shape[0]), w.shape[2]
    To = T * stride
    ends = sx_ends(B, T, lens, rag_add, rag_mul)
    live = np.arange(T)[None, :] < ends[:, None]                       # [B, T] input columns that exist
    xin = lrelu(np.where(live[:, None, :], x, 0.0), islope)
    if stride > 1:
        v = conv_transpose1d(xin, w, stride)
    else:
        v = conv1d(xin, w, dil, dil * (K - 1) // 2 if pad_l is None else pad_l)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :, None]
    if bias_b is not None:
        v = v + np.asarray(bias_b, np.float64)[:, :Cout, None]
    prev = np.full((B, Cout, To), np.float64(np.float32(sentinel)))
    if old_out is not None:
        prev[:] = np.asarray(old_out, np.float64)
    if "res" in f:
        v = v + np.asarray(res, np.float64)
    if "acc" in f:
        v = v + prev
    if "div" in f:
        v = v / div
    owned = np.broadcast_to((np.arange(To)[None, :] < (ends * stride)[:, None])[:, None, :], (B, Cout, To)).copy()
    out = own = pl = own_pl = None
    if raw:
        own = owned & ("no_raw_store" not in f)
        out = np.where(own, lrelu(v, oslope), prev)
    if planes:
        own_pl = owned.copy()
        pl = np.where(own_pl, lrelu(v, oslope2), np.float64(np.float32(sentinel)))
    return {"out": out, "planes": pl, "own": own, "own_pl": own_pl, "value": v}
