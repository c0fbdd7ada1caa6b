"""What one launch of the f32 conv engine has to compute, in float64 numpy: the operation, not the kernel.

    value = act(conv(pro(x)) + bias + bias_b[b])            then the rule of the flags

The rules are those the EPI_* enum of conv_engine.hip.hpp documents and the module formulas it cites:
  mask      value * (t < len[b]), BEFORE a residual is added (attentions.py FFN: x = x + ffn(x) * mask)
  res       + res[b, co, t]
  acc       + the previous contents of out          } the multi-receptive-field sum of the generator:
  div       / div, after the accumulation           } xs = (rb_0(x) + rb_1(x) + ..) / nk
  coupling  out = (out - value * mask) * mask       (modules.py:464, mean-only coupling, reverse)
  wn        the WN layer's update folded into its res_skip conv (modules.py:200-209): rows [0, wn_split) are the residual
            half, x = (x + value * mask); rows [wn_split, Cout) the skip half, skip = skip + value * mask - stored, not
            added, by the first layer (wn_first).  wn_split = 0 is the last layer, whose rows are all skip rows.
  oslope    what `out` stores is leaky_relu(v, oslope), what `out2` stores leaky_relu(v, oslope2): the producer-side
            activation of the generator (a tensor needed raw and activated is stored twice)
Besides the expected tensors the reference says which elements the launch OWNS (must have written): the conv's rows of the
output window, their pitch columns included (those read +0.0); everything else keeps what it held.
"""
import numpy as np

FLAG_NAMES = ("pro_lrelu", "pro_mask", "relu", "mask", "res", "acc", "div", "coupling", "wn", "wn_first")


def lrelu(v, slope):
    return np.where(v >= 0, v, v * slope)


def conv1d(x, w, dil, pad_l):
    """Conv1d, w [Cout, Cin, K], output length = input length, zero padding pad_l on the left"""
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    xp = np.zeros((B, Cin, T + dil * (K - 1)), np.float64)
    xp[:, :, pad_l:pad_l + T] = x
    y = np.zeros((B, Cout, T), np.float64)
    for k in range(K):
        y += np.einsum("oc,bct->bot", w[:, :, k], xp[:, :, k * dil:k * dil + T])
    return y


def conv_transpose1d(x, w, stride):
    """ConvTranspose1d, w [Cin, Cout, K], padding (K - stride) / 2: output length T * stride"""
    B, Cin, T = x.shape
    _, Cout, K = w.shape
    p = (K - stride) // 2
    assert K - 2 * p == stride
    full = np.zeros((B, Cout, (T - 1) * stride + K), np.float64)
    for k in range(K):
        full[:, :, k:k + (T - 1) * stride + 1:stride] += np.einsum("co,bct->bot", w[:, :, k], x)
    return full[:, :, p:p + T * stride]


def conv_epi_ref(x, w, bias=None, flags=(), dil=1, pad_l=None, stride=1, lens=None, bias_b=None, res=None, old_out=None,
                 old_out2=None, out2=False, slope=0.1, div=1.0, oslope=1.0, oslope2=1.0, wn_split=0, out_cstride=0,
                 out_rows=0, out_row0=0, pl_rows=0, sentinel=0.0, **_launch_only):
    """-> dict(out, out2, planes, own, own2): expected tensors [B, out_rows, pitch] (float64; sentinel / old contents where
    the launch owns nothing), expected planes [B, pl_rows, T], and the ownership masks of out and out2."""
    assert set(flags) <= set(FLAG_NAMES), flags
    f = set(flags)
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, Cin, T = x.shape
    Cout, K = (w.shape[1] if stride > 1 else w.shape[0]), w.shape[2]
    Tout = T * stride
    lens = np.full(B, T) if lens is None else np.asarray(lens)
    m = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)[:, None, :]  # [B, 1, T]
    assert stride == 1 or not (f & {"mask", "coupling", "wn"}), "no call site masks the output of a transposed conv"
    # ---- value
    xin = x * m if "pro_mask" in f else x
    if "pro_lrelu" in f:
        xin = lrelu(xin, slope)
    if stride > 1:
        v = conv_transpose1d(xin, w, stride)
    else:
        v = conv1d(xin, w, dil, dil * (K - 1) // 2 if pad_l is None else pad_l)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :, None]
    if bias_b is not None:
        v = v + np.asarray(bias_b, np.float64)[:, :Cout, None]
    if "relu" in f:
        v = np.maximum(v, 0.0)
    # ---- the buffers as the launch finds them
    rows, pitch = out_rows or Cout, out_cstride or Tout
    has2 = out2 or old_out2 is not None or "wn" in f

    def image(old):
        a = np.full((B, rows, pitch), np.float64(np.float32(sentinel)))
        if old is not None:
            a[:, :, :Tout] = old
        return a

    out, o2 = image(old_out), (image(old_out2) if has2 else None)
    own = np.zeros((B, rows, pitch), bool)
    own2 = np.zeros((B, rows, pitch), bool) if has2 else None
    prev, prev2 = out.copy(), (o2.copy() if has2 else None)
    planes = None
    # ---- the rule
    vm = v * m if ("mask" in f or "coupling" in f) else v
    if "wn" in f:
        assert out_row0 == 0 and not (f & {"res", "acc", "div", "coupling"})
        H, S = wn_split, Cout - wn_split
        out[:, :H, :Tout] = prev[:, :H, :Tout] + vm[:, :H]                 # x = x + res * mask
        o2[:, :S, :Tout] = vm[:, H:] if "wn_first" in f else prev2[:, :S, :Tout] + vm[:, H:]   # skip (+)= skip half * mask
        out[:, :H, Tout:], o2[:, :S, Tout:] = 0.0, 0.0
        own[:, :H], own2[:, :S] = True, True
        stored = out[:, :H, :Tout]
    else:
        r0, r1 = out_row0, out_row0 + Cout
        if "coupling" in f:
            assert not has2 and not (f & {"res", "acc", "div"})
            val = (prev[:, r0:r1, :Tout] - vm) * m
            out[:, r0:r1, :Tout] = val
        else:
            val = vm
            if "res" in f:
                val = val + np.asarray(res, np.float64)[:, :, :Tout]
            if "acc" in f:
                val = val + prev[:, r0:r1, :Tout]
            if "div" in f:
                val = val / div
            out[:, r0:r1, :Tout] = lrelu(val, oslope)
            if has2:
                o2[:, r0:r1, :Tout] = lrelu(val, oslope2)
                o2[:, r0:r1, Tout:] = 0.0
                own2[:, r0:r1] = True
        out[:, r0:r1, Tout:] = 0.0
        own[:, r0:r1] = True
        stored = out[:, r0:r1, :Tout]
    if pl_rows:
        planes = stored[:, :pl_rows].copy()
    return {"out": out, "out2": o2, "planes": planes, "own": own, "own2": own2}
