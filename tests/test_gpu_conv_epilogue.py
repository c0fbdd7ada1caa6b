"""The f32 conv engine (csrc/conv_engine.hip.hpp) by value, launch by launch as the pipeline forms them: every tile
configuration at its edges, every prologue / epilogue rule, row pitches, the second output, the fp16 operand planes - and the
two gate kernels and the speaker-conditioning kernel of the flow's f32 path.

Each conv case is held to three things:
  1. the float64 reference of tests/conv_epi_ref.py, at the tolerance the project holds this engine to: 2e-5 * max|want|
     (3e-5 where Cin * K > 1024), max|want| >= 1; planes within 2e-5 * scale of the rows they copy;
  2. ownership: outside the reference's ownership mask every element keeps its bits (the sentinel or its old contents),
     every owned pitch column is +0.0;
  3. the epilogue bit for bit: the same packed conv (same tile, same chunk) launched plain - bias and per-utterance bias only,
     dense rows, x masked on the host where the case has PRO_MASK - then the flag's rule applied in numpy float32 in the order
     the EPI_* enum documents must equal the fused launch exactly (the summation order depends neither on the DMA width nor
     on a pitch).
"""
import re

import numpy as np
import pytest

from conv_epi_ref import conv_epi_ref

pytestmark = pytest.mark.gpu

BM = (32, 64, 128, 64, 32, 32)
BN = (512, 256, 128, 64, 128, 64)


# ---- csrc/conv_geom.hpp's stage arithmetic, to say which path a case took (the kernel's name gives tile, DMA width, KS)
def _stage(cfg, K, dil, pad_l, CK, vec4):
    halo = (K - 1) * dil
    if vec4:
        pad_la = (pad_l + 3) & ~3
        LW = BN[cfg] + pad_la + ((halo - pad_l + 3) & ~3)
        xs = (CK * LW + 1023) // 1024 * 1024
    else:
        LW = BN[cfg] + halo
        xs = (CK * LW + 255) // 256 * 256
    return xs, xs + (BM[cfg] // 32) * (K * CK // 8) * 256


def _cap(cfg):
    return 6144 if cfg == 5 else (9728 if cfg <= 2 else 4864)


def _largest_ck(cfg, K, dil, pad_l):
    return next(ck for ck in (32, 16, 8) if _stage(cfg, K, dil, pad_l, ck, True)[1] <= _cap(cfg))


def _template_args(kernel):
    m = re.fullmatch(r"conv_engine_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>", kernel)
    assert m, kernel
    return dict(zip(("MW", "NW", "WM", "WN", "VEC", "ACT", "KS"), map(int, m.groups())))


def _reach(got, Cin, Cout, K, dil, pad_l, wn_split=0):
    """what the launch reached, from its name and the stage arithmetic"""
    t = _template_args(got["kernel"])
    cfg, ck = got["cfg"], got["ck"]
    assert (t["WM"] * t["MW"] * 32, t["WN"] * t["NW"] * 32) == ((BM[cfg], BN[cfg]) if t["KS"] == 1 else (32, 64)), (got, t)
    xs, _ = _stage(cfg, K, dil, pad_l, ck, t["VEC"] == 4)
    return {"cfg": cfg, "ck": ck, "vec": t["VEC"], "ks": t["KS"], "fastx": xs // (256 * t["VEC"]) <= 4 and Cin % ck == 0,
            "partial_chunk": Cin % ck != 0, "dead_rows": Cout % BM[cfg] != 0,
            "split_inside_tile": wn_split % BM[cfg] != 0}


# ---- the rules in float32, in the order the EPI_* enum documents them, applied to a plain launch's result
def _lrelu32(v, slope):
    return np.where(v >= 0, v, v * np.float32(slope))


def _rule32(plain, flags, mask, res, old, old2, div, oslope, oslope2, wn_split):
    f = set(flags)
    v = np.maximum(plain, np.float32(0)) if "relu" in f else plain
    m = mask.astype(np.float32)
    if "coupling" in f:
        return (old - v * m) * m, None
    if "wn" in f:
        vm = v * m if "mask" in f else v
        H = wn_split
        skip = vm[:, H:] if "wn_first" in f else vm[:, H:] + old2[:, :vm.shape[1] - H]
        return old[:, :H] + vm[:, :H], skip
    if "mask" in f:
        v = v * m
    if "res" in f:
        v = v + res
    if "acc" in f:
        v = v + old
    if "div" in f:
        v = v / np.float32(div)
    return _lrelu32(v, oslope), _lrelu32(v, oslope2)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_case(name, x, w, bias, tol=2e-5, group=None, **kw):
    """one launch against the three assertions of the module docstring (every figure printed in front of its assertion,
    tagged with the call-site group); returns the hook's result"""
    from phoonnx_amd.session import CONV_EPI_SENTINEL, test_conv1d_epi
    got = test_conv1d_epi(x, w, bias, **kw)
    want = conv_epi_ref(x, w, bias, sentinel=CONV_EPI_SENTINEL, **kw)
    flags, stride = kw.get("flags", ()), kw.get("stride", 1)
    B, Cin, T = x.shape
    Cout = w.shape[1] if stride > 1 else w.shape[0]
    Tout = T * stride
    wn_split = kw.get("wn_split", 0)
    # 1. the float64 reference
    for o, own in (("out", "own"), ("out2", "own2")):
        if want[o] is None:
            assert got[o] is None, name
            continue
        sel = want[own].copy()
        sel[:, :, Tout:] = False
        if sel.any():
            scale = np.abs(want[o][sel]).max()
            assert scale >= 1, (name, o, scale)
            err = np.abs(got[o].astype(np.float64) - want[o])[sel].max()
            print(f"[{group or name}] {name}: {o} max err {err:.3e} = {err / scale:.2e} * scale (tolerance {tol:.0e} * {scale:.2f}); "
                  f"{got['kernel']} CK {got['ck']}")
            assert err <= tol * scale, (name, o, err, scale)
        # 2. ownership
        keep = ~want[own]
        assert np.array_equal(_bits(got[o])[keep], _bits(want[o])[keep]), (name, o, "an element the launch does not own changed")
        pitch_cols = want[own].copy()
        pitch_cols[:, :, :Tout] = False
        assert not want[o][pitch_cols].any() and np.array_equal(_bits(got[o])[pitch_cols], _bits(want[o])[pitch_cols]), \
            (name, o, "an owned pitch column is not +0.0")
    if want["planes"] is not None:
        scale = np.abs(want["planes"]).max()
        assert scale >= 1, (name, scale)
        err = np.abs(got["planes"].astype(np.float64) - want["planes"]).max()
        print(f"{name}: planes max err {err:.3e} = {err / scale:.2e} * scale")
        assert err <= 2e-5 * scale, (name, "planes", err, scale)
    # 3. the epilogue bit for bit
    lens = kw.get("lens")
    lens = np.full(B, T) if lens is None else np.asarray(lens)
    mask = (np.arange(T)[None, :] < lens[:, None])[:, None, :]
    xz = np.where(mask, x, np.float32(0)) if "pro_mask" in flags else x
    plain = test_conv1d_epi(xz, w, bias, bias_b=kw.get("bias_b"), dil=kw.get("dil", 1), pad_l=kw.get("pad_l"), stride=stride,
                            cfg=got["cfg"], ck=got["ck"])
    assert plain["kernel"].split(",")[:4] == got["kernel"].split(",")[:4], (plain["kernel"], got["kernel"])
    old = kw.get("old_out")
    r0 = kw.get("out_row0", 0)
    res = None if kw.get("res") is None else np.asarray(kw["res"], np.float32)[:, :, :Tout]
    e1, e2 = _rule32(plain["out"], flags, mask, res, None if old is None else np.asarray(old, np.float32)[:, r0:r0 + Cout],
                     kw.get("old_out2"), kw.get("div", 1.0), kw.get("oslope", 1.0), kw.get("oslope2", 1.0), wn_split)
    if "wn" in flags:
        assert np.array_equal(got["out"][:, :wn_split, :Tout], e1), (name, "residual rows differ from the rule on the plain conv")
        assert np.array_equal(got["out2"][:, :Cout - wn_split, :Tout], e2), (name, "skip rows differ from the rule on the plain conv")
    else:
        assert np.array_equal(got["out"][:, r0:r0 + Cout, :Tout], e1), (name, "out differs from the rule on the plain conv")
        if got["out2"] is not None:
            assert np.array_equal(got["out2"][:, r0:r0 + Cout, :Tout], e2), (name, "out2 differs from the rule on the plain conv")
    return got


def _data(seed, B, Cin, Cout, T, K, stride=1):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    shape = (Cin, Cout, K) if stride > 1 else (Cout, Cin, K)
    w = (r.standard_normal(shape) / np.sqrt(Cin * K)).astype(np.float32)
    return r, x, w, r.standard_normal(Cout).astype(np.float32)


def _n(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------ a. every tile configuration at its edges

@pytest.mark.parametrize("cfg", range(6))
def test_every_tile_configuration_at_its_edges(cfg):
    # the encoder's FFN epilogue (EPI_MASK | EPI_RES) on a ragged second time tile, a last M tile with rows behind Cout,
    # both halos live (K = 3, dilation 2); T = BN + 4 takes the 16-byte DMA, T = BN + 5 the 4-byte one; Cin = 64 is whole
    # chunks, Cin = 29 a partial last chunk on the per-round address path
    K, dil = 3, 2
    Cout = {32: 48, 64: 96, 128: 160}[BM[cfg]]
    ck = _largest_ck(cfg, K, dil, dil)
    for Cin, last_len in ((64, 0), (29, 1)):
        for T in (BN[cfg] + 4, BN[cfg] + 5):
            r, x, w, b = _data(cfg * 100 + Cin + T, 3, Cin, Cout, T, K)
            got = check_case(f"cfg{cfg} Cin{Cin} T{T}", x, w, b, group="tiles", flags=("mask", "res"), dil=dil, cfg=cfg, ck=ck,
                             lens=[T, T // 3, last_len], res=_n(r, 3, Cout, T))
            reach = _reach(got, Cin, Cout, K, dil, dil)
            print(f"cfg{cfg} Cin{Cin} T{T}: {reach}")
            assert (reach["cfg"], reach["ck"]) == (cfg, ck) and reach["dead_rows"]
            assert reach["vec"] == (4 if T % 4 == 0 else 1) and reach["ks"] == (4 if cfg == 5 else 1)
            assert reach["partial_chunk"] == (Cin == 29) and not (Cin == 29 and reach["fastx"])


def test_split_k_tile_on_the_shape_it_exists_for():
    # the encoder's deep FFN conv scaled down: Cin * K = 1152 products per output through cfg 5 as the token domain's hint
    # chooses it; twelve k-groups per chunk over four waves, every wave reduces, the two live ones store a 32 x 64 tile
    Cin, Cout, T, K = 384, 64, 70, 3
    r, x, w, b = _data(5, 3, Cin, Cout, T, K)
    got = check_case("split-K 384x3 -> 64", x, w, b, tol=3e-5, flags=("mask", "res"), hint=2, lens=[T, T // 3, 1], res=_n(r, 3, Cout, T))
    reach = _reach(got, Cin, Cout, K, 1, 1)
    print(reach)
    assert reach["cfg"] == 5 and reach["ks"] == 4


# ------------------------------------------------------------------ b. every epilogue rule, as the pipeline forms it

@pytest.mark.parametrize("flags", [("pro_mask", "relu"), ("pro_mask", "mask")])
def test_duration_predictor_convs_mask_their_input(flags):
    # dpp_conv1 / conv2 / proj: K = 3, the taps that reach across len[b] must see zeros; T % 4 == 0 and PRO_MASK still takes
    # the 4-byte DMA (a 16-byte piece would carry columns behind the length in)
    Cin, Cout, T, K = 64, 160, 68, 3
    r, x, w, b = _data(11, 3, Cin, Cout, T, K)
    lens = [T, T // 3, 1]
    got = check_case("duration " + "|".join(flags), x, w, b, group="duration", flags=flags, cfg=3, ck=8, lens=lens)
    assert _reach(got, Cin, Cout, K, 1, 1)["vec"] == 1
    # the masked input matters: column len - 1 of the second utterance differs from the conv of the unmasked input
    unmasked = conv_epi_ref(x, w, b, flags=tuple(f for f in flags if f != "pro_mask"), lens=lens)["out"]
    assert np.abs(got["out"][1, :, lens[1] - 1] - unmasked[1, :, lens[1] - 1]).max() > 1e-2


@pytest.mark.parametrize("case", ["o: res", "ffn1: relu|mask", "ffn2: mask|res"])
def test_encoder_epilogues(case):
    flags = tuple(case.split(": ")[1].split("|"))
    K = 1 if case.startswith("o") else 3
    Cin, Cout, T = 96, 96, 70
    r, x, w, b = _data(21 + K, 3, Cin, Cout, T, K)
    res = _n(r, 3, Cout, T) if "res" in flags else None
    got = check_case("encoder " + case, x, w, b, group="encoder", flags=flags, cfg=3, ck=8, lens=[T, T // 3, 0], res=res)
    if flags == ("mask", "res"):  # behind the length: the residual alone, bit for bit
        assert np.array_equal(got["out"][1, :, T // 3:], res[1, :, T // 3:]) and np.array_equal(got["out"][2], res[2])


@pytest.mark.parametrize("layer,planes", [("first", False), ("first", True), ("middle", False), ("middle", True), ("last", False)])
@pytest.mark.parametrize("cfg,T", [(3, 70), (2, 133), (2, 132)])   # (132: the 16-byte DMA in front of the same epilogue)
def test_flow_res_skip_update(cfg, T, layer, planes):
    # res_skip 1 x 1 conv with the WN update folded in: H = 96 residual rows into x, 96 skip rows into skip.  On both
    # tiles (64 and 128 rows) the split falls inside an M tile.  First layer: skip holds garbage and is stored; last: skip rows only, x keeps
    # every bit.  planes: the updated x once more as the next in-layer's fp16 operand planes (the last layer has no next
    # in-layer: no call site gives it planes, and its x rows store nothing a plane could copy)
    H = 96
    last = layer == "last"
    Cout, split = (H, 0) if last else (2 * H, H)
    r, x, w, b = _data(31 + cfg + T, 3, H, Cout, T, 1)
    old_x, old_skip = _n(r, 3, H, T), _n(r, 3, H, T) * (1e6 if layer == "first" else 1)
    flags = ("wn", "mask") + (("wn_first",) if layer == "first" else ())
    got = check_case(f"res_skip {layer} cfg{cfg}" + (" +planes" if planes else ""), x, w, b, group="flow", flags=flags, cfg=cfg,
                     ck=_largest_ck(cfg, 1, 1, 0), lens=[T, T // 3, 1], old_out=old_x, old_out2=old_skip, wn_split=split, out_rows=H,
                     pl_rows=H if planes else 0)
    reach = _reach(got, H, Cout, 1, 1, 0, split)
    print(reach)
    assert reach["split_inside_tile"] == (not last)  # row 96 of the 64-row tile 64..127, of the 128-row tile 0..127
    if last:
        assert np.array_equal(_bits(got["out"]), _bits(old_x))


def test_flow_in_layer_takes_the_speaker_bias_of_its_rows():
    # cd.wn[i].in on the f32 engine: no flags, bias_b = this layer's rows of the conditioning, whose rows are longer than Cout
    H, T, K = 96, 133, 5
    r, x, w, b = _data(41, 2, H, 2 * H, T, K)
    check_case("flow in-layer bias_b", x, w, b, group="flow", hint=1, bias_b=_n(r, 2, 4 * 2 * H))


def test_flow_pre_and_post():
    H, half, T = 96, 96, 133
    r, x, w, b = _data(51, 3, half, H, T, 1)
    lens = [T, T // 3, 0]
    check_case("flow pre mask +planes", x, w, b, group="flow", flags=("mask",), hint=1, lens=lens, pl_rows=H)
    # post: x1 = (x1 - post(skip) * mask) * mask where x1 is the upper half of z: a window of `half` rows in rows of 2 * half
    r, x, w, b = _data(52, 3, H, half, T, 1)
    z = _n(r, 3, 2 * half, T)
    got = check_case("flow post coupling", x, w, b, group="flow", flags=("coupling",), hint=1, lens=lens, old_out=z, out_rows=2 * half,
                     out_row0=half)
    assert np.array_equal(_bits(got["out"][:, :half]), _bits(z[:, :half]))


def test_generator_conv_pre_pitches():
    # conv_pre of run_generator_f32: z * y_mask, + cond(g), leaky_relu(0.1) stored; z's rows have the frame pitch, the output's
    # the next multiple of 4 (its pitch columns read 0: ups[0] reads them through the 16-byte DMA)
    Cin, Cout, T, K = 48, 96, 261, 7
    r, x, w, b = _data(61, 3, Cin, Cout, T, K)
    got = check_case("conv_pre", x, w, b, group="generator", flags=("pro_mask",), hint=0, lens=[T, T // 3, 0], bias_b=_n(r, 3, Cout),
                     oslope=0.1, x_cstride=T + 7, out_cstride=(T + 3) & ~3)
    assert got["out"].shape[2] == 264 and not _bits(got["out"][:, :, T:]).any()
    # ... and without lengths (ylen == nullptr): no prologue mask
    check_case("conv_pre unmasked", x, w, b, group="generator", hint=0, bias_b=_n(r, 3, Cout), oslope=0.1, x_cstride=T + 7,
               out_cstride=(T + 3) & ~3)


@pytest.mark.parametrize("cfg", [None, 3])
@pytest.mark.parametrize("u,K,Cin,Cout,T", [(2, 4, 96, 48, 69), (8, 16, 32, 16, 65)])
def test_generator_up_conv_on_the_transposed_form(u, K, Cin, Cout, T, cfg):
    # stg.up: pixel-shuffled dense conv, input rows at the pitch conv_pre left (a multiple of 4 > T: 16-byte DMA pieces that
    # reach into the zeroed pitch columns), out raw and out2 = leaky_relu(0.1)
    r, x, w, b = _data(71 + u, 2, Cin, Cout, T, K, stride=u)
    kw = {} if cfg is None else {"cfg": cfg, "ck": 8}
    got = check_case(f"up u{u} K{K} cfg{cfg}", x, w, b, group="generator", stride=u, hint=0, x_cstride=(T + 3) & ~3, out2=True,
                     oslope2=0.1, **kw)
    assert _template_args(got["kernel"])["VEC"] == 4


@pytest.mark.parametrize("form", ["c1: oslope", "step: res+out2", "mrf0: res", "mrf1: res|acc", "mrf2: res|acc|div"])
def test_generator_resblock_and_mrf_forms(form):
    # the ResBlock walk of run_generator_f32: c1 stores leaky_relu(0.1) for c2; a step stores the stream raw and activated;
    # the last steps form xs = (rb_0 + rb_1 + rb_2) / 3 (mrf_flags), the final one with the stage's output slope
    C, T, K, dil = 80, 261, 3, 3
    r, x, w, b = _data(81, 2, C, C, T, K)
    kw = {"c1: oslope": dict(oslope=0.1),
          "step: res+out2": dict(flags=("res",), res=_n(r, 2, C, T), out2=True, oslope2=0.1),
          "mrf0: res": dict(flags=("res",), res=_n(r, 2, C, T)),
          "mrf1: res|acc": dict(flags=("res", "acc"), res=_n(r, 2, C, T), old_out=_n(r, 2, C, T)),
          "mrf2: res|acc|div": dict(flags=("res", "acc", "div"), res=_n(r, 2, C, T), old_out=_n(r, 2, C, T), div=3.0, oslope=0.01)}[form]
    check_case("generator " + form, x, w, b, group="generator", hint=0, dil=dil, **kw)


# ------------------------------------------------------------------ what the hook refuses

def test_conv_epilogue_hook_refuses_what_the_engine_cannot_form():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import SessionError, test_conv1d_epi, test_wn_gate
    x, w = np.zeros((1, 32, 40), np.float32), np.zeros((64, 32, 1), np.float32)
    o2 = np.zeros((1, 64, 40), np.float32)
    for match, kw in (("wn_split", dict(flags=("wn",), old_out2=o2, wn_split=16)),
                      ("wn_split", dict(flags=("wn",), old_out2=o2, wn_split=96)),
                      ("needs out2", dict(flags=("wn",), wn_split=32)),
                      ("pl_rows", dict(pl_rows=24)),
                      ("pl_rows", dict(pl_rows=96)),
                      ("pl_rows", dict(flags=("wn",), old_out2=o2, wn_split=32, pl_rows=64)),
                      ("EPI_RES without res", dict(flags=("res",))),
                      ("x_cstride smaller", dict(x_cstride=39)),
                      ("out_cstride smaller", dict(out_cstride=36)),
                      ("beyond the last time tile", dict(cfg=3, ck=8, out_cstride=68)),
                      ("leave the output tensor", dict(out_rows=80, out_row0=32)),
                      ("lens outside", dict(flags=("mask",), lens=[41])),
                      ("bias_b rows", dict(bias_b=np.zeros((1, 48), np.float32))),
                      ("chunk of 8, 16 or 32", dict(cfg=3, ck=12)),
                      ("does not fit", dict(cfg=3, ck=32, dil=1))):
        if match == "does not fit":  # a stage beyond the tile's capacity: pick_tiling throws, the hook reports it
            kw["dil"] = 1
            wide = np.zeros((64, 32, 11), np.float32)
            with pytest.raises(SessionError, match=match):
                test_conv1d_epi(x, wide, None, **kw)
            continue
        with pytest.raises(SessionError, match=match):
            test_conv1d_epi(x, w, None, **kw)
    wt = np.zeros((32, 16, 4), np.float32)
    with pytest.raises(SessionError, match="transposed conv"):
        test_conv1d_epi(x, wt, None, stride=2, pl_rows=32)
    with pytest.raises(SessionError, match="dense rows"):
        test_conv1d_epi(x, wt, None, stride=2, out_cstride=84)
    with pytest.raises(SessionError, match="8 channels"):
        test_wn_gate(np.zeros((1, 12, 5), np.float32), blocked=True)
    # ... which the library refuses itself, whoever calls it
    a = _ffi.VitsTestConvEpiArgs()
    assert _ffi.load().vits_test_conv1d_epi(0, a) == -3 and "conv epilogue hook" in _ffi.last_error(None)
    # and what it accepts next to those runs
    got = test_conv1d_epi(x, w, None, cfg=3, ck=8, out_cstride=64, pl_rows=64)
    assert not got["out"].any() and not got["planes"].any()


# ------------------------------------------------------------------ d. the gate and the conditioning

@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("H", [8, 96])
def test_wn_gate_both_layouts_match_float64(H, T):
    from phoonnx_amd.session import test_wn_gate
    r = np.random.default_rng(H * 1000 + T)
    a = (r.standard_normal((2, 2 * H, T)) * 3).astype(np.float32)
    planted = np.array([20, -20, 90, -90, 0], np.float32)
    for i, v in enumerate(planted):       # every planted value on the tanh side against every one on the sigmoid side
        for j, s in enumerate(planted):
            a[(i + j) % 2, (i * 5 + j) % H, (i * 7 + j * 3) % T] = v
            a[(i + j) % 2, H + (i * 5 + j) % H, (i * 7 + j * 3) % T] = s
    a64 = a.astype(np.float64)
    want = np.tanh(a64[:, :H]) * (1.0 / (1.0 + np.exp(-a64[:, H:])))
    planar, blocked = test_wn_gate(a), test_wn_gate(a, blocked=True)
    for name, got in (("planar", planar), ("blocked", blocked)):
        assert np.isfinite(got).all(), name
        err = np.abs(got - want).max()
        print(f"gate {name} H{H} T{T}: max err {err:.2e} (tolerance 3e-6)")
        assert err <= 3e-6, (name, err)
    assert np.array_equal(_bits(planar), _bits(blocked))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("gin", [1, 512])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 384])
def test_cond_matvec_matches_float64_and_clamps_the_speaker_id(rows, gin, with_bias):
    from phoonnx_amd.session import test_cond_matvec
    r = np.random.default_rng(rows * 7 + gin)
    emb, W = _n(r, 3, gin), _n(r, rows, gin)
    bias = _n(r, rows) if with_bias else None
    sid = np.array([0, 2, -1, 7], np.int64)
    got = test_cond_matvec(emb, sid, W, bias)
    # the kernel clamps an id outside the table to its nearest row: -1 reads speaker 0, 7 reads speaker 2
    clamped = np.clip(sid, 0, 2)
    want = emb.astype(np.float64)[clamped] @ W.astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"cond rows{rows} gin{gin} bias{with_bias}: max err {err:.2e} = {err / scale:.2e} * scale")
    assert got.shape == (4, rows) and err <= 2e-5 * scale, (err, scale)
    assert np.array_equal(got[2], got[0]) and np.array_equal(got[3], got[1])
