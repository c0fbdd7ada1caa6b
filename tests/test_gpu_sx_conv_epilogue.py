"""The split-operand conv engine (csrc/conv_sx_engine.hip.hpp, conv_sx_kernel) by value, launch by launch as conv_sx() forms
them: every (arithmetic, main loop, input form, run tile) at its edges, every epilogue the generator's call sites form,
per-utterance tensor ends, transposed convs with their zero-tap skip, the fp16 range guard.

Each case is held to three things (every measured figure is printed in front of its assertion):
  1. the float64 reference of tests/sx_epi_ref.py on the elements the launch owns, at the tolerances the project already holds
     this engine to:
       bf16x6 / f16x3 raw outputs   2e-5 * max|want|, max|want| >= 1 (the f32 engine's figure)
       f16x3 planes                 3e-7 relative to the float32 value they copy (absolute floor 2^-36, sx_split.hip.hpp)
       residual read from two planes  + 2^-22 |res| (the bound documented at SX_RES_PL)
       f16 (one plane)              against the float64 conv of the fp16-rounded operands: 3e-5 absolute on unit-scale
                                    outputs (+ 1e-5 relative), 2^-10 relative for the plane output - the figures of
                                    test_conv_sx_single_plane_mode_is_the_fp16_operand_product
  2. ownership: every raw or plane element outside the reference's mask keeps its bits - the sentinel or old_out;
  3. the epilogue bit for bit: the same packing on the same run tile launched plain (bias and bias_b only, raw output only, no
     slope), then + res, + old, / div, max(v, v * slope) in numpy float32 must equal the fused launch's raw output exactly, and
     the planes must be the split of that same float32 value.
"""
import re

import numpy as np
import pytest

from sx_epi_ref import sx_epi_ref

pytestmark = pytest.mark.gpu

SENT = -1234.5678
SX_BM = (128, 64, 32, 64)
SX_BN = (256, 256, 256, 128)
RES, ACC, DIV, HAS_RAW, HAS_PL, RAW_ACT, PL_ACT, BIASB, RES_EARLY, RES_PL = 16, 32, 64, 1 << 9, 1 << 10, 1 << 11, 1 << 12, 1 << 13, 1 << 14, 1 << 22
# the kSxEpi* constants of conv_sx_engine.hip.hpp
EPI = {"Planes": HAS_PL | PL_ACT, "Up": HAS_RAW | HAS_PL | PL_ACT, "Inner": RES | HAS_RAW | HAS_PL | PL_ACT, "First": RES | HAS_RAW,
       "Accum": RES | ACC | HAS_RAW, "Raw": HAS_RAW, "StageOut": RES | ACC | DIV | HAS_PL | PL_ACT, "InnerPl": RES | HAS_PL | PL_ACT,
       "AccumDiv": RES | ACC | DIV | HAS_RAW}
# the wave arrangement (MW, NW, WM, WN) of each run tile, per main loop (launch_conv_sx_f16_s16 / _s32 / _bf16 / _h1_s16)
TILE16 = {0: (1, 8, 4, 1), 1: (1, 4, 2, 2), 3: (1, 2, 2, 2), 2: (1, 2, 1, 4)}
TILE32 = {0: (2, 4, 2, 2), 1: (1, 4, 2, 2), 2: (1, 2, 1, 4)}


def _template_args(kernel):
    m = re.fullmatch(r"conv_sx_kernel<(\d+), (\d+), (\d+), (\d+), (-?\d+), (true|false), (true|false), (\d+), (\d+)>", kernel)
    assert m, kernel
    g = m.groups()
    return {"tile": tuple(map(int, g[:4])), "EPI": int(g[4]), "PROF": g[5] == "true", "RAWIN": g[6] == "true", "NP": int(g[7]),
            "SH": int(g[8])}


def _lrelu32(v, slope):
    return v if slope == 1.0 else np.maximum(v, v * np.float32(slope))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f16(v):
    return np.clip(v, np.float32(-65504), np.float32(65504)).astype(np.float16).astype(np.float32)


def _through_planes(v, precision):
    """float32 values as they read back from the operand planes the epilogue splits them into"""
    v = np.asarray(v, np.float32)
    if precision == "bf16x6":
        return v                                    # three bf16 planes hold the 24 bits exactly
    h0 = _f16(v)
    if precision == "f16":
        return h0
    c = np.clip(v, np.float32(-65504), np.float32(65504))
    h1 = ((c - h0) * np.float32(2048)).astype(np.float16).astype(np.float32)
    return h1 * np.float32(1.0 / 2048.0) + h0


def _f16_operands(x, w):
    """the single-plane arithmetic's operands (tests/test_gpu_parity.py _f16_operands), as float64"""
    _, e = np.frexp(np.float32(np.abs(w).max()))
    mul = np.float32(2.0) ** (15 - int(e))
    wq = (w * mul).astype(np.float16).astype(np.float64) / float(mul)
    return x.astype(np.float16).astype(np.float64), wq


WORST = {}


def _note(group, what, ratio, kernel):
    key = (group, what)
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, kernel)
    print(f"[{group}] worst so far {what}: {WORST[key][0]:.3f} x tolerance ({WORST[key][1]})")


def check_case(name, group, x, w, bias, want=None, **kw):
    """one launch against the three assertions of the module docstring; returns the hook's result"""
    from phoonnx_amd.session import test_conv1d_sx_epi
    precision = kw.get("precision", "f16x3")
    flags = set(kw.get("flags", ()))
    got = test_conv1d_sx_epi(x, w, bias, sentinel=SENT, **kw)
    k = got["kernel"]
    res32 = None
    if kw.get("res_is_x"):
        res32 = x
    elif kw.get("res_planes"):
        rs = got["res_seen"]
        unsl = np.float32(1.0) / np.float32(kw.get("res_slope", 1.0))
        res32 = np.where(rs < 0, rs * unsl, rs).astype(np.float32)
    elif kw.get("res") is not None:
        res32 = np.asarray(kw["res"], np.float32)
    # ---- 1. the float64 reference on owned elements
    if want is None:
        rkw = dict(kw)
        if precision == "f16":
            xq, wq = _f16_operands(x, w)
            if res32 is not None:
                rkw["res"] = res32.astype(np.float64)           # the residual as its fp16 plane holds it
        else:
            xq, wq = x, w
            if kw.get("res_is_x"):
                rkw["res"] = x
        want = sx_epi_ref(xq, wq, bias, sentinel=SENT, **rkw)
    extra = 0.0
    if precision == "f16x3" and kw.get("res_planes"):
        extra = 2.0 ** -22 * float(np.abs(np.asarray(kw["res"])).max())
    for o, own in (("out", "own"), ("planes", "own_pl")):
        if want[o] is None:
            assert got[o] is None, (name, o)
            continue
        sel = want[own]
        if sel.any():
            err = np.abs(got[o].astype(np.float64) - want[o])
            if precision == "f16":
                rtol = 1e-5 if o == "out" else 2.0 ** -10
                ratio = float((err[sel] / (3e-5 + rtol * np.abs(want[o][sel]))).max())
                print(f"[{group}] {name}: {o} max err {err[sel].max():.3e} = {ratio:.3f} x (3e-5 + {rtol:.1e} |want|); {k}")
            else:
                scale = float(np.abs(want[o][sel]).max())
                assert scale >= 1, (name, o, scale)
                ratio = float(err[sel].max() / (2e-5 * scale + extra))
                print(f"[{group}] {name}: {o} max err {err[sel].max():.3e} = {ratio:.3f} x (2e-5 * {scale:.2f} + {extra:.1e}); {k}")
            _note(group, f"{precision} {o} vs float64", ratio, k)
            assert ratio <= 1, (name, o, ratio)
        # ---- 2. ownership
        keep = ~sel
        held = want[o].astype(np.float32) if o == "out" else np.full(want[o].shape, _through_planes(np.float32(SENT), precision))
        assert np.array_equal(_bits(got[o])[keep], _bits(held)[keep]), (name, o, "an element the launch does not own changed")
    # ---- 3. the epilogue bit for bit
    pkw = {a: kw[a] for a in ("precision", "dil", "pad_l", "stride", "force16", "no_s16", "min_cfg", "bias_b", "islope", "lens",
                              "rag_add", "rag_mul") if a in kw}
    plain = test_conv1d_sx_epi(x, w, bias, sentinel=SENT, run_cfg=got["run_cfg"], **pkw)
    print(f"  plain launch reached {plain['kernel']}")
    tp, tg = _template_args(plain["kernel"]), _template_args(k)
    assert (plain["pack_cfg"], plain["run_cfg"]) == (got["pack_cfg"], got["run_cfg"]), (plain, got)
    assert all(tp[a] == tg[a] for a in ("tile", "RAWIN", "NP", "SH")), (plain["kernel"], k)
    v = plain["out"]
    if "res" in flags:
        v = v + res32
    if "acc" in flags:
        v = v + np.asarray(kw["old_out"], np.float32)
    if "div" in flags:
        v = v / np.float32(kw["div"])
    assert v.dtype == np.float32
    if got["out"] is not None and "no_raw_store" not in flags:
        e = _lrelu32(v, kw.get("oslope", 1.0))
        same = np.array_equal(_bits(got["out"])[want["own"]], _bits(e)[want["own"]])
        print(f"[{group}] {name}: raw output equals the rule on the plain launch bit for bit: {same}")
        assert same, (name, "raw", float(np.abs(got["out"] - e)[want["own"]].max()))
    if got["planes"] is not None:
        o2 = _lrelu32(v, kw.get("oslope2", 1.0))
        e = _through_planes(o2, precision)
        sel = want["own_pl"]
        same = np.array_equal(_bits(got["planes"])[sel], _bits(e)[sel])
        print(f"[{group}] {name}: planes are the split of the same float32 value bit for bit: {same}")
        assert same, (name, "planes", float(np.abs(got["planes"] - e)[sel].max()))
        if precision == "f16x3" and sel.any():   # ... and within 3e-7 relative of the float32 value they copy
            small = np.abs(o2) <= 65504
            rel = float((np.abs(got["planes"].astype(np.float64) - o2)[sel & small] / (3e-7 * np.abs(o2[sel & small]) + 2.0 ** -36)).max())
            print(f"[{group}] {name}: planes vs the float32 value they copy: {rel:.3f} x (3e-7 relative + 2^-36)")
            _note(group, "f16x3 planes vs the value they copy", rel, k)
            assert rel <= 1, (name, rel)
    got["want"] = want
    return got


def _data(seed, B, Cin, Cout, T, K, stride=1):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    shape = (Cin, Cout, K) if stride > 1 else (Cout, Cin, K)
    w = (r.standard_normal(shape) / np.sqrt(Cin * K / stride)).astype(np.float32)
    return r, x, w, r.standard_normal(Cout).astype(np.float32)


def _n(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


def _neg(r, *shape):
    """the `neg` pattern of tests/test_gpu_pair_single_read.py: leaky_relu(v) = 0.1 v there, so a residual taken behind the
    activation is off by 0.9 |v|"""
    v = _n(r, *shape)
    return np.where(r.random(shape) < 0.25, -np.abs(v) * np.float32(900.0) - np.float32(100.0), v).astype(np.float32)


def _inner_kw(precision, r, B, Cout, T, res=None):
    """the residual conv inside a block: residual, raw and planes with slope; the single-plane arithmetic reads the residual
    from its plane"""
    res = _n(r, B, Cout, T) if res is None else res
    kw = dict(flags=("res",), res=res, planes=True, oslope2=0.1)
    if precision == "f16":
        kw.update(res_planes=True, res_slope=0.1)
    return kw


def _expect_name(got, tiles, run, EPI_want, NP, SH, rawin):
    t = _template_args(got["kernel"])
    print(f"  reached {got['kernel']} (packed for cfg {got['pack_cfg']}, run on cfg {got['run_cfg']}, rawin {got['rawin']}, s16 {got['s16']}, "
          f"CK {got['ck']})")
    assert t["tile"] == tiles[run] and got["run_cfg"] == run, (got["kernel"], run)
    assert (t["EPI"], t["NP"], t["SH"], t["RAWIN"], t["PROF"]) == (EPI_want, NP, SH, rawin, False), (got["kernel"], EPI_want)
    assert t["tile"][0] * t["tile"][2] * 32 == SX_BM[run] and t["tile"][1] * t["tile"][3] * 32 == SX_BN[run]
    return t


# ------------------------------------------------------------------ a. every (arithmetic, loop, input form, run tile) at its edges

# (name, precision, Cin, Cout, packed cfg, run tiles, s16, rawin)
COMBOS = [
    ("f16x3 16x16x32 packed 128 rows", "f16x3", 128, 128, 0, (0, 1, 2, 3), True, False),
    ("f16x3 16x16x32 packed 64 rows", "f16x3", 128, 192, 1, (1, 3, 2), True, False),
    ("f16x3 16x16x32 packed 32 rows", "f16x3", 128, 96, 2, (2,), True, False),
    ("f16x3 32x32x16 packed 128 rows", "f16x3", 80, 128, 0, (0, 1, 2), False, False),
    ("f16x3 32x32x16 packed 64 rows", "f16x3", 80, 192, 1, (1, 2), False, False),
    ("f16x3 32x32x16 packed 32 rows", "f16x3", 80, 96, 2, (2,), False, False),
    ("bf16x6 packed 128 rows", "bf16x6", 80, 128, 0, (0, 1, 2), False, False),
    ("bf16x6 packed 64 rows", "bf16x6", 80, 192, 1, (1, 2), False, False),
    ("bf16x6 packed 32 rows", "bf16x6", 80, 96, 2, (2,), False, False),
    ("f16x3 raw input 64 ch cfg 1", "f16x3", 64, 64, 1, (1,), False, True),
    ("f16x3 raw input 64 ch cfg 2", "f16x3", 64, 96, 2, (2,), False, True),
    ("f16x3 raw input 16 ch cfg 1", "f16x3", 16, 64, 1, (1,), False, True),
    ("f16x3 raw input 16 ch cfg 2", "f16x3", 16, 96, 2, (2,), False, True),
    ("bf16x6 raw input 64 ch cfg 1", "bf16x6", 64, 64, 1, (1,), False, True),
    ("bf16x6 raw input 64 ch cfg 2", "bf16x6", 64, 96, 2, (2,), False, True),
    ("bf16x6 raw input 16 ch cfg 1", "bf16x6", 16, 64, 1, (1,), False, True),
    ("bf16x6 raw input 16 ch cfg 2", "bf16x6", 16, 96, 2, (2,), False, True),
    ("f16 single plane packed 128 rows", "f16", 128, 128, 0, (0, 1, 3, 2), True, False),
]


@pytest.mark.parametrize("combo", COMBOS, ids=[c[0] for c in COMBOS])
def test_every_arithmetic_loop_input_form_and_run_tile_at_its_edges(combo):
    # the residual conv inside a block (residual, raw, planes with slope; K = 3, dilation 2: both halos live) on a ragged second
    # time tile (T = BN + 5), on whole tiles (T = 2 BN) and on a tensor shorter than the halo (T = 3)
    name, precision, Cin, Cout, pack, runs, s16, rawin = combo
    K, dil, B = 3, 2, 2
    NP = {"f16x3": 2, "bf16x6": 6, "f16": 1}[precision]
    tiles = TILE16 if s16 else TILE32
    # (the raw-input and single-plane families have no instantiation of this epilogue: the generic kernel)
    epi = EPI["Inner"] if not rawin and precision != "f16" else -1
    for T in sorted({SX_BN[r] + 5 for r in runs} | {2 * SX_BN[r] for r in runs} | {3}):
        r, x, w, b = _data(Cin * 7 + Cout + T, B, Cin, Cout, T, K)
        kw = _inner_kw(precision, r, B, Cout, T)
        first = None
        for run in runs:
            got = check_case(f"{name} run {run} T{T}", "tiles", x, w, b, want=first["want"] if first else None, precision=precision,
                             dil=dil, run_cfg=run, **kw)
            assert (got["pack_cfg"], got["s16"], got["rawin"]) == (pack, s16, rawin), got
            _expect_name(got, tiles, run, epi, NP, 16 if s16 else 32, rawin)
            if first is None:
                first = got
            else:  # "same products in the same order": what chunked rendering's bit equality rests on
                same = np.array_equal(_bits(got["out"]), _bits(first["out"])) and np.array_equal(_bits(got["planes"]), _bits(first["planes"]))
                print(f"[tiles] {name} T{T}: run tile {run} equals run tile {runs[0]} bit for bit: {same}")
                assert same, (name, T, run, float(np.abs(got["out"] - first["out"]).max()))


# ------------------------------------------------------------------ b. every epilogue conv_sx()'s callers form

def _epilogue_kw(form, precision, r, B, C, T):
    """the call sites' launches by the name of their kSxEpi* constant; residuals carry the large negative values"""
    res = _neg(r, B, C, T)
    old = _n(r, B, C, T)
    rp = dict(res_planes=True, res_slope=0.1) if precision == "f16" else {}
    return {"Planes": dict(raw=False, planes=True, oslope2=0.1),
            "Up": dict(planes=True, oslope2=0.1),
            "Inner": dict(flags=("res",), res=res, planes=True, oslope2=0.1, **rp),
            "First": dict(flags=("res",), res=res, **rp),
            "Accum": dict(flags=("res", "acc"), res=res, old_out=old, **rp),
            "AccumDiv": dict(flags=("res", "acc", "div"), res=res, old_out=old, div=3.0, **rp),
            "Raw": dict(),
            "StageOut": dict(flags=("res", "acc", "div", "no_raw_store"), res=res, old_out=old, div=3.0, planes=True, oslope2=0.1, **rp),
            "InnerPl": dict(flags=("res",), res=res, raw=False, planes=True, oslope2=0.1, **rp)}[form]


PLANE_FAMILIES = {"f16x3 16x16x32": ("f16x3", 128, TILE16, 2, 16), "f16x3 32x32x16": ("f16x3", 80, TILE32, 2, 32),
                  "bf16x6": ("bf16x6", 80, TILE32, 6, 32)}


@pytest.mark.parametrize("form", ["Planes", "Up", "Inner", "First", "Accum", "Raw", "StageOut", "InnerPl"])
@pytest.mark.parametrize("family", list(PLANE_FAMILIES))
def test_generator_epilogues_on_plane_input(family, form):
    # launch_conv_sx_epi's instantiations on every tile of the family (a 128-row packing read by each run tile); InnerPl has
    # none outside the plane-stream generator: the generic kernel.  StageOut: the raw tensor is the accumulate operand only and
    # keeps every bit
    precision, Cin, tiles, NP, SH = PLANE_FAMILIES[family]
    B, C, T, K, dil = 2, 128, 261, 3, 2
    r, x, w, b = _data(len(form) * 31 + Cin, B, Cin, C, T, K)
    kw = _epilogue_kw(form, precision, r, B, C, T)
    first = None
    for run in tiles:
        got = check_case(f"{family} {form} run {run}", "epilogues", x, w, b, want=first["want"] if first else None, precision=precision,
                         dil=dil, run_cfg=run, **kw)
        _expect_name(got, tiles, run, -1 if form == "InnerPl" else EPI[form], NP, SH, False)
        if form == "StageOut":
            assert np.array_equal(_bits(got["out"]), _bits(kw["old_out"]))
        first = first or got
        for o in ("out", "planes"):
            assert got[o] is None or np.array_equal(_bits(got[o]), _bits(first[o])), (family, form, run, o)


@pytest.mark.parametrize("form", ["InnerPl", "First", "Accum", "StageOut"])
def test_residual_read_from_two_planes(form):
    # the plane-stream generator (SX_RES_PL, launch_conv_sx_s16p_epi): the residual is the operand planes of leaky_relu(res, 0.1),
    # un-activated on the way in - a residual taken behind the activation would be off by 0.9 |res| on the negative values
    B, C, T, K, dil = 2, 128, 261, 3, 2
    r, x, w, b = _data(len(form) * 37, B, C, C, T, K)
    kw = _epilogue_kw(form, "f16x3", r, B, C, T)
    kw.update(res_planes=True, res_slope=0.1)
    first = None
    for run in TILE16:
        got = check_case(f"res from planes {form} run {run}", "residual planes", x, w, b, want=first["want"] if first else None,
                         precision="f16x3", dil=dil, run_cfg=run, **kw)
        _expect_name(got, TILE16, run, EPI[form] | RES_PL, 2, 16, False)
        first = first or got
        for o in ("out", "planes"):
            assert got[o] is None or np.array_equal(_bits(got[o]), _bits(first[o])), (form, run, o)
    # the planes hold the residual to 22 bits: the split's documented 2^-22 |v| with its absolute floor of 2^-36 below
    # |v| = 2^-14 (sx_split.hip.hpp), v = leaky_relu(res, 0.1f) rounded to float32 (2^-24) and multiplied back by the float32
    # 1 / 0.1f (its own error and the product's rounding: 2 * 2^-24; the floor grows by that factor of 10)
    seen = np.where(first["res_seen"] < 0, first["res_seen"] * (np.float32(1) / np.float32(0.1)), first["res_seen"])
    bound = (2.0 ** -22 + 3 * 2.0 ** -24) * np.abs(kw["res"]) + 10 * 2.0 ** -36
    ratio = float((np.abs(seen.astype(np.float64) - kw["res"]) / bound).max())
    print(f"[residual planes] {form}: residual as read from its planes: {ratio:.3f} x ((2^-22 + 3 * 2^-24) |res| + 10 * 2^-36)")
    assert ratio <= 1, ratio
    # on the 32x32x16 loop there is no such instantiation: the generic kernel reads the planes
    r, x, w, b = _data(5, B, 80, C, T, K)
    got = check_case(f"res from planes {form} 32x32x16", "residual planes", x, w, b, precision="f16x3", dil=dil, **kw)
    _expect_name(got, TILE32, 0, -1, 2, 32, False)


@pytest.mark.parametrize("form", ["First", "Accum", "AccumDiv"])
@pytest.mark.parametrize("precision,C,cfg", [("f16x3", 64, 1), ("f16x3", 32, 2), ("bf16x6", 32, 2), ("bf16x6", 64, 1)])
def test_resblock2_residual_is_the_raw_input(precision, C, cfg, form):
    # x = conv(leaky_relu(x)) + x on a raw-format stage: the residual is requested in the prologue (SX_RES_EARLY) - except
    # bf16x6 on the 64-row tile, which has no registers for it: First / Accum read it in the epilogue, Accum|Div runs generic
    B, T, K, dil = 2, 261, 3, 2
    r, _, w, b = _data(C + cfg + len(form), B, C, C, T, K)
    x = _neg(r, B, C, T)
    kw = _epilogue_kw(form, precision, r, B, C, T)
    kw.pop("res")
    got = check_case(f"{precision} C{C} {form} res = x", "residual = input", x, w, b, precision=precision, dil=dil, res_is_x=True, islope=0.1,
                     **kw)
    early = precision == "f16x3" or cfg == 2
    want_epi = EPI[form] | RES_EARLY if early else (-1 if form == "AccumDiv" else EPI[form])
    _expect_name(got, TILE32, cfg, want_epi, 2 if precision == "f16x3" else 6, 32, True)


@pytest.mark.parametrize("form", ["Planes", "InnerPl", "First", "Accum", "AccumDiv", "StageOut"])
def test_single_plane_epilogues(form):
    # launch_conv_sx_h1_epi's set on every tile: the stream is one fp16 plane, the residual is recovered from the plane that holds
    # leaky_relu(res, 0.1), the multi-receptive-field sum stays fp32
    B, C, T, K, dil = 2, 128, 261, 3, 2
    r, x, w, b = _data(len(form) * 41, B, C, C, T, K)
    kw = _epilogue_kw(form, "f16", r, B, C, T)
    first = None
    for run in TILE16:
        got = check_case(f"f16 {form} run {run}", "single plane", x, w, b, want=first["want"] if first else None, precision="f16", dil=dil,
                         run_cfg=run, **kw)
        _expect_name(got, TILE16, run, EPI[form], 1, 16, False)
        first = first or got
        for o in ("out", "planes"):
            assert got[o] is None or np.array_equal(_bits(got[o]), _bits(first[o])), (form, run, o)


def test_launches_without_an_instantiation_run_generic():
    B, T, K, dil = 2, 261, 7, 1
    # conv_pre: + cond(g) per utterance, leaky_relu(0.1) stored raw
    for family, (precision, Cin, tiles, NP, SH) in PLANE_FAMILIES.items():
        r, x, w, b = _data(77 + Cin, B, Cin, 128, T, K)
        got = check_case(f"conv_pre {family}", "generic", x, w, b, precision=precision, dil=dil, bias_b=_n(r, B, 160), oslope=0.1)
        _expect_name(got, tiles, 0, -1, NP, SH, False)
    # a residual that is not the input, on a raw-input conv.  First and Accum have raw-input instantiations that read the
    # residual in the epilogue (launch_conv_sx_rawin: the non-early cases); with the division there is none: generic
    for precision, NP, Cout, cfg in (("f16x3", 2, 64, 1), ("bf16x6", 6, 64, 1), ("f16x3", 2, 96, 2), ("bf16x6", 6, 96, 2)):
        r, x, w, b = _data(78 + NP + cfg, B, 64, Cout, T, 3)
        for form, want_epi in (("First", EPI["First"]), ("Accum", EPI["Accum"]), ("AccumDiv", -1)):
            kw = _epilogue_kw(form, precision, r, B, Cout, T)
            got = check_case(f"{precision} raw input cfg {cfg} {form} res != x", "generic", x, w, b, precision=precision, dil=2, islope=0.1,
                             **kw)
            _expect_name(got, TILE32, cfg, want_epi, NP, 32, True)


# ------------------------------------------------------------------ c. ragged ends

RAGGED = {"plane input": dict(precision="f16x3", Cin=128, Cout=128, stride=1, K=3, dil=2),
          "raw input": dict(precision="f16x3", Cin=64, Cout=64, stride=1, K=3, dil=2),
          "transposed": dict(precision="f16x3", Cin=128, Cout=64, stride=2, K=4, dil=1)}


@pytest.mark.parametrize("add,where", [(10, "inside the first tile"), (28, "on the seam of the first two tiles"), (50, "inside the second tile")])
@pytest.mark.parametrize("kind", list(RAGGED))
def test_ragged_ends_are_neither_read_nor_written(kind, add, where):
    # T = 600 input columns = 300 frames of 2 columns (mul = 2): the full utterance ends at T inside the third tile, the
    # second at (100 + add) * 2 = 220 / 256 / 300 columns, the third has no frames: its tiles start behind its end, nothing is
    # written.  x holds 1e3 behind every end: read, it would show in the owned columns
    c = RAGGED[kind]
    B, T, mul = 3, 600, 2
    lens = [300, 100, 0]
    u = c["stride"]
    r, x, w, b = _data(add + c["Cin"] + u, B, c["Cin"], c["Cout"], T, c["K"], stride=u)
    end = (100 + add) * mul
    assert end == {10: 220, 28: 256, 50: 300}[add]
    x[1, :, end:] = 1e3
    x[2] = 1e3
    if kind == "plane input":
        kw = _inner_kw("f16x3", r, B, c["Cout"], T)
    elif kind == "raw input":
        kw = dict(flags=("res",), res_is_x=True, islope=0.1)
    else:
        kw = dict(planes=True, oslope2=0.1)
    got = check_case(f"ragged {kind}, second utterance ends {where}", "ragged", x, w, b, precision=c["precision"], dil=c["dil"], stride=u,
                     lens=lens, rag_add=add, rag_mul=mul, **kw)
    print(f"  reached {got['kernel']}")
    want = got["want"]
    assert want["own"][0].all() and want["own"][1, :, :end * u].all() and not want["own"][1, :, end * u:].any() and not want["own"][2].any()
    # nothing behind end * ups changes a bit; the utterance without frames changes nothing at all
    for o in ("out", "planes"):
        if got[o] is not None:
            keep = _through_planes(np.float32(SENT), c["precision"]) if o == "planes" else np.float32(SENT)
            assert (_bits(got[o][1, :, end * u:]) == _bits(keep)).all() and (_bits(got[o][2]) == _bits(keep)).all(), (kind, o)
    # the 1e3 behind the end was not read: the last owned columns are what the zeroed input gives (assertion 1 held them to
    # the float64 reference of the zeroed input; a read of 1e3 through one tap is off by hundreds)
    assert np.abs(got["out"][1, :, :end * u]).max() < 100


# ------------------------------------------------------------------ d. transposed convs

@pytest.mark.parametrize("u,K,Cout", [(2, 4, 64), (8, 16, 32)])
def test_transposed_convs_skip_their_zero_tap(u, K, Cout):
    # the upsamplers (kernel 2 u) in their dense 3-tap form, Cout * u a multiple of 128: the four-wave tile of the 16x16x32 loop
    # (a wave = one output phase) skips the MFMAs of its phase's all-zero tap; the 64- and 32-row tiles of the same packing run
    # all three taps and must give the same bits
    B, Cin = 2, 128
    for T in (261, 3):
        r, x, w, b = _data(u * 100 + T, B, Cin, Cout, T, K, stride=u)
        first = None
        for run in (0, 1, 2, 3):
            got = check_case(f"transposed u{u} K{K} run {run} T{T}", "transposed", x, w, b, want=first["want"] if first else None,
                             precision="f16x3", stride=u, run_cfg=run, planes=True, oslope2=0.1)
            assert got["pack_cfg"] == 0 and got["s16"]
            _expect_name(got, TILE16, run, EPI["Up"], 2, 16, False)
            first = first or got
            same = np.array_equal(_bits(got["out"]), _bits(first["out"])) and np.array_equal(_bits(got["planes"]), _bits(first["planes"]))
            print(f"[transposed] u{u} K{K} T{T}: run tile {run} equals the zero-tap-skipping tile bit for bit: {same}")
            assert same, (u, K, T, run)


# ------------------------------------------------------------------ e. range guard

def test_range_guard_tracks_what_is_split_into_fp16_planes():
    """SxArgs::peak (fp16 arithmetics): split2h_pair_pk / cvt1h_pair_pk record max(|x|, |y|) of every pair they split, BEFORE the
    clamp to +-65504.  The epilogue calls them on the values the planes store - leaky_relu(value, oslope2) of every owned
    element - and on nothing else: a launch without plane output tracks nothing there.  The raw-input prologue calls them on
    every cell it stages: leaky_relu(x, islope) of the tile's columns and halo, the zeros of the padding included.  NaN is not
    tracked (fmax drops it); the raw output is not tracked."""
    from phoonnx_amd.session import test_conv1d_sx_epi
    B, C, T, K, dil = 2, 128, 261, 3, 2
    r, x, w, b = _data(91, B, C, C, T, K)
    got = test_conv1d_sx_epi(x, w, b, precision="f16x3", dil=dil, planes=True, oslope2=1.0, lens=[130, 40], rag_add=2, rag_mul=2)
    own = np.zeros(got["out"].shape, bool)
    own[0, :, :T], own[1, :, :84] = True, True
    top = float(np.abs(got["out"][own]).max())
    print(f"[range guard] plane input: peak {got['peak']!r}, max|out| over owned elements {top!r}; {got['kernel']}")
    assert got["peak"] == top
    # ... with a slope on the planes it is the activated value that is tracked
    got = test_conv1d_sx_epi(x, w, b, precision="f16x3", dil=dil, planes=True, oslope2=0.1)
    top = float(np.abs(_lrelu32(got["out"], 0.1)).max())
    print(f"[range guard] plane input, oslope2 0.1: peak {got['peak']!r}, max|leaky_relu(out)| {top!r}")
    assert got["peak"] == top
    # ... and without plane output nothing is
    assert test_conv1d_sx_epi(x, w, b, precision="f16x3", dil=dil)["peak"] == 0.0
    # the single-plane arithmetic tracks the same values
    got = test_conv1d_sx_epi(x, w, b, precision="f16", dil=dil, planes=True, oslope2=1.0)
    assert got["peak"] == float(np.abs(got["out"]).max()), (got["peak"], np.abs(got["out"]).max())
    # values beyond fp16: the peak says so, the planes are clamped and finite, the raw output is exact
    big = test_conv1d_sx_epi(x, w, b + np.float32(1e5), precision="f16x3", dil=dil, planes=True, oslope2=1.0)
    print(f"[range guard] bias 1e5: peak {big['peak']!r}, max|planes| {np.abs(big['planes']).max()!r}")
    assert np.isfinite(big["peak"]) and big["peak"] > 65504 and big["peak"] == float(np.abs(big["out"]).max())
    assert np.isfinite(big["planes"]).all() and np.abs(big["planes"]).max() == 65504.0
    assert np.array_equal(big["planes"], _through_planes(big["out"], "f16x3"))
    # the raw-input prologue: the activated input, whatever the epilogue stores
    r, x, w, b = _data(92, B, 64, 64, T, K)
    x[1, 5, 17] = -3e4
    got = test_conv1d_sx_epi(x, w, b, precision="f16x3", dil=dil, islope=0.1)
    top = float(np.abs(_lrelu32(x, 0.1)).max())
    print(f"[range guard] raw input: peak {got['peak']!r}, max|leaky_relu(x, 0.1)| {top!r}; {got['kernel']}")
    assert got["rawin"] and got["peak"] == top and 2999 < top < 3001


# ------------------------------------------------------------------ f. what the hook refuses

def test_sx_conv_epilogue_hook_refuses_what_the_engine_cannot_form():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import SessionError, test_conv1d_sx_epi
    T = 40
    x, w = np.zeros((1, 128, T), np.float32), np.zeros((128, 128, 3), np.float32)
    xr, wr = np.zeros((1, 64, T), np.float32), np.zeros((64, 64, 3), np.float32)
    o = np.zeros((1, 128, T), np.float32)
    for match, args, kw in (("acc without a raw tensor", (x, w), dict(flags=("acc",), raw=False, planes=True)),
                            ("exactly one form", (x, w), dict(flags=("res",))),
                            ("exactly one form", (xr, wr), dict(flags=("res",), res=o[:, :64], res_is_x=True)),
                            ("res_planes on raw input", (xr, wr), dict(flags=("res",), res=o[:, :64], res_planes=True, res_slope=0.1)),
                            ("res_planes in bf16x6", (x, w), dict(flags=("res",), res=o, res_planes=True, res_slope=0.1, precision="bf16x6")),
                            ("reads its residual from a plane", (x, w), dict(flags=("res",), res=o, precision="f16")),
                            ("res_is_x needs a raw-input conv", (x, w), dict(flags=("res",), res_is_x=True)),
                            ("run_cfg 3 without s16", (x, w), dict(run_cfg=3, no_s16=True)),
                            ("run_cfg 3 without s16", (x, w), dict(run_cfg=3, precision="bf16x6")),
                            ("taller than the packed one", (x, w[:96]), dict(run_cfg=1)),
                            ("taller than the packed one", (x, w), dict(run_cfg=0, min_cfg=1)),
                            ("raw input on cfg 0", (xr, np.zeros((128, 64, 3), np.float32)), dict(run_cfg=0)),
                            ("packed for", (xr, np.zeros((128, 64, 3), np.float32)), dict(run_cfg=2)),
                            # (a stage that does not fit: pack_conv_sx refuses the halo of 300 columns for every tile)
                            ("not supported by the sx engine", (x, np.zeros((128, 128, 7), np.float32)), dict(dil=50, precision="bf16x6")),
                            ("not supported by the sx engine", (x, np.zeros((128, 128, 7), np.float32)), dict(dil=50)),
                            ("islope on a plane-input conv", (x, w), dict(islope=0.1)),
                            ("lens outside", (x, w), dict(lens=[T + 1])),
                            ("lens outside", (x, w), dict(lens=[-1])),
                            ("rag_mul < 1", (x, w), dict(lens=[T], rag_mul=0)),
                            ("bias_b rows", (x, w), dict(bias_b=np.zeros((1, 96), np.float32))),
                            ("a residual operand without", (x, w), dict(res=o)),
                            ("neither a raw nor a plane", (x, w), dict(raw=False)),
                            ("Cin % 16", (x[:, :24], w[:, :24]), dict()),
                            ("Cin % 32 == 0", (x[:, :80], w[:, :80]), dict(precision="f16"))):
        with pytest.raises(SessionError, match=match):
            test_conv1d_sx_epi(*args, None, **kw)
    # tensors whose shape does not match the launch are refused in front of the library
    for kw in (dict(flags=("res",), res=o[:, :64]), dict(flags=("acc",), old_out=o[:, :, :T - 1]), dict(lens=[T, T])):
        with pytest.raises(ValueError, match="the launch needs"):
            test_conv1d_sx_epi(x, w, None, **kw)
    # ... which the library refuses itself, whoever calls it
    a = _ffi.VitsTestConvSxEpiArgs()
    assert _ffi.load().vits_test_conv1d_sx_epi(0, a) == -3 and "sx conv epilogue hook" in _ffi.last_error(None)
    # and what it accepts next to those runs: zeros in, zeros out, in the raw tensor and through the planes
    got = test_conv1d_sx_epi(x, w, None, run_cfg=3, planes=True)
    assert not got["out"].any() and not got["planes"].any() and _template_args(got["kernel"])["tile"] == TILE16[3]
