"""The fused ResBlock-step kernel (csrc/conv_sx_pair16.hip.hpp, conv_sx_pair16_kernel) by value, launch by launch as the
generator's conv_sx_pair16() forms them: every one-shot instantiation at its edges and seams, every call-site form of the
epilogue, per-utterance tensor ends inside one launch, the residual's identity, the fp16 range guard, what is refused.

Each case is ONE launch through session.test_conv_pair16_epi and is held to three things (every measured figure is printed in
front of its assertion; WORST keeps the largest ratio per (group, check)):
  a. value, against the float64 reference of tests/pair_epi_ref.py on the elements the launch owns, at the figures the project
     already holds this kernel to:
       f16x3 raw and planes  5e-5 absolute + 1e-5 relative on unit-scale outputs (test_conv_pair16_f16x3_matches_two_launches_
                             and_oracle); with acc / div the absolute part is scaled by max(1, max|want|) - in this arithmetic
                             only; + 2^-22 |x| for the residual read from two planes (the bound documented at SX_RES_PL);
                             the residual group instead: 2e-5 * max|want| with the residual as the planes hold it
       f16x3 planes          3e-7 relative to the float32 value they copy (absolute floor 2^-36, sx_split.hip.hpp)
       f16 (one plane)       against the `quantized` reference, in every form, acc and div included, unscaled: raw 3e-3
                             absolute, rms < 1e-4, at most 0.1 % of the owned elements off by more than 1e-4 (an intermediate
                             that rounds the other way), and against the unrounded reference rms < 2e-3 of its rms; planes
                             (fp16 values) 3e-3 absolute + 2^-10 relative (test_conv_pair16_single_plane_mode)
  b. ownership: every raw or plane element outside the reference's masks keeps its bits - the sentinel or old_out -, the
     guard bands behind both tensors are intact, and without "raw" the whole raw tensor is what was uploaded;
  c. the epilogue bit for bit: the same pair launched plain ("raw" only) gives `base`; the fused form's value must be
     (base + old) / div in numpy float32, in that order, and planes must be the split of leaky_relu of that float32 value.

Instantiations: the launcher's one-shot set is <32,2,256> <32,1,256> <64,2,128,OVL> <64,1,128> <32,2,128> <32,1,128>, each
as PAIR and CHAIN.  The first four are what sx_pair16_plan chooses; <32,2,128> is reached in-process by a pair whose 256-column
tile does not fit the LDS of two workgroups per CU (k 11, dilations (9, 4)); <32,1,128> by no supported shape (the single
plane halves the LDS): both 128-column forms are run in a child process under VITSMI_PAIR16_BN=128, as the existing switch
tests do.
"""
import os
import re
import sys

import numpy as np
import pytest

from pair_epi_ref import pair_epi_ref
from test_gpu_sx_conv_epilogue import _bits, _lrelu32, _neg, _through_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -1234.5678
SLOPE = 0.1
LDS_TWO_PER_CU = 160 * 1024 // 2 - 256          # conv_geom.hpp kLdsTwoPerCu
WPS = {(32, 1, 256): 3, (32, 1, 128): 4, (64, 1, 128): 3, (32, 2, 128): 3, (32, 2, 256): 2, (64, 2, 128): 2}   # P16_CASE
NPL = {"f16x3": 2, "f16": 1}
WORST = {}
REACHED = set()


def _note(group, what, ratio, kernel):
    key = (group, what)
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, kernel)
    print(f"[{group}] worst so far {what}: {WORST[key][0]:.3f} x tolerance ({WORST[key][1]})")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nWORST ratio per (group, check):")
    for (group, what), (ratio, kernel) in sorted(WORST.items()):
        print(f"  [{group}] {what}: {ratio:.3f} x tolerance ({kernel})")
    print("instantiations reached:")
    for k in sorted(REACHED):
        print("  " + k)


# ---- sx_pair16_geom / sx_pair16_plan (conv_sx_pair16.hip.hpp), restated: which tile a pair runs on

def _geom(C, npl, BN, ovl, K, d1, d2):
    halo1, halo2 = (K - 1) * d1, (K - 1) * d2
    pad2 = halo2 // 2
    if halo1 > 96 or K % 2 == 0:
        return None
    RS1 = (BN + halo1 + 15) // 16 * 16
    RS2 = (BN + pad2 + 15) // 16 * 16
    xb, yb = npl * (C // 8) * RS1 * 16, npl * (C // 8) * RS2 * 16 + (pad2 + 16) * 16
    lds = (max(xb, yb) if ovl else xb + yb) + 1024
    return lds if BN - halo2 >= BN // 2 + BN // 8 else None


def plan(C, precision, K, d1, d2):
    """-> (BN, BNo, ovl), or None where the pair is refused"""
    npl = NPL[precision]
    if C not in (32, 64):
        return None
    ovl = npl == 2 and C == 64
    pref = [128, 128] if C == 64 else ([128, 256] if os.environ.get("VITSMI_PAIR16_BN") == "128" else [256, 128])
    for BN in pref:
        lds = _geom(C, npl, BN, ovl, K, d1, d2)
        if lds is not None and lds <= LDS_TWO_PER_CU:
            return BN, BN - (K - 1) * d2, ovl
    return None


def _kernel_name(C, precision, BN, chain, ovl):
    tf = lambda v: "true" if v else "false"
    return f"conv_sx_pair16_kernel<{C}, {NPL[precision]}, {BN}, {tf(chain)}, {tf(ovl)}, {WPS[(C, NPL[precision], BN)]}, false>"


def weights(seed, C, K, positive=False, s2=2.0):
    r = np.random.default_rng(seed)
    w1 = r.standard_normal((C, C, K)) / np.sqrt(C * K)
    w2 = r.standard_normal((C, C, K)) / np.sqrt(C * K) * s2
    if positive:   # (taps that sum to about 1: unit-scale outputs from a constant input)
        w1, w2 = np.abs(w1) * (1.25 / np.sqrt(C * K)), np.abs(w2) * (1.25 / np.sqrt(C * K) / s2)
    return (w1.astype(np.float32), r.standard_normal(C).astype(np.float32), w2.astype(np.float32),
            r.standard_normal(C).astype(np.float32))


def w2_scale(precision):
    """c2's weights relative to unit scale.  f16x3: 2, as the tests before this one.  f16: 1 / 8 - an intermediate that lies on a
    rounding boundary of its fp16 plane and falls the other way moves C * K outputs by ulp(mid) * |w2| each; at unit scale one
    such element (about 1e-4 of them) alone puts more than 0.1 % of a 16 k-element case beyond 1e-4, whatever the seed
    (measured on the MI355X at w2 scale 2: 0.63 % of the 16.3 k elements of the 64-channel PAIR case at T = BNo + 1, at rms
    1.6e-5 and a largest error of 4.4e-4; float32 accumulation on the CPU gives 0.17 % on the 32-channel T = 254 case).  With
    |w2| ~ 0.0125 only intermediates beyond |mid| = 2 can, and the cap of check a counts what it is meant to count.  A wrong tap
    or a wrong padding of c2 still moves outputs by ~0.05, far beyond every figure."""
    return 2.0 if precision == "f16x3" else 0.125


def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _ratio(err, tol, sel):
    return float((err[sel] / tol[sel]).max()) if sel.any() else 0.0


def check_case(name, group, x, wb, flags, precision, K, d1, d2, chain, res_seen=False, base=None, **kw):
    """one launch against the three assertions of the module docstring; returns the hook's result (with the reference as
    got["want"] and the plain launch as got["base"])"""
    from phoonnx_amd.session import test_conv_pair16_epi
    w1, b1, w2, b2 = wb
    f = set(flags)
    B, C, T = x.shape
    got = test_conv_pair16_epi(x, w1, b1, w2, b2, flags=flags, dil1=d1, dil2=d2, chain=chain, slope=SLOPE, precision=precision,
                               sentinel=SENT, **kw)
    k = got["kernel"]
    REACHED.add(k)
    # ---- the tile: the rule of sx_pair16_geom, so that a silent change of tile choice shows
    BN, BNo, ovl = plan(C, precision, K, d1, d2)
    print(f"[{group}] {name}: {k}, BN {got['BN']} BNo {got['BNo']} ovl {got['ovl']}, peak {got['peak']!r}")
    assert (got["BN"], got["BNo"], got["ovl"]) == (BN, BNo, ovl), (name, got["BN"], got["BNo"], got["ovl"], BN, BNo, ovl)
    assert k == _kernel_name(C, precision, BN, chain, ovl), (name, k)
    rkw = {a: kw[a] for a in ("div", "old_out", "lens", "rag_add", "rag_mul") if a in kw}
    rkw.update(flags=flags, dil1=d1, dil2=d2, chain=chain, slope=SLOPE, sentinel=SENT)
    xs = got["x_seen"]
    ref = pair_epi_ref(x, w1, b1, w2, b2, res_x=xs if res_seen else None, **rkw)
    want = pair_epi_ref(x, w1, b1, w2, b2, quantized=True, **rkw) if precision == "f16" else ref
    accdiv = bool(f & {"acc", "div"})
    # ---- a. value on owned elements
    for o, own in (("out", "own"), ("planes", "own_pl")):
        if want[o] is None:
            assert got[o] is None, (name, o)
            continue
        sel = want[own]
        if not sel.any():
            continue
        err = np.abs(got[o].astype(np.float64) - want[o])
        if precision == "f16x3":
            scale = max(1.0, float(np.abs(want[o][sel]).max())) if accdiv or res_seen else 1.0
            if res_seen:   # the residual as the planes hold it: the engine's 2e-5 grade, no 2^-22 |x| allowance
                tol = np.full(err.shape, 2e-5 * scale)
                desc = f"2e-5 * {scale:.1f}"
            else:
                tol = 5e-5 * scale + 1e-5 * np.abs(want[o]) + 2.0 ** -22 * np.abs(x)
                desc = f"5e-5 * {scale:.2f} + 1e-5 |want| + 2^-22 |x|"
            ratio = _ratio(err, tol, sel)
            print(f"[{group}] {name}: {o} max err {err[sel].max():.3e} = {ratio:.3f} x ({desc})")
            _note(group, f"f16x3 {o} vs float64", ratio, k)
            assert ratio <= 1, (name, o, ratio)
        else:
            tol = 3e-3 + (2.0 ** -10 * np.abs(want[o]) if o == "planes" else 0.0) + np.zeros(err.shape)
            ratio = _ratio(err, tol, sel)
            print(f"[{group}] {name}: {o} vs quantized: max err {err[sel].max():.3e} = {ratio:.3f} x tolerance")
            _note(group, f"f16 {o} vs quantized float64", ratio, k)
            assert ratio <= 1, (name, o, ratio)
            if o == "planes":   # (fp16 values, each 2^-11 of its magnitude off: the per-element figures are the raw tensor's)
                continue
            rms = float(np.sqrt((err[sel] ** 2).mean()))
            share = float((err[sel] > 1e-4).mean())
            r64 = ref[o]
            rms_u = float(np.sqrt(((got[o] - r64)[sel] ** 2).mean()) / max(np.sqrt((r64[sel] ** 2).mean()), 1e-30))
            print(f"[{group}] {name}: {o} vs quantized: rms {rms:.3e} (< 1e-4), {100 * share:.4f} % of {int(sel.sum())} owned elements off "
                  f"by > 1e-4 (<= 0.1 %); vs unrounded: rms {rms_u:.3e} of its rms (< 2e-3)")
            _note(group, f"f16 {o} rms vs quantized / 1e-4", rms / 1e-4, k)
            _note(group, f"f16 {o} share off by > 1e-4 / 0.1 %", share / 1e-3, k)
            _note(group, f"f16 {o} rms vs unrounded / 2e-3", rms_u / 2e-3, k)
            assert rms < 1e-4, (name, o, rms)
            assert share <= 1e-3, (name, o, share)
            assert rms_u < 2e-3, (name, o, rms_u)
    # ---- b. ownership
    assert got["guard_ok"], (name, "the guard band behind an output changed")
    prev = np.full(x.shape, np.float32(SENT)) if kw.get("old_out") is None else np.asarray(kw["old_out"], np.float32)
    keep = ~want["own"]
    assert np.array_equal(_bits(got["out"])[keep], _bits(prev)[keep]), (name, "a raw element the launch does not own changed")
    if "raw" not in f:
        assert np.array_equal(_bits(got["out"]), _bits(prev)), (name, "the raw tensor of a launch without raw store changed")
    if got["planes"] is not None:
        keep = ~want["own_pl"]
        held = np.full(x.shape, _through_planes(np.float32(SENT), precision))
        assert np.array_equal(_bits(got["planes"])[keep], _bits(held)[keep]), (name, "a plane element the launch does not own changed")
    # ---- c. the epilogue bit for bit
    if f != {"raw"}:
        if base is None:
            pkw = {a: kw[a] for a in ("lens", "rag_add", "rag_mul", "x_tail") if a in kw}
            base = test_conv_pair16_epi(x, w1, b1, w2, b2, flags=("raw",), dil1=d1, dil2=d2, chain=chain, slope=SLOPE,
                                        precision=precision, sentinel=SENT, **pkw)
        assert base["kernel"] == k, (base["kernel"], k)
        v = base["out"]
        if "acc" in f:
            v = v + np.asarray(kw["old_out"], np.float32)
        if "div" in f:
            v = v / np.float32(kw["div"])
        assert v.dtype == np.float32
        if "raw" in f:
            sel = want["own"]
            same = np.array_equal(_bits(got["out"])[sel], _bits(v)[sel])
            print(f"[{group}] {name}: raw output equals (base + old) / div on the plain launch bit for bit: {same}")
            assert same, (name, "raw", float(np.abs(got["out"] - v)[sel].max()))
        if "planes" in f:
            sel = want["own_pl"]
            src = got["out"] if "raw" in f else v
            o2 = _lrelu32(src, SLOPE)
            e = _through_planes(o2, precision)
            same = np.array_equal(_bits(got["planes"])[sel], _bits(e)[sel])
            print(f"[{group}] {name}: planes are the split of leaky_relu of the same float32 value bit for bit: {same}")
            assert same, (name, "planes", float(np.abs(got["planes"] - e)[sel].max()))
            if precision == "f16x3" and sel.any():
                small = sel & (np.abs(o2) <= 65504)
                rel = float((np.abs(got["planes"].astype(np.float64) - o2)[small] / (3e-7 * np.abs(o2[small]) + 2.0 ** -36)).max())
                print(f"[{group}] {name}: planes vs the float32 value they copy: {rel:.3f} x (3e-7 relative + 2^-36)")
                _note(group, "f16x3 planes vs the value they copy", rel, k)
                assert rel <= 1, (name, rel)
    got["want"], got["ref"], got["base"] = want, ref, base
    return got


# ------------------------------------------------------------------ 1. every instantiation at its edges

INST = [(C, p, chain) for C in (32, 64) for p in ("f16x3", "f16") for chain in (False, True)]
INST_IDS = [f"C{C}-{p}-{'chain' if ch else 'pair'}" for C, p, ch in INST]
# the widest supported halos: (C, K, d1, d2, chain)
HALOS = [(32, 11, 5, 1, False), (64, 11, 5, 1, False), (32, 7, 3, 12, True), (64, 5, 2, 6, True)]


def edge_lengths(C, precision, K, d1, d2):
    BN, BNo, _ = plan(C, precision, K, d1, d2)
    pad1 = d1 * (K - 1) // 2
    return sorted({1, pad1, pad1 + 1, BNo - 1, BNo, BNo + 1, 2 * BNo, 2 * BNo + 1})


def edge_cases():
    """(name, C, precision, K, d1, d2, chain, T, seed) of group 1; the CPU test of the f16 cap walks the same list"""
    out = []
    for C, p, chain in INST:
        K, d1, d2 = 3, 1, (2 if chain else 1)
        for T in edge_lengths(C, p, K, d1, d2):
            out.append((f"C{C} {p} {'chain' if chain else 'pair'} k{K} d({d1},{d2}) T{T}", C, p, K, d1, d2, chain, T, 1000 * C + 10 * T + chain))
    for C, K, d1, d2, chain in HALOS:
        for p in ("f16x3", "f16"):
            for T in edge_lengths(C, p, K, d1, d2):
                out.append((f"C{C} {p} {'chain' if chain else 'pair'} k{K} d({d1},{d2}) T{T}", C, p, K, d1, d2, chain, T, 2000 * C + 10 * T + K))
    return out


def edge_data(case, B=2):
    _, C, p, K, d1, d2, chain, T, seed = case
    return normal(seed, B, C, T), weights(seed + 1, C, K, s2=w2_scale(p))


def _run_edges(cases, group):
    for case in cases:
        name, C, p, K, d1, d2, chain, T, _ = case
        x, wb = edge_data(case)
        check_case(name, group, x, wb, ("raw", "planes"), p, K, d1, d2, chain)


@pytest.mark.parametrize("inst", INST, ids=INST_IDS)
def test_every_instantiation_at_its_edges(inst):
    # raw + planes, B = 2, k 3: T = 1, the halo, the halo + 1, one column either side of one and of two tiles of BNo kept columns
    C, p, chain = inst
    _run_edges([c for c in edge_cases() if (c[1], c[2], c[6], c[3]) == (C, p, chain, 3)], "edges")


@pytest.mark.parametrize("halo", HALOS, ids=[f"C{C}-k{K}-d{d1}-{d2}" for C, K, d1, d2, _ in HALOS])
def test_the_widest_halos(halo):
    C, K, d1, d2, chain = halo
    _run_edges([c for c in edge_cases() if (c[1], c[3], c[4], c[5], c[6]) == (C, K, d1, d2, chain)], "halos")


def test_every_one_shot_instantiation_is_reached():
    """What sx_pair16_plan chooses by itself - <32,2,256> <32,1,256> <64,2,128,OVL> <64,1,128> - and the 128-column tile at 32
    channels where the 256-column one does not fit (f16x3, k 11, dilations (9, 4): x tile + Y > the LDS of two workgroups per
    CU), each as PAIR and CHAIN, named by the launcher."""
    seen = set()
    for C, p, chain in INST:
        K, d1, d2 = 3, 1, (2 if chain else 1)
        BN, BNo, ovl = plan(C, p, K, d1, d2)
        got = check_case(f"reach C{C} {p} chain {chain}", "reach", normal(5, 2, C, BNo + 1), weights(6, C, K, s2=w2_scale(p)), ("raw", "planes"), p, K, d1, d2, chain)
        seen.add(got["kernel"])
    for chain in (False, True):
        assert plan(32, "f16x3", 11, 9, 4) == (128, 88, False)
        got = check_case(f"reach C32 f16x3 128 columns chain {chain}", "reach", normal(7, 2, 32, 89), weights(8, 32, 11), ("raw", "planes"), "f16x3",
                         11, 9, 4, chain)
        seen.add(got["kernel"])
    want = {_kernel_name(C, p, 256 if C == 32 else 128, chain, C == 64 and p == "f16x3") for C, p, chain in INST}
    want |= {_kernel_name(32, "f16x3", 128, chain, False) for chain in (False, True)}
    print("reached:", sorted(seen))
    assert seen == want, seen ^ want


def bn128_child():
    """(child process, VITSMI_PAIR16_BN=128) the 32-channel instantiations on 128-column tiles: at their edges, in the six
    call-site forms at one seam length, and on ragged ends"""
    assert os.environ.get("VITSMI_PAIR16_BN") == "128"
    for p in ("f16x3", "f16"):
        for chain in (False, True):
            K, d1, d2 = 3, 1, (2 if chain else 1)
            assert plan(32, p, K, d1, d2)[0] == 128
            for T in edge_lengths(32, p, K, d1, d2):
                case = (f"C32 {p} {'chain' if chain else 'pair'} 128 columns T{T}", 32, p, K, d1, d2, chain, T, 3000 + 10 * T + chain)
                _run_edges([case], "edges 128")
            _run_forms(32, p, chain, "forms 128")
            _run_ragged(32, p, chain, "ragged 128")
    for (group, what), (ratio, kernel) in sorted(WORST.items()):
        print(f"  [{group}] {what}: {ratio:.3f} x tolerance ({kernel})")
    assert REACHED == {_kernel_name(32, p, 128, chain, False) for p in ("f16x3", "f16") for chain in (False, True)}, REACHED
    print("BN128_OK")


def test_the_128_column_tiles_at_32_channels():
    """<32,2,128> and <32,1,128>, PAIR and CHAIN, at the same edges, call-site forms and ragged ends as the others.  No supported shape makes sx_pair16_plan fall
    back to 128 columns in the single-plane arithmetic, so both run under the A/B switch VITSMI_PAIR16_BN=128, in a child
    process: the switch is read once per process."""
    import subprocess
    code = "import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_pair16_epilogue as t; t.bn128_child()"
    env = dict(os.environ, VITSMI_PAIR16_BN="128")
    r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "BN128_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------ 2. every call-site form of p16_flags()

FORMS = {"planes": (("planes",), None), "raw": (("raw",), None), "acc+raw": (("acc", "raw"), None), "acc+div+raw": (("acc", "div", "raw"), 3.0),
         "acc+div+planes": (("acc", "div", "planes"), 2.0), "raw+planes": (("raw", "planes"), None)}


def _run_forms(C, p, chain, group):
    # one column behind the first seam, B = 2; old_out of unit scale; the plain launch is shared by the six forms
    K, d1, d2 = 3, 1, (2 if chain else 1)
    T = plan(C, p, K, d1, d2)[1] + 1
    x, wb, old = normal(40 + C, 2, C, T), weights(41 + C + chain, C, K, s2=w2_scale(p)), normal(42 + C, 2, C, T)
    base = None
    for form, (flags, div) in FORMS.items():
        kw = {}
        if "acc" in flags:
            kw["old_out"] = old
        if div:
            kw["div"] = div
        got = check_case(f"C{C} {p} {'chain' if chain else 'pair'} {form}", group, x, wb, flags, p, K, d1, d2, chain, base=base, **kw)
        base = base or got["base"] or (got if form == "raw" else None)
        if form == "acc+div+planes":
            assert np.array_equal(_bits(got["out"]), _bits(old)), "the accumulate operand of a launch without raw store changed"


@pytest.mark.parametrize("inst", INST, ids=INST_IDS)
def test_every_call_site_form(inst):
    _run_forms(*inst, "forms")


# ------------------------------------------------------------------ 3. ragged ends

def ragged_data(C, p, chain):
    K, d1, d2 = (5, 2, 6) if chain else (7, 3, 1)
    BNo = plan(C, p, K, d1, d2)[1]
    T = 2 * BNo + 1
    sets = (([0, 37, T], 0, 1, [0, 37, T]), ([BNo - 1, BNo, BNo + 1], 0, 1, [BNo - 1, BNo, BNo + 1]), ([0, 5, T], 2, 8, [0, 56, T]))
    return K, d1, d2, BNo, T, np.full((3, C, T), 0.75, np.float32), weights(50 + C + chain, C, K, positive=True), sets


def _run_ragged(C, p, chain, group):
    """B = 3, constant input 0.75 and positive weights: c1 evaluated behind an utterance's end is far from zero, so a hand-over
    that keeps it moves the last pad2 owned columns visibly (pad2 = 3 for the pair k 7 d (3, 1), 12 for the chain k 5 d (2, 6)).
    Ends of 0, inside the first tile, BNo - 1, BNo, BNo + 1 and T; frames of 8 columns with a margin of 2.  Every launch twice,
    with zeros and with finite garbage of magnitude 1e4 in the input planes behind the ends: the owned outputs must not differ
    in a bit."""
    K, d1, d2, BNo, T, x, wb, sets = ragged_data(C, p, chain)
    garbage = (normal(51, 3, C, T) * np.float32(1e4)).astype(np.float32)
    for lens, add, mul, want_ends in sets:
        runs = []
        for tail in (np.zeros_like(x), garbage):
            got = check_case(f"C{C} {p} {'chain' if chain else 'pair'} lens {lens} add {add} mul {mul}", group, x, wb, ("raw", "planes"), p, K,
                             d1, d2, chain, lens=lens, rag_add=add, rag_mul=mul, x_tail=tail)
            runs.append(got)
        own = runs[0]["want"]["own"]
        ends = [int(own[b, 0].sum()) for b in range(3)]
        assert ends == want_ends, (ends, want_ends)
        for o in ("out", "planes"):
            same = np.array_equal(_bits(runs[0][o]), _bits(runs[1][o]))
            print(f"[{group}] C{C} {p} ends {ends}: {o} with garbage behind the ends equals {o} with zeros there bit for bit: {same}")
            assert same, (C, p, chain, lens, o)


@pytest.mark.parametrize("inst", INST, ids=INST_IDS)
def test_ragged_ends_inside_one_launch(inst):
    _run_ragged(*inst, "ragged")


# ------------------------------------------------------------------ 4. residual identity

@pytest.mark.parametrize("C,chain", [(32, False), (32, True), (64, False), (64, True)])
def test_the_residual_is_x_not_its_activation(C, chain):
    """The `neg` inputs of tests/test_gpu_pair_single_read.py: a quarter of the elements near -1e3, where leaky_relu(x) = 0.1 x,
    so a residual taken behind the activation is off by 0.9 |x|.  Against the reference with the residual the kernel recovers
    from its planes (x_seen), at the engine's 2e-5 * max|want| - not the looser 2^-22 |x| allowance -, and x_seen itself within
    the planes' documented resolution of x.  64 channels: Y overlays the x tile and the residual waits in registers (OVL); 32:
    it is read back from LDS in the epilogue."""
    K, d1, d2 = 3, 1, (2 if chain else 1)
    T = plan(C, "f16x3", K, d1, d2)[1] + 1
    x = _neg(np.random.default_rng(60 + C + chain), 2, C, T)
    got = check_case(f"neg C{C} {'chain' if chain else 'pair'}", "residual", x, weights(61 + C, C, K), ("raw",), "f16x3", K, d1, d2, chain,
                     res_seen=True)
    assert got["ovl"] == (C == 64)
    bound = (2.0 ** -22 + 3 * 2.0 ** -24) * np.abs(x) + 10 * 2.0 ** -36     # (tests/test_gpu_sx_conv_epilogue.py, residual planes)
    ratio = float((np.abs(got["x_seen"].astype(np.float64) - x) / bound).max())
    print(f"[residual] C{C}: x as recovered from its planes: {ratio:.3f} x ((2^-22 + 3 * 2^-24) |x| + 10 * 2^-36)")
    assert ratio <= 1, ratio


# ------------------------------------------------------------------ 5. range guard

@pytest.mark.parametrize("C,precision", [(32, "f16x3"), (64, "f16x3"), (32, "f16"), (64, "f16")])
def test_range_guard_tracks_the_intermediate_and_the_planes(C, precision):
    """SxPair16Args::peak: split2h_pair_pk / cvt1h_pair_pk record what they split - in the hand-over the intermediate
    leaky_relu(mid) of every live column (it exists nowhere but in LDS), in the epilogue what the planes store.  Unlike the plain
    engine (test_range_guard_tracks_what_is_split_into_fp16_planes: no plane output, peak 0), a fused launch WITHOUT plane
    output still reports a peak: the intermediate's."""
    from phoonnx_amd.session import test_conv_pair16_epi
    K, d1, d2, chain = 3, 1, 1, False
    BN, BNo, _ = plan(C, precision, K, d1, d2)
    T, lens = BNo + 40, [BNo + 40, BNo + 1, 17]
    x = normal(70 + C, 3, C, T)
    w1, b1, w2, b2 = weights(71 + C, C, K)
    kw = dict(dil1=d1, dil2=d2, chain=chain, slope=SLOPE, precision=precision, sentinel=SENT, lens=lens)
    own = np.arange(T)[None, None, :] < np.asarray(lens)[:, None, None]
    own = np.broadcast_to(own, x.shape)
    rel = lambda a, b: abs(a - b) / abs(b)
    # the output dominates: exactly the largest stored plane value
    got = test_conv_pair16_epi(x, w1, b1, w2, b2 + np.float32(50), flags=("raw", "planes"), **kw)
    top = float(np.abs(_lrelu32(got["out"], SLOPE))[own].max())
    print(f"[range guard] C{C} {precision}: planes dominate: peak {got['peak']!r}, max|leaky_relu(raw)| over owned {top!r}; {got['kernel']}")
    assert got["peak"] == top and top > 40
    # the intermediate beyond fp16, the output in range: reported although it never leaves LDS
    tiny = (w2 * np.float32(1e-7)).astype(np.float32)
    got = test_conv_pair16_epi(x, w1, b1 + np.float32(1e5), tiny, b2, flags=("raw", "planes"), **kw)
    ref = pair_epi_ref(x, w1, b1 + np.float32(1e5), tiny, b2, flags=("raw", "planes"), dil1=d1, dil2=d2, chain=chain, slope=SLOPE, lens=lens)
    mid_top = float(np.abs(np.where(ref["mid"] >= 0, ref["mid"], ref["mid"] * SLOPE))[own].max())
    print(f"[range guard] C{C} {precision}: b1 = 1e5: peak {got['peak']!r}, reference max|leaky_relu(mid)| {mid_top!r}, max|out| "
          f"{float(np.abs(got['out'][own]).max())!r}")
    assert np.isfinite(got["peak"]) and got["peak"] > 65504 and rel(got["peak"], mid_top) < 1e-5
    assert np.abs(got["out"][own]).max() < 100 and np.isfinite(got["planes"]).all()
    # no plane output, small intermediate: the intermediate's maximum, not 0
    got = test_conv_pair16_epi(x, w1, b1, w2, b2, flags=("raw",), **kw)
    ref = pair_epi_ref(x, w1, b1, w2, b2, flags=("raw",), dil1=d1, dil2=d2, chain=chain, slope=SLOPE, lens=lens, quantized=precision == "f16")
    mid_top = float(np.abs(np.where(ref["mid"] >= 0, ref["mid"], ref["mid"] * SLOPE))[own].max())
    print(f"[range guard] C{C} {precision}: raw only: peak {got['peak']!r}, reference max|leaky_relu(mid)| {mid_top!r}")
    assert got["peak"] > 0 and rel(got["peak"], mid_top) < 1e-5
    # columns behind an utterance's end never feed it: large values only there
    tail = np.full(x.shape, 1e4, np.float32)
    far = test_conv_pair16_epi(x, w1, b1, w2, b2, flags=("raw",), x_tail=tail, **kw)
    print(f"[range guard] C{C} {precision}: 1e4 behind the ends: peak {far['peak']!r}")
    assert far["peak"] == got["peak"]


# ------------------------------------------------------------------ 6. refusals

def test_the_hook_refuses_what_the_kernel_cannot_form():
    from phoonnx_amd.session import SessionError, test_conv_pair16_epi
    T = 40
    z = lambda C, K: (np.zeros((1, C, T), np.float32), np.zeros((C, C, K), np.float32), None, np.zeros((C, C, K), np.float32), None)
    old = np.zeros((1, 32, T), np.float32)
    for match, args, kw in (("launch_conv_sx_pair16", z(32, 3), dict(flags=("div", "raw"), div=2.0)),
                            ("acc without old_out", z(32, 3), dict(flags=("acc", "raw"))),
                            ("cannot run fused", z(32, 4), dict()),
                            ("cannot run fused", z(128, 3), dict()),
                            ("cannot run fused", z(64, 7), dict(dil1=3, dil2=12, chain=True)),
                            ("lens outside", z(32, 3), dict(lens=[T + 1])),
                            ("rag_mul < 1", z(32, 3), dict(lens=[T], rag_mul=0))):
        with pytest.raises(SessionError, match=match):
            test_conv_pair16_epi(*args, **kw)
    with pytest.raises(ValueError, match="the launch needs"):
        test_conv_pair16_epi(*z(32, 3), flags=("acc", "raw"), old_out=old[:, :, :T - 1])
    # and what it accepts next to those runs: zeros in, zeros out
    got = test_conv_pair16_epi(*z(32, 3), flags=("acc", "div", "raw", "planes"), old_out=old, div=2.0)
    assert got["guard_ok"] and not got["out"].any() and not got["planes"].any()
    assert re.fullmatch(r"conv_sx_pair16_kernel<32, 2, 256, false, false, 2, false>", got["kernel"])
