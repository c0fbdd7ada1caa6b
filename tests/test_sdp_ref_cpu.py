"""tests/sdp_ref.py checked without a GPU: its float64 chain of the stochastic duration predictor reproduces out_logw of every
SDP fixture the reference project produced; its fp32 restatement stays inside every tolerance the GPU tests
(tests/test_gpu_sdp_kernels.py) use; and each deliberate mistake in the float64 reference leaves that tolerance somewhere."""
import functools
import os

import numpy as np
import pytest

import sdp_ref as R
from conftest import GOLDEN, case_get, golden_cases

SDP_FIXTURES = ("tiny_rb1", "tiny_rb2_ms", "sx_rb1", "sx_rb2_ms")
_CASES = [(p, c) for p in SDP_FIXTURES for c in golden_cases(np.load(os.path.join(GOLDEN, p + ".npz")))]


@functools.lru_cache(maxsize=None)
def _weights(preset):
    from onnx_walk import OnnxModel
    from vits_oracle import resolve_weights
    return resolve_weights(OnnxModel(os.path.join(GOLDEN, preset + ".onnx")))


def test_every_sdp_fixture_is_covered():
    assert {p for p, _ in _CASES} == set(SDP_FIXTURES) and len(_CASES) >= 20


# the worst |float64 chain - out_logw| over the valid tokens of all cases, measured: FIXTURE_ERR (the fixtures are the
# reference project's fp32 arithmetic: its rounding through three spline flows); asserted at 2 x that
FIXTURE_ERR = 4.4e-6


@pytest.mark.parametrize("preset,case", _CASES)
def test_float64_chain_reproduces_out_logw(preset, case):
    W, ints = _weights(preset)
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    x, lens, sc, sid = (case_get(g, case, k) for k in ("out_x", "lens", "scales", "sid"))
    noise = case_get(g, case, "noise_dp")
    if noise is None:
        assert sc[2] == 0
        noise = np.zeros((x.shape[0], 2, x.shape[2]), np.float32)
    got = R.sdp_logw_ref(W, ints, x, lens, noise, sc[2], sid)
    want = case_get(g, case, "out_logw")[:, 0, :]
    valid = R.mask_of(lens, x.shape[2])
    err = float(np.abs(got - want)[valid].max())
    print(f"{preset}/{case}: max|float64 chain - out_logw| = {err:.3e}")
    assert err <= 2 * FIXTURE_ERR, err


# ------------------------------------------------------------------ (a) the fp32 restatement is inside every tolerance

def _dw_eval(C, K, dil, T, dt=np.float64, mut=None):
    c = R.dw_case(C, K, dil, T)
    return c, R.dw_ln_gelu_ref(c["x"], c["dw_w"], c["dw_b"], dil, c["gamma"], c["beta"], c["lens"], dt, mut)


def _dw_bound(c):
    v = R.depthwise_ref(c["x"], c["dw_w"], c["dw_b"], c["dil"], c["lens"])
    return R.ln_bound(v, c["gamma"], c["beta"], v_err=R.dw_v_err(c["x"], c["dw_w"], c["dw_b"], c["dil"], c["lens"]))


def test_restatement_passes_the_layernorm_bound():
    """every launch of the GPU module - R.ln_runs() is the table it runs from: by width with the in-place accumulate, by
    length, the plane cases and the one past the fp16 range - and every depthwise + LN case"""
    worst = 0.0
    for run in R.ln_runs():
        _, _, r64, bound = R.ln_run_ref(run)
        worst = max(worst, R.excess(R.ln_run_ref(run, np.float32)[2], r64, bound))
    for a in R.DW_CASES:
        c, r64 = _dw_eval(*a)
        worst = max(worst, R.excess(_dw_eval(*a, dt=np.float32)[1], r64, _dw_bound(c)))
    print(f"worst restatement error / bound: {worst:.3f}")
    assert worst <= 1.0, worst


def _dds_evals():
    for C in R.DDS_WIDTHS[32]:
        for T, dil, m in R.dds_single_cases(32, C):
            yield ("single", C, T, dil, m), R.dds_single_eval(C, T, dil, m)[1:]
        yield ("onehot", C), R.dds_single_eval(C, 33, 3, False, True)[1:]
    for C, n in sorted({(C, n) for _, C, n in R.DDS_STACKS}):
        yield ("stack", C, n), R.dds_stack_eval(C, n)[1:]
    for C, ch in R.DDS_HEAD_CASES:
        yield ("head", C, ch), R.dds_flow_eval(C, ch)[3:]
        for rows in R.DDS_TAIL_ROWS(C):
            yield ("head+tail", C, ch, rows), R.dds_flow_eval(C, ch, rows)[3:]
            yield ("tail", C, ch, rows), R.dds_flow_eval(C, ch, rows, head=False)[3:]


def test_dds_and_spline_cases_are_well_conditioned():
    """The per-case tolerance is 4 x the restatement's own error, so the restatement passes it by construction; what can go
    wrong is an LN column of so small a variance that rounding is amplified and the tolerance stops meaning anything.  A
    well-conditioned case's restatement error stays within 16 x 2^-24 of the largest output: tolerance <= 64 x 2^-24 x that."""
    worst = 0.0
    for name, (r64, tol, valid) in _dds_evals():
        big = float(np.abs(r64).max())
        assert 0 < tol <= 64 * R.U32 * big, (name, tol, big)
        worst = max(worst, tol / (R.U32 * big))
    print(f"largest DDS tolerance: {worst:.1f} x 2^-24 x max|out|")
    # the spline: sharp softmaxes are ill conditioned on purpose (bins at the 1e-3 floor); the tolerance stays far below the
    # width of a floor bin (1e-2 in x) all the same
    for a in R.spline_cases():
        _, r64, tol, _ = R.spline_eval(*a)
        assert tol <= 3e-3, (a, tol)


# ------------------------------------------------------------------ (b) every mutation leaves its family's tolerance

def _caught(pairs):
    """pairs of (mutated float64, reference float64, tolerance, valid): the worst excess over the family's cases"""
    return max(R.excess(m, r, tol, valid) for m, r, tol, valid in pairs)


def _ln_family(mut):
    for run in R.ln_runs():
        c, _, r64, bound = R.ln_run_ref(run)
        valid = R.valid_of(c["lens"], run[2], bool(run[3] & R.LN_MASK))
        yield R.ln_run_ref(run, mut=mut)[2], r64, bound, valid
    for a in R.DW_CASES:
        c, r64 = _dw_eval(*a)
        yield _dw_eval(*a, mut=mut)[1], r64, _dw_bound(c), None


def _dds_family(mut):
    for C in (32, 192):
        for T, dil, m in R.dds_single_cases(32, C):
            c, r64, tol, valid = R.dds_single_eval(C, T, dil, m)
            yield R.dds_layer_ref(c["x"], c["layers"][0], c["lens"], m, mut=mut), r64, tol, valid
    c, r64, tol, valid = R.dds_stack_eval(64, 3)
    yield R.dds_stack_ref(c["x"], c["layers"], c["lens"], mut=mut), r64, tol, valid
    # head, tail, head + tail: the ConvFlow's shape
    for rows, head in ((None, True), (29, False), (29, True)):
        c, hd, tl, r64, tol, valid = R.dds_flow_eval(192, 1, rows, head)
        h = R.cf_pre_ref(hd["z"], 1, hd["pre_w"], hd["pre_b"], hd["cond"]) if head else np.asarray(c["x"], np.float64)
        h = R.dds_stack_ref(h, c["layers"], c["lens"], mut=mut)
        yield (R.masked_proj_ref(h, tl["w"], tl["b"], c["lens"]) if rows else h), r64, tol, valid


def _spline_family(mut):
    for a in R.spline_cases():
        c, r64, tol, valid = R.spline_eval(*a)
        tol_el = np.zeros(r64.shape) + tol
        tol_el[:, c["ch0"] ^ 1] = R.spline_tol(tol, r64[:, c["ch0"] ^ 1], c["pr"], c["nb"], c["sqrt_c"])
        yield R.rqs_inverse_ref(c["pr"], c["z"], c["lens"], c["ch0"], c["nb"], c["sqrt_c"], mut=mut), r64, tol_el, valid


_FAMILIES = {
    "mean_c_minus_1": (_ln_family, _dds_family), "eps_1e-6": (_ln_family, _dds_family), "tanh_gelu": (_ln_family, _dds_family),
    "taps_reversed": (_ln_family, _dds_family), "input_not_masked": (_ln_family, _dds_family),
    "residual_of_masked_x": (_dds_family,), "mask_every_layer": (_dds_family,),
    "bin_off_by_one": (_spline_family,), "derivative_shifted": (_spline_family,), "widths_heights_swapped": (_spline_family,),
}


def test_the_mutation_list_is_whole():
    assert set(_FAMILIES) | {"tail_exclusive"} == set(R.MUTATIONS)


@pytest.mark.parametrize("mut", sorted(_FAMILIES))
def test_mutation_is_caught(mut):
    for family in _FAMILIES[mut]:
        worst = _caught(family(mut))
        print(f"{mut} in {family.__name__}: worst error / tolerance = {worst:.3g}")
        assert worst > 2.0, (mut, family.__name__, worst)


def test_each_feature_has_a_case_a_mutation_fails():
    """the coverage claim feature by feature, not family by family: the head, the tail, head + tail, the plane cases, every
    LN_* flag set and each bin count (both NBMAX paths, nb < NBMAX and nb == NBMAX) each hold a case that leaves its
    tolerance under a mutation"""
    def one(mutated, r64, tol, valid):
        return R.excess(mutated, r64, tol, valid)
    # head, tail, head + tail (the order of _dds_family's last three entries)
    flow = list(_dds_family("mean_c_minus_1"))[-3:]
    for name, entry in zip(("head", "tail", "head + tail"), flow):
        assert one(*entry) > 2.0, name
    by_flags, planes = {}, 0.0
    runs = R.ln_runs()
    for run, entry in zip(runs, _ln_family("mean_c_minus_1")):
        e = one(*entry)
        by_flags[run[3]] = max(by_flags.get(run[3], 0.0), e)
        if run[0] == "planes":
            planes = max(planes, e)
    assert set(by_flags) >= set(R.LN_FLAGS) and min(by_flags.values()) > 2.0, by_flags
    assert planes > 2.0, planes
    by_nb = {}
    for a, entry in zip(R.spline_cases(), _spline_family("bin_off_by_one")):
        by_nb[a[0]] = max(by_nb.get(a[0], 0.0), one(*entry))
    assert set(by_nb) == set(R.SPLINE_NB) and min(by_nb.values()) > 2.0, by_nb


def test_tail_bound_mutation_is_neutral_by_value():
    """An exclusive upper tail bound (x < 5 instead of x <= 5) changes which branch the input +5 takes, not the value: at
    the last knot the quadratic's root is exactly 1 (a = h (d1 - delta), b = h (2 delta - d1), c = -delta h: the
    discriminant is (h d1)^2), so the spline returns cumwidths[nb] = 5, the identity branch's own answer.  No by-value test
    can tell the two; what the GPU test pins at the bound is that +-5 stay within tolerance of 5 and that the next floats
    outward come back bit for bit."""
    for a in R.spline_cases():
        c, r64, _, valid = R.spline_eval(*a)
        m = R.rqs_inverse_ref(c["pr"], c["z"], c["lens"], c["ch0"], c["nb"], c["sqrt_c"], mut="tail_exclusive")
        assert float(np.abs(m - r64).max()) <= 1e-12
    x = np.full((1, 1), 5.0)
    pr = np.random.default_rng(0).standard_normal((1, 29, 1))
    assert abs(float(R.spline_inverse_ref(x, pr, 10, 3.0)[0, 0]) - 5.0) <= 1e-12


def test_a_nan_cannot_be_pooled_away():
    """excess() is what the GPU tests pool with max(): a NaN the kernel computes (not the 0xff fill) must come out as inf,
    because max(0.0, nan) is 0.0; outside the valid elements it does not count"""
    r64 = np.ones((2, 3, 4))
    got = r64.astype(np.float32)
    got[1, 2, 3] = np.nan
    assert max(0.0, R.excess(got, r64, 1e-6)) == np.inf
    got[1, 2, 3] = np.inf
    assert max(0.0, R.excess(got, r64, 1e-6)) == np.inf
    valid = np.ones((2, 1, 4), bool)
    valid[1, 0, 3] = False
    assert R.excess(got, r64, 1e-6, valid) == 0.0
