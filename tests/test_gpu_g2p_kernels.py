"""g2p_attention_kernel, g2p_rmsnorm_kernel and g2p_argmax_kernel (phoonnx_amd/csrc/g2p.hip) by value, one launch at a time through
g2p_test_attention / g2p_test_rmsnorm / g2p_test_argmax, against the float64 references of tests/g2p_kernels_ref.py (pinned on the
CPU by tests/test_g2p_kernels_ref_cpu.py).

Attention runs in the five forms the engine launches - the batched encoder (seg = S, lens per sequence), the prefill's self and
cross attention ([C][T] queries, one sequence), the decoder step's self attention (one query per sequence at q_off = t over a
cache of t + 1 keys) and cross attention (lens per sequence), the step forms with the narrow ([NB][C]) and the wide ([C][NB])
query strides - at key counts on both sides of every boundary of g2p_attention_body_t<64>: a lane round (64 keys), the value
prefetch (256), a pass of the score loop (256), and the far end of the bucket table (1023); d_kv 64 takes that body, 16 / 40 /
20 / 128 the generic one (whole groups of eight channels, no whole round of 32, a ragged tail, more than one round).  A prefill
of up to 65 columns runs whole; a longer one at its query columns 0, 63 and 64, 255 and 256, and the last (each group one launch,
placed through q_off and seg: g2p_kernels_ref.prefill_groups).

Four kinds of evidence per launch: float64 on random data (bound: 4 x what NumPy float32 is away from float64 on the same
arrays, the rule of F32_GAP in test_gpu_g2p_width.py); NaN in every key / value the launch must not read (same bits); a
sentinel in every element of `out` it must not write; and integer families whose answer is exact, so that ONE dropped, doubled
or shifted key shows (a whole-model logit moves by far less than its tolerance when one of 300 keys goes missing)."""
import numpy as np
import pytest

import g2p_kernels_ref as gr

pytestmark = pytest.mark.gpu

# max over every random launch of this file at the head width of |NumPy float32 - float64| / max|v| (CPU, reference against
# reference: test_recorded_attention_gap_is_the_measured_one holds each to its measurement); the kernel's bound is 4 x that.
# ATT_ENGINE_WORST: the kernel's worst launch in the same unit, measured on an MI355X (a record, not a bound: 0.18 .. 0.26 of it).
ATT_F32_GAP = {16: 6.98e-7, 20: 5.61e-7, 40: 9.21e-7, 64: 1.108e-6, 128: 1.504e-6}   # measured 6.977e-7, 5.609e-7, 9.210e-7, 1.1073e-6, 1.5033e-6
ATT_ENGINE_WORST = {16: 5.07e-7, 20: 4.59e-7, 40: 8.00e-7, 64: 9.63e-7, 128: 1.56e-6}
RMS_F32_GAP = 5.85e-7     # measured 5.842e-7: the same for g2p_rmsnorm_kernel, in units of max|y| of the case; the kernel: 1.4e-7


def ulps(got, want):
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def run(c):
    from phoonnx_amd import g2p
    return g2p.test_attention(**c)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_ownership(c, got, what):
    """every element the strides do not address keeps the bits it came in with; every one they address was written"""
    own = gr.owned(c)
    rest = np.ones(got.size, bool)
    rest[own.reshape(-1)] = False
    assert np.array_equal(bits(got[rest]), bits(c["out"][rest])), what
    assert np.isfinite(got[own]).all() and not np.any(got[own] == gr.SENTINEL), what
    return got[own]


# ------------------------------------------------------------------------------------------------ float64, poison, ownership
@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
@pytest.mark.parametrize("form", gr.FORMS)
def test_attention_matches_float64_and_reads_and_writes_only_what_it_owns(form, dk):
    worst = 0.0
    for Tk in gr.DK_TKS[dk]:
        for n, c in enumerate(gr.random_cases(form, Tk, dk)):
            what = f"{form} dk {dk} Tk {Tk} launch {n} (cols {c['cols']} q_off {c['q_off']})"
            got = run(c)
            mine = check_ownership(c, got, what)
            ref = gr.attention_ref(c)[gr.owned(c)]
            err = float(np.abs(mine.astype(np.float64) - ref).max()) / float(np.abs(c["v"]).max())
            bound = 4 * ATT_F32_GAP[dk]
            print(f"{what}: err {err:.3e} of max|v|  bound {bound:.3e}")
            worst = max(worst, err)
            assert err <= bound, (what, err, bound)
            again = run(gr.poisoned(c))
            assert np.array_equal(bits(again), bits(got)), what      # NaN where it must not read: the same bits
    print(f"{form} dk {dk}: worst {worst:.3e} of max|v|")


# ------------------------------------------------------------------------------------------------ exact families
@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
@pytest.mark.parametrize("form", gr.FORMS)
def test_attention_returns_a_selected_key_bit_for_bit(form, dk):
    """q = 40 e_0, k channel 0 one at key j* only, no bias: out = v[:, j*] exactly (g2p_kernels_ref.selected_key_cases), for j*
    0, 63, 64, 255, 256, 257 and lim - 1 - the first and last key of every lane round, prefetch round and pass."""
    n = 0
    for Tk in gr.DK_TKS[dk]:
        for c, want in gr.selected_key_cases(form, Tk, dk):
            got = check_ownership(c, run(c), (form, dk, Tk))
            bad = int((bits(got) != bits(want)).sum())
            print(f"{form} dk {dk} Tk {Tk} selected key, launch {n}: {bad} of {got.size} outputs differ")
            assert bad == 0, (form, dk, Tk)
            n += 1


@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
@pytest.mark.parametrize("form", gr.FORMS)
def test_attention_means_are_exact_sums_over_exactly_the_keys(form, dk):
    """Uniform: q = 0, no bias - out = (exact integer sum over the lim keys) / lim to 2 ulp, channel 0 = 1, channel 1 = (lim - 1)
    / 2.  Bucket selection (the forms with a bias): one bucket per head lifted by 40 - out = the mean over exactly the keys
    whose (j - ipos) falls in it: the lut index, q_off and the head's bias column."""
    for Tk in gr.DK_TKS[dk]:
        for c, sums, cnt in gr.uniform_cases(form, Tk, dk):
            got = check_ownership(c, run(c), (form, dk, Tk))
            u = float(ulps(got, (sums / np.repeat(cnt, dk, 0)).astype(np.float32)).max())
            one = float(ulps(got[::dk], np.ones_like(got[::dk])).max())
            print(f"{form} dk {dk} Tk {Tk} uniform: {u:.2f} ulp, channel 0 against 1: {one:.2f} ulp")
            assert u <= 2 and one <= 2, (form, dk, Tk, u, one)
        if form in ("enc", "pre_self", "step_self_narrow", "step_self_wide"):
            for c, sums, cnt in gr.bucket_cases(form, Tk, dk):
                got = check_ownership(c, run(c), (form, dk, Tk))
                u = float(ulps(got, (sums / np.repeat(cnt, dk, 0)).astype(np.float32)).max())
                print(f"{form} dk {dk} Tk {Tk} q_off {c['q_off']} bucket selection: {u:.2f} ulp")
                assert u <= 2, (form, dk, Tk, u)


@pytest.mark.parametrize("form", gr.FORMS)
def test_the_two_attention_bodies_agree(form):
    """d_kv 64 (the compile-time body) against the same scores through the generic body: d_kv 128 with the upper 64 channels of q
    zero - a second opinion beside the reference, within the bound of the float64 comparison."""
    for Tk in gr.DK_TKS[128]:
        for c in gr.random_cases(form, Tk, 64):
            w, lo = gr.widened(c)
            a, b = run(c)[gr.owned(c)], run(w)[gr.owned(w)[lo]]
            d = float(np.abs(a.astype(np.float64) - b).max()) / float(np.abs(c["v"]).max())
            print(f"{form} Tk {Tk}: |body<64> - generic body| {d:.3e} of max|v|  bound {4 * ATT_F32_GAP[64]:.3e}")
            assert d <= 4 * ATT_F32_GAP[64], (form, Tk, d)


def test_attention_hook_refuses_what_the_kernel_cannot_take():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import SessionError
    c = gr.random_cases("enc", 5, 16)[0]
    lib = _ffi.load()

    def refused(**change):
        with pytest.raises(SessionError):
            run(dict(c, **change))
        assert lib.g2p_last_error(None).decode()

    run(c)
    refused(Tk=0)
    refused(Tk=gr.KMAX)
    refused(lens=np.array([5, 0, 5, 4], np.int32))
    refused(lens=np.array([5, 1, 6, 4], np.int32))
    refused(cols=c["cols"] - 1, q=c["q"][:-1], out=c["out"][:-1], lens=None)    # not whole sequences
    refused(q_off=gr.KMAX - 2)                                                   # the lut index would turn negative
    refused(lut=np.where(np.arange(2 * gr.KMAX - 1) == 7, gr.NUM_BUCKETS, c["lut"]).astype(np.int32))
    refused(lut=None)                                                            # bias without lut
    refused(q_cs=1, q_ts=1, q=c["q"][:32 + 19], out=c["out"][:32 + 19])          # two elements in one place
    refused(k=c["k"][:-8], v=c["v"][:-8])                                        # the last sequence's keys do not fit
    refused(kp=4)
    assert lib.g2p_test_attention(0, None, None, 20, 1, None, None, 1, 5, 0, None, 0, None, 2, 16, 20, 5, None, 5, 0, 0) < 0


# ------------------------------------------------------------------------------------------------ RMS norm
@pytest.mark.parametrize("C", gr.RMS_C)
def test_rmsnorm_matches_float64_and_leaves_the_pitch_padding(C):
    from phoonnx_amd import g2p
    for T in gr.RMS_T:
        x, g, y, eps = gr.rms_case(C, T)
        got = g2p.test_rmsnorm(x, g, y, T, eps)
        assert np.array_equal(bits(got[:, T:]), bits(y[:, T:])), (C, T)
        ref = gr.rmsnorm_ref(x, g, y, T, eps)[:, :T]
        err = float(np.abs(got[:, :T].astype(np.float64) - ref).max() / np.abs(ref).max())
        print(f"rmsnorm C {C} T {T}: err {err:.3e} of max|y|  bound {4 * RMS_F32_GAP:.3e}")
        assert err <= 4 * RMS_F32_GAP, (C, T, err)
        x, g, y, eps = gr.rms_case(C, T, exact=True)     # x = +-1, eps = 0: mean x^2 = 1, y = x g
        got = g2p.test_rmsnorm(x, g, y, T, eps)
        want = x[:, :T] * g[:, None]
        assert np.array_equal(bits(got[:, T:]), bits(y[:, T:])), (C, T)
        u = float(ulps(got[:, :T], want).max())
        print(f"rmsnorm C {C} T {T} exact family: {u:.2f} ulp")
        assert (np.array_equal(bits(got[:, :T]), bits(want)) if C & (C - 1) == 0 else u <= 2), (C, T, u)


def test_rmsnorm_hook_checks_its_arguments():
    from phoonnx_amd import g2p
    from phoonnx_amd.session import SessionError
    x, g, y, eps = gr.rms_case(8, 3)
    with pytest.raises(SessionError):
        g2p.test_rmsnorm(x, g, y, 0, eps)
    with pytest.raises(SessionError):
        g2p.test_rmsnorm(x, g, y, 7, eps)          # more columns than x's pitch
    with pytest.raises(SessionError):
        g2p.test_rmsnorm(x, g, y, 3, -1.0)


# ------------------------------------------------------------------------------------------------ argmax
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("V", gr.ARGMAX_V)
def test_argmax_returns_the_first_maximum_in_both_layouts(wide, V):
    """The maximum at 0, 255, 256 and V - 1; equal maxima at (5, 300), (255, 256), (0, V - 1): the lower index; -0.0 = +0.0; a row
    of -inf: 0; a row of NaN: 0 (an id inside [0, V), not the kernel's starting index); NaNs among finite values: the first
    maximum of the others.  ids and the host copy agree; every slot but the written one keeps its value."""
    from phoonnx_amd import g2p
    for NB in gr.ARGMAX_NB:
        rows, kinds = gr.argmax_rows(V, NB)
        want = np.array([gr.argmax_ref(r) for r in rows], np.int64)
        pitch, lb, size, at = gr.argmax_layout(wide, V, NB)
        lg = np.zeros(size, np.float32)
        lg[at] = rows
        for slot in (3, 0):
            ids = np.arange(NB * 5, dtype=np.int64).reshape(NB, 5) - 1000
            a, b = g2p.test_argmax(lg, V, pitch, 0, lb, NB, ids, slot)
            print(f"argmax wide {wide} V {V} NB {NB} slot {slot}: {int((a[:, slot] != want).sum())} rows differ")
            assert np.array_equal(a[:, slot], want), (wide, V, NB, slot, a[:, slot], want)
            assert np.array_equal(a, b)
            keep = np.arange(5) != slot
            assert np.array_equal(a[:, keep], ids[:, keep])


def test_argmax_hook_checks_its_arguments():
    from phoonnx_amd import g2p
    from phoonnx_amd.session import SessionError
    ids = np.zeros((2, 3), np.int64)
    with pytest.raises(SessionError):
        g2p.test_argmax(np.zeros(8, np.float32), 4, 1, 0, 4, 2, ids, 3)      # slot outside a row of ids
    with pytest.raises(SessionError):
        g2p.test_argmax(np.zeros(8, np.float32), 0, 1, 0, 4, 2, ids, 0)
