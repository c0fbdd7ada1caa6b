"""tests/attention_ref.py (the float64 reference of the attention kernel tests) against the C oracle's attention core on every
shape family of tests/test_gpu_attention.py, and against the closed forms of the structured band inputs.  No GPU.

The oracle is an fp32 evaluation with sequential sums over up to T keys and dk channels, and it rounds q / sqrt(dk) where the
reference scales the finished dot product; it is held to 16 x the error of the reference's own float32 evaluation (a
pairwise-summing fp32 evaluation of the same formula), at least 2^-20 max|want|, under the ceilings of the first attention
tests.  Queries >= len are zeros in the reference (what the kernels write) and softmaxes over masked logits in the oracle:
only valid queries are compared."""
import numpy as np
import pytest

import attention_ref as ar

A16_L = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 161, 193)
F32_L = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 161)


def _against_oracle(qkv, heads, rk, rv, lens, sharp=False):
    from vits_oracle import attention_core
    want = ar.attention_ref(qkv, heads, rk, rv, lens)
    f32 = ar.attention_ref_f32(qkv, heads, rk, rv, lens)
    got = attention_core(qkv, heads, rk, rv, lens)
    e32 = float(np.abs(f32 - want).max())
    scalar = max(16 * e32, 2.0 ** -20 * float(np.abs(want).max()))
    atol, rtol = ar.SHARP_CEILING if sharp else ar.ORDINARY_CEILING
    worst = 0.0
    for b in range(qkv.shape[0]):
        L = int(min(lens[b], qkv.shape[2]))
        bound = np.minimum(scalar, atol + rtol * np.abs(want[b, :, :L]))
        err = np.abs(got[b, :, :L] - want[b, :, :L])
        worst = max(worst, float((err / bound).max()) if err.size else 0.0)
        assert not want[b, :, L:].any()
    return worst, e32


@pytest.mark.parametrize("dk", [8, 12, 16, 32, 48, 64, 96, 100, 104, 128])
def test_reference_matches_the_oracle_over_the_length_family(dk):
    Ls = sorted(set(A16_L) | set(F32_L)) if dk in (32, 64, 96) else F32_L
    worst = 0.0
    for n, L in enumerate(Ls):
        T = L + (11 if n % 2 else 0)
        qkv, rk, rv = ar.random_case(1000 * dk + L, 2, 2, dk, T)
        r, e32 = _against_oracle(qkv, 2, rk, rv, np.asarray([L, (L + 1) // 2], np.int64))
        worst = max(worst, r)
    print(f"dk {dk}: oracle worst {worst:.3f} x bound over {len(Ls)} lengths")
    assert worst <= 1.0


@pytest.mark.parametrize("B,heads,dk", [(5, 2, 96), (9, 1, 32), (3, 2, 16)])
def test_reference_matches_the_oracle_on_ragged_batches_with_filled_padding(B, heads, dk):
    """the independence family: rows of length 1, rows whose later query tiles are all padding, the columns behind len at
    +-1000 - and the reference's valid outputs do not move by a bit when that padding is zeroed"""
    T = 150
    lens = np.asarray([(T, 1, 97, 64, 33, 150, 2, 129, 65)[b % 9] for b in range(B)], np.int64)
    qkv, rk, rv = ar.random_case(B * 31 + dk, B, heads, dk, T)
    zeroed = np.array(qkv, copy=True)
    for b, L in enumerate(lens):
        qkv[b, :, L:] = 1000.0 * np.where(np.arange(T - L) % 2 == 0, 1.0, -1.0)
        zeroed[b, :, L:] = 0.0
    r, e32 = _against_oracle(qkv, heads, rk, rv, lens)
    print(f"B {B} x {heads} heads dk {dk}: oracle {r:.3f} x bound (float32 evaluation {e32:.2e})")
    assert r <= 1.0
    assert np.array_equal(ar.attention_ref(qkv, heads, rk, rv, lens), ar.attention_ref(zeroed, heads, rk, rv, lens))
    assert np.array_equal(ar.attention_ref(qkv, heads, rk, rv, lens + 7 * (lens == T)), ar.attention_ref(qkv, heads, rk, rv, lens))


@pytest.mark.parametrize("window", [0, 1, 2, 3, 4])
def test_reference_matches_the_oracle_with_unit_scale_bands(window):
    qkv, rk, rv = ar.random_case(77 + window, 2, 2, 32, 76, window, rel_scale=1.0)
    r, e32 = _against_oracle(qkv, 2, rk, rv, np.asarray([65, 3], np.int64), sharp=True)
    print(f"window {window}: oracle {r:.3f} x bound (float32 evaluation {e32:.2e})")
    assert r <= 1.0


@pytest.mark.parametrize("kind", ar.RESCALE_KINDS)
@pytest.mark.parametrize("dk", [32, 96])
def test_reference_matches_the_oracle_on_the_rescale_family(kind, dk):
    qkv, rk, rv, lens = ar.rescale_case(kind, 5, 2, dk, 161, 172)
    r, e32 = _against_oracle(qkv, 2, rk, rv, lens, sharp=True)
    print(f"{kind} dk {dk}: oracle {r:.3f} x bound (float32 evaluation {e32:.2e})")
    assert r <= 1.0


def _band_lengths(w):
    return sorted({L for L in (1, 2, w, w + 1, 33, 65) if L >= 1})


@pytest.mark.parametrize("window", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("v_zero", [False, True])
def test_one_hot_band_inputs_give_their_closed_forms(window, v_zero):
    """every m*, every length of the band family: the reference lands on V[:, i + m* - w] + E_v[m*] (the uniform average where
    that key does not exist) to e^-64 and float64 rounding - and a band shifted by one entry would not: the check below moves
    m* by one and requires a difference of order |V|, |E_v|"""
    rng = np.random.default_rng(window * 2 + int(v_zero))
    worst = worst_oracle = 0.0
    for L in _band_lengths(window):
        for m_star in range(2 * window + 1):
            qkv, rk, rv, lens = ar.band_one_hot(16, 2, window, m_star, L, L + 5, rng, v_zero=v_zero)
            want = ar.attention_ref(qkv, 2, rk, rv, lens)
            closed = ar.band_one_hot_closed_form(qkv, 2, rk, rv, lens, m_star)
            err = float(np.abs(want - closed).max())
            worst = max(worst, err)
            assert err < 1e-12 * max(1.0, float(np.abs(closed).max())), (L, m_star, err)
            assert not want[:, :, L:].any()
            r, _ = _against_oracle(qkv, 2, rk, rv, lens, sharp=True)
            worst_oracle = max(worst_oracle, r)
            assert r <= 1.0, (L, m_star, r)
            if window and L > window + 1:
                other = ar.band_one_hot_closed_form(qkv, 2, rk, rv, lens, (m_star + 1) % (2 * window + 1))
                assert float(np.abs(other - closed).max()) > 0.5
    print(f"window {window} v_zero {v_zero}: reference - closed form {worst:.2e}; oracle {worst_oracle:.3f} x bound")


def test_float32_evaluation_is_a_float32_evaluation():
    qkv, rk, rv = ar.random_case(3, 1, 2, 32, 70)
    lens = np.asarray([65], np.int64)
    f32 = ar.attention_ref_f32(qkv, 2, rk, rv, lens)
    want = ar.attention_ref(qkv, 2, rk, rv, lens)
    assert f32.dtype == np.float32 and want.dtype == np.float64
    e = float(np.abs(f32 - want).max())
    assert 0 < e < 1e-5
    bound, scalar = ar.tolerance(want, f32)
    assert scalar >= 2.0 ** -22 * np.abs(want).max() and (bound <= 2e-5 + 1e-4 * np.abs(want)).all()


def test_planes_round_trip():
    x = (np.random.default_rng(0).standard_normal((2, 16, 9)) * 100).astype(np.float32)
    pl = ar.split_planes(x)
    assert not pl[:, 2].any()
    np.testing.assert_allclose(ar.planes_value(pl), x.astype(np.float64), rtol=3e-7, atol=1e-9)
