"""The activation -> operand-plane helpers of csrc/sx_split.hip.hpp by value: a small kernel (split_forms_kernel,
test_dev.hip.hpp) applies lrelu_max, the clamp and the two-plane split - the engine-wide form and the one conv_sx_pair_kernel
uses (low plane by v_fma_mixlo/hi_f16, guard magnitude by v_max3_f32) - to an array; the planes, the guard magnitude and the
reconstruction of the high plane are compared bit for bit with NumPy's float32 / float16 arithmetic.  The fused-launch tests
compare two paths that share these helpers; this is the independent pin."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOPE = 0.1


def _edges():
    f16_exact = np.array([1.0, -1.0, 0.5, 1.5, 1023.5, 2047.0, -2048.0, 3.140625, 65472.0, -0.333251953125], np.float32)
    small = np.array([2.0 ** -14, 1.5 * 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1e-30], np.float32)
    sub32 = np.array([1, 2, 0x3fffff, 0x400000, 0x7fffff], np.uint32).view(np.float32)    # fp32 subnormals
    big = np.array([65504.0, 65519.9, 65520.0, 7e4], np.float32)
    v = np.concatenate([np.array([0.0, -0.0], np.float32), f16_exact, small, -small, sub32, -sub32, big, -big,
                        np.array([-1e5, 1e5, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -12, 2049.0, 4097.5, -4097.5], np.float32)])
    assert v.size % 2 == 0, v.size
    return v.astype(np.float32)


def _random(n=1 << 20):
    """every fp16 exponent (and the ranges below and above it): sign * 2^e * [1, 2), e uniform in [-30, 17]"""
    rng = np.random.default_rng(20240607)
    e = rng.integers(-30, 18, n)
    m = 1.0 + rng.random(n)
    s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return (s * m * np.exp2(e)).astype(np.float32)


def _reference(x, slope):
    s = np.float32(slope)
    a = np.maximum(x, x * s)                       # float32
    pk = np.maximum(np.abs(a[0::2]), np.abs(a[1::2]))
    c = np.clip(a, np.float32(-65504.0), np.float32(65504.0))
    h0 = c.astype(np.float16)                      # round to nearest even, subnormals kept
    h1 = ((c - h0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    f = h0.astype(np.float32)
    rec = np.where(f < 0, f * (np.float32(1.0) / s), f).astype(np.float32)
    return h0, h1, pk, rec


@pytest.fixture(scope="module")
def values():
    x = np.concatenate([_edges(), _random()])
    x.setflags(write=False)
    return x, _reference(x, SLOPE)


@pytest.mark.parametrize("form", ["engine", "pair"])
def test_split_forms_equal_numpy(values, form):
    from phoonnx_amd.session import test_split_forms
    x, (h0, h1, pk, rec) = values
    r = test_split_forms(x, slope=SLOPE, form=form)
    for name, got, want in (("h0", r["h0"].view(np.uint16), h0.view(np.uint16)), ("h1", r["h1"].view(np.uint16), h1.view(np.uint16)),
                            ("pk", r["pk"].view(np.uint32), pk.view(np.uint32)), ("rec", r["rec"].view(np.uint32), rec.view(np.uint32))):
        bad = np.flatnonzero(got != want)
        src = x if name != "pk" else x[0::2]
        assert bad.size == 0, (form, name, int(bad.size), [(float(src[i]), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]])


def test_slope_and_overflow_cases():
    """-1e5 with slope 0.1 is -1e4 (in range); +-7e4 clamps to +-65504 with a zero low plane, and the guard still sees 7e4"""
    from phoonnx_amd.session import test_split_forms
    x = np.array([-1e5, 7e4, -7e4 / 0.1, 65519.9], np.float32)
    r = test_split_forms(x, slope=SLOPE, form="pair")
    want_a = np.maximum(x, x * np.float32(SLOPE))
    assert r["h0"].astype(np.float32).tolist() == np.clip(want_a, -65504, 65504).astype(np.float16).astype(np.float32).tolist()
    assert float(r["h0"][1]) == 65504.0 and float(r["h1"][1]) == 0.0
    assert r["pk"].tolist() == [float(max(abs(want_a[0]), abs(want_a[1]))), float(max(abs(want_a[2]), abs(want_a[3])))]
