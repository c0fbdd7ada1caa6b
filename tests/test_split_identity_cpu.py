"""The identity conv_sx_pair_kernel's low plane rests on (csrc/sx_split.hip.hpp, split2h_pair_pk_mix), on the host in
_Float16 / fmaf (vits_test_split_identity: no device): with v clamped to +-65504 and h0 = f16(v),
    f16((v - h0) * 2048) == f16(fmaf(h0, -2048, v * 2048))
because v - h0 and the scalings are exact in fp32, so both round the same real number once.  Edge values and 2^22 random bit
patterns here; the exhaustive sweep over all 2^32 patterns (vits_test_split_identity_sweep) is run once per change of the
formula and noted in DESIGN 5.1b."""
import ctypes as C

import numpy as np

from phoonnx_amd import _ffi


def _both(x):
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    old, fused = np.empty(x.size, np.uint16), np.empty(x.size, np.uint16)
    assert lib.vits_test_split_identity(_ffi.ptr(x), x.size, _ffi.ptr(old), _ffi.ptr(fused)) == 0
    return old, fused


def _edges():
    small = np.array([2.0 ** -14, 1.5 * 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 1e-30], np.float32)
    sub32 = np.array([1, 2, 0x3fffff, 0x400000, 0x7fffff], np.uint32).view(np.float32)
    big = np.array([65504.0, 65519.9, 65520.0, 7e4, 1e5, np.inf], np.float32)
    exact = np.array([0.0, 1.0, 0.5, 1.5, 1023.5, 2047.0, 2048.0, 3.140625, 65472.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -12],
                     np.float32)
    v = np.concatenate([exact, small, sub32, big])
    return np.concatenate([v, -v]).astype(np.float32)


def test_edges_old_equals_fused_and_numpy():
    x = _edges()
    old, fused = _both(x)
    assert np.array_equal(old, fused), [(float(v), hex(a), hex(b)) for v, a, b in zip(x, old, fused) if a != b]
    # ... and both are what NumPy's float16 arithmetic gives
    c = np.clip(x, np.float32(-65504.0), np.float32(65504.0))
    want = ((c - c.astype(np.float16).astype(np.float32)) * np.float32(2048.0)).astype(np.float16).view(np.uint16)
    assert np.array_equal(old, want)


def test_random_bit_patterns_old_equals_fused():
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    old, fused = _both(x)
    bad = np.flatnonzero(old != fused)  # (a NaN leaves the clamp as a finite bound, in both forms alike)
    assert bad.size == 0, [(hex(int(bits[i])), hex(int(old[i])), hex(int(fused[i]))) for i in bad[:5]]


def test_sweep_form_agrees_on_a_slice():
    """the sweep entry over 2^20 consecutive patterns around 1.0 and around the fp16 subnormal range: no mismatch"""
    lib = _ffi.load()
    first_bad = C.c_uint32(0)
    for first in (0x3f800000 - (1 << 19), 0x33800000 - (1 << 19), 0xc77fe000 - (1 << 19)):
        assert lib.vits_test_split_identity_sweep(first, 1 << 20, C.byref(first_bad)) == 0, hex(first_bad.value)
