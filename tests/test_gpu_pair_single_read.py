"""conv_sx_pair_kernel: the x tile is loaded once, in the accumulator layout - the registers that feed
the fp16 split ARE the residual, only the halo columns go through whole-cell staging registers.  What that prologue can get
wrong and tests/test_gpu_parity.py's PAIR_CASES / CHAIN_CASES do not pin: the seams between tiles of BNo = 256 - (K2 - 1) dil2
kept columns, tensors shorter than c1's reach, the widest supported halos, the zero fill outside the tensor, and a residual
that must be raw x (not leaky_relu(x)).  Every case: the fused launch against the two-launch form of the same arithmetic,
bit for bit, at 64 channels (two workgroups per CU, four block columns per wave) and at 32 (three workgroups, two block
columns, all four channel groups in one wave).  None of these shapes is refused by the hook (sx_pair_supported: K >= 3,
2 (256 + halo1) <= 768, >= 200 kept columns at 64 channels, >= 160 at 32); the ones it does refuse are pinned by
test_conv_pair_sx_refuses_what_it_cannot_fuse and left out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _x(kind, rng, B, C, T):
    if kind == "const":   # a wrong zero fill of the halo shows as an error at the tensor's edges
        return np.full((B, C, T), 0.75, np.float32)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    if kind == "neg":     # leaky_relu(x) = 0.1 x there: a residual taken behind the activation is off by 0.9 |x|
        m = rng.random((B, C, T)) < 0.25
        x = np.where(m, -np.abs(x) * np.float32(900.0) - np.float32(100.0), x).astype(np.float32)
    return x


def _weights(rng, C, K, s2):
    w1 = (rng.standard_normal((C, C, K)) / np.sqrt(C * K)).astype(np.float32)
    w2 = (rng.standard_normal((C, C, K)) / np.sqrt(C * K) * s2).astype(np.float32)
    return w1, rng.standard_normal(C).astype(np.float32), w2, rng.standard_normal(C).astype(np.float32)


def _seams(bno, ns):
    return [bno * n + d for n in ns for d in (-1, 0, 1)]


PAIR = (
    # (B, T, K, dil1, kind): second conv dilation 1 -> BNo = 254 / 250 / 246 kept columns for k = 3 / 7 / 11
    [(1, T, 3, 1, "normal") for T in _seams(254, (1, 3))] +
    [(1, T, 7, 3, "normal") for T in _seams(250, (1, 2))] +
    [(1, T, 11, 5, "normal") for T in _seams(246, (1, 2))] +      # k = 11, d = 5: the widest halo (25 columns a side)
    [(2, T, 11, 5, "normal") for T in (1, 24, 25, 26)] +          # the tensor is shorter than / as long as c1's reach
    [(1, 1, 3, 1, "normal"), (2, 1, 7, 5, "normal")] +
    [(3, 600, 11, 5, "const"), (3, 255, 3, 1, "const"), (3, 26, 11, 5, "const")] +
    [(2, 700, 3, 3, "neg"), (1, 493, 11, 5, "neg"), (2, 251, 7, 1, "neg")]
)


PAIR32 = (
    [(1, T, 3, 1, "normal") for T in _seams(254, (1, 2))] +
    [(1, T, 11, 5, "normal") for T in _seams(246, (1, 2))] +
    [(2, T, 11, 5, "normal") for T in (1, 24, 25, 26)] +
    [(3, 600, 11, 5, "const"), (3, 255, 3, 1, "const"), (2, 700, 7, 3, "neg")]
)


@pytest.mark.parametrize("B,T,K,dil,kind,C", [c + (64,) for c in PAIR] + [c + (32,) for c in PAIR32])
def test_pair_single_read_equals_two_launches(B, T, K, dil, kind, C):
    from phoonnx_amd.session import test_conv1d_sx, test_conv_pair_sx
    rng = np.random.default_rng(C * 1000 + 131 * T + 7 * K + dil + B)
    x = _x(kind, rng, B, C, T)
    w1, b1, w2, b2 = _weights(rng, C, K, 3)
    got = test_conv_pair_sx(x, w1, b1, w2, b2, dil1=dil, dil2=1, slope=0.1)
    pad1, pad2 = dil * (K - 1) // 2, (K - 1) // 2
    mid = test_conv1d_sx(x, w1, b1, dil=dil, pad_l=pad1, in_slope=0.1, precision="f16x3")
    two = test_conv1d_sx(mid, w2, b2, dil=1, pad_l=pad2, in_slope=0.1, precision="f16x3") + x
    assert got.shape == x.shape
    assert np.array_equal(got, two), float(np.abs(got - two).max())


CHAIN = (
    # (B, T, K, dil1, dil2, kind): BNo = 252 for k = 3, d2 = 2; 232 for k = 5, d2 = 6 (the widest second reach 64 channels fuse)
    [(1, T, 3, 1, 2, "normal") for T in _seams(252, (1, 3))] +
    [(1, T, 5, 2, 6, "normal") for T in _seams(232, (1, 2))] +
    [(2, 1, 5, 2, 6, "normal"), (2, 3, 5, 2, 6, "normal"), (1, 1, 3, 1, 2, "normal")] +
    [(3, 500, 5, 2, 6, "const"), (3, 253, 3, 1, 2, "const")] +
    [(2, 700, 3, 1, 2, "neg"), (1, 465, 5, 2, 6, "neg")]
)


CHAIN32 = (
    # 32 channels fuse down to 160 kept columns: k = 7, d = (3, 12) keeps 184 (halo 9 a side in, 36 a side between the convs)
    [(1, T, 3, 1, 2, "normal") for T in _seams(252, (1, 2))] +
    [(1, T, 7, 3, 12, "normal") for T in _seams(184, (1, 3))] +
    [(2, 1, 7, 3, 12, "normal"), (2, 8, 7, 3, 12, "normal")] +
    [(3, 500, 7, 3, 12, "const"), (3, 253, 3, 1, 2, "const"), (2, 700, 5, 2, 6, "neg")]
)


@pytest.mark.parametrize("B,T,K,d1,d2,kind,C", [c + (64,) for c in CHAIN] + [c + (32,) for c in CHAIN32])
def test_chain_single_read_equals_two_launches(B, T, K, d1, d2, kind, C):
    from phoonnx_amd.session import test_conv1d_sx, test_conv_pair_sx
    rng = np.random.default_rng(C * 1000 + 1000 + 131 * T + 7 * K + d1 + B)
    x = _x(kind, rng, B, C, T)
    w1, b1, w2, b2 = _weights(rng, C, K, 2)
    got = test_conv_pair_sx(x, w1, b1, w2, b2, dil1=d1, dil2=d2, chain=True, slope=0.1)
    p1, p2 = d1 * (K - 1) // 2, d2 * (K - 1) // 2
    x1 = test_conv1d_sx(x, w1, b1, dil=d1, pad_l=p1, in_slope=0.1, residual=True, precision="f16x3")
    two = test_conv1d_sx(x1, w2, b2, dil=d2, pad_l=p2, in_slope=0.1, residual=True, precision="f16x3")
    assert got.shape == x.shape
    assert np.array_equal(got, two), float(np.abs(got - two).max())
