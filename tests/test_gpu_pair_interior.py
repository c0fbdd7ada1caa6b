"""conv_sx_pair_kernel decides once per workgroup whether its tile is INTERIOR - every column it reads or writes, the kept
columns and h = pad1 + pad2 more on each side, inside this utterance's tensor [0, end_b) - and runs such tiles through a body
compiled without the per-column predicates (clamped load columns, zero fills, `live ? v : 0`, tensor-end store predicate);
every other tile runs the predicated body.  What can go wrong: the classification itself (off by one at either side, the
per-utterance end of a ragged batch ignored), and an interior body that differs from the edge body in anything but the
predicates.  Every case: the fused launch as the generator issues it (vits_test_conv_pair_sx_epi: per-utterance ends, ACC,
ACC | DIV) against the two-launch form of the same arithmetic on each utterance's own columns, bit for bit; columns behind
an utterance's end must keep what the output tensor held.

Lengths, with BNo = 256 - (K - 1) dil2 kept columns per tile (tile n keeps [n BNo, (n + 1) BNo)); tile 1 is interior iff
end >= 2 BNo + h:
  short      T = 40: edge tiles only
  mid        T = 3 BNo + 17: tile 1 interior, tiles 0, 2, 3 edges
  exact      T = 3 BNo: the last tile ends with the tensor
  ragged     B = 2, T = 3 BNo + 17, lens = (T, BNo + 100): tile 1 interior for utterance 0 and an edge for utterance 1, whose
             tile 2 lies behind its end
  end-1/0/+1 lens = 2 BNo + h + (-1, 0, +1) in a T = 3 BNo + 17 tensor: the boundary of "interior" for tile 1"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLOPE = 0.1
DIV = 3.0

# (K, dil1, dil2, chain)
CONVS = {
    64: [(3, 1, 1, False), (11, 5, 1, False), (3, 1, 2, True)],
    32: [(3, 1, 1, False), (11, 5, 1, False), (3, 1, 2, True), (7, 3, 12, True)],
}
LENGTHS = ("short", "mid", "exact", "ragged", "end-1", "end+0", "end+1")
KINDS = ("normal", "neg", "const")
FLAGS = ((), ("acc",), ("acc", "div"))


def _x(kind, rng, B, C, T):  # (the input kinds of tests/test_gpu_pair_single_read.py)
    if kind == "const":   # a wrong zero fill of the halo shows as an error at the tensor's edges
        return np.full((B, C, T), 0.75, np.float32)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    if kind == "neg":     # leaky_relu(x) = 0.1 x there: a residual taken behind the activation is off by 0.9 |x|
        m = rng.random((B, C, T)) < 0.25
        x = np.where(m, -np.abs(x) * np.float32(900.0) - np.float32(100.0), x).astype(np.float32)
    return x


def _shape(length, K, d1, d2):
    """-> (B, T, lens or None)"""
    bno = 256 - (K - 1) * d2
    h = (d1 + d2) * (K - 1) // 2
    if length == "short":
        return 1, 40, None
    if length == "mid":
        return 1, 3 * bno + 17, None
    if length == "exact":
        return 1, 3 * bno, None
    T = 3 * bno + 17
    if length == "ragged":
        return 2, T, [T, bno + 100]
    return 1, T, [2 * bno + h + int(length[3:])]


@functools.lru_cache(maxsize=None)
def _case(C, conv, length, kind):
    """inputs and the two-launch result of each utterance's own columns (computed once, read-only)"""
    from phoonnx_amd.session import test_conv1d_sx
    K, d1, d2, chain = conv
    B, T, lens = _shape(length, K, d1, d2)
    rng = np.random.default_rng([C, K, d1, d2, int(chain), LENGTHS.index(length), KINDS.index(kind)])
    x = _x(kind, rng, B, C, T)
    w1 = (rng.standard_normal((C, C, K)) / np.sqrt(C * K)).astype(np.float32)
    w2 = (rng.standard_normal((C, C, K)) / np.sqrt(C * K) * 2).astype(np.float32)
    b1, b2 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    init = rng.standard_normal((B, C, T)).astype(np.float32)
    p1, p2 = d1 * (K - 1) // 2, d2 * (K - 1) // 2
    ends = [T] * B if lens is None else lens
    two = []
    for b in range(B):
        xb = np.ascontiguousarray(x[b:b + 1, :, :ends[b]])
        if chain:
            x1 = test_conv1d_sx(xb, w1, b1, dil=d1, pad_l=p1, in_slope=SLOPE, residual=True, precision="f16x3")
            r = test_conv1d_sx(x1, w2, b2, dil=d2, pad_l=p2, in_slope=SLOPE, residual=True, precision="f16x3")
        else:
            mid = test_conv1d_sx(xb, w1, b1, dil=d1, pad_l=p1, in_slope=SLOPE, precision="f16x3")
            r = test_conv1d_sx(mid, w2, b2, dil=d2, pad_l=p2, in_slope=SLOPE, precision="f16x3") + xb
        two.append(r[0])
    for a in (x, w1, b1, w2, b2, init, *two):
        a.setflags(write=False)
    return x, w1, b1, w2, b2, init, lens, ends, two


CASES = [(C, conv) for C in (32, 64) for conv in CONVS[C]]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "+".join(f) or "plain")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("C,conv", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_pair_tiles_equal_two_launches(C, conv, length, kind, flags):
    from phoonnx_amd.session import test_conv_pair_sx_epi
    K, d1, d2, chain = conv
    x, w1, b1, w2, b2, init, lens, ends, two = _case(C, conv, length, kind)
    r = test_conv_pair_sx_epi(x, w1, b1, w2, b2, flags=flags, dil1=d1, dil2=d2, chain=chain, slope=SLOPE, div=DIV,
                              out_init=init if flags else None, lens=lens)
    assert r["BNo"] == 256 - (K - 1) * d2, r
    epi = {(): 0, ("acc",): 32, ("acc", "div"): 96}[flags]
    assert r["kernel"].startswith("conv_sx_pair_kernel<") and f", {epi}, {'true' if chain else 'false'}, 1>" in r["kernel"], r["kernel"]
    got = r["out"]
    start = init if flags else np.zeros_like(x)
    for b in range(x.shape[0]):
        e = ends[b]
        want = two[b]
        if "acc" in flags:
            want = want + init[b, :, :e]
        if "div" in flags:
            want = want / np.float32(DIV)
        assert want.dtype == np.float32
        bad = got[b, :, :e] != want
        assert not bad.any(), (b, int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(np.abs(got[b, :, :e] - want).max()))
        assert np.array_equal(got[b, :, e:], start[b, :, e:]), (b, "columns behind the utterance's end were written")
