"""tests/sx_epi_ref.py against independent statements of the same things: torch's convs, the literal multi-receptive-field
mean, "zero the input, crop the output" for the ragged ends, and the ownership masks written out by hand."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sx_epi_ref import sx_ends, sx_epi_ref


def _data(seed, B, Cin, Cout, T, K, stride=1):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, Cin, T))
    w = r.standard_normal((Cin, Cout, K) if stride > 1 else (Cout, Cin, K)) / np.sqrt(Cin * K)
    return r, x, w, r.standard_normal(Cout)


@pytest.mark.parametrize("K,dil,pad_l", [(3, 2, None), (7, 1, None), (1, 1, None), (3, 3, 0), (3, 3, 6)])
def test_conv_part_matches_torch(K, dil, pad_l):
    r, x, w, b = _data(K * 10 + dil, 2, 16, 32, 37, K)
    bb = r.standard_normal((2, 40))
    got = sx_epi_ref(x, w, b, dil=dil, pad_l=pad_l, bias_b=bb, islope=0.1)
    pl = dil * (K - 1) // 2 if pad_l is None else pad_l
    xin = F.pad(F.leaky_relu(torch.from_numpy(x), 0.1), (pl, dil * (K - 1) - pl))
    want = F.conv1d(xin, torch.from_numpy(w), torch.from_numpy(b), dilation=dil).numpy() + bb[:, :32, None]
    assert got["out"].dtype == np.float64 and got["planes"] is None and got["own_pl"] is None
    assert np.abs(got["out"] - want).max() < 1e-12
    assert got["own"].all()


@pytest.mark.parametrize("u,K", [(2, 4), (8, 16), (4, 8)])
def test_transposed_part_matches_torch(u, K):
    r, x, w, b = _data(u, 2, 16, 32, 19, K, stride=u)
    got = sx_epi_ref(x, w, b, stride=u, planes=True, oslope2=0.1)
    want = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=u, padding=(K - u) // 2)
    assert got["out"].shape == (2, 32, 19 * u)
    assert np.abs(got["out"] - want.numpy()).max() < 1e-12
    assert np.abs(got["planes"] - F.leaky_relu(want, 0.1).numpy()).max() < 1e-12


def test_rule_order_is_the_multi_receptive_field_mean():
    # three ResBlock outputs rb_k = conv_k(lrelu(x)) + x; xs = rb0, xs += rb1, x' = (xs + rb2) / 3 stored as planes of
    # leaky_relu(x', 0.1): the three launches conv_sx()'s callers form (First, Accum, StageOut)
    r, x, _, _ = _data(5, 2, 32, 32, 41, 3)
    ws = [r.standard_normal((32, 32, 3)) / 10 for _ in range(3)]
    bs = [r.standard_normal(32) for _ in range(3)]
    xt = torch.from_numpy(x)
    rb = [F.conv1d(F.pad(F.leaky_relu(xt, 0.1), (k + 1, k + 1)), torch.from_numpy(ws[k]), torch.from_numpy(bs[k]), dilation=k + 1) + xt
          for k in range(3)]
    mean = ((rb[0] + rb[1] + rb[2]) / 3).numpy()
    xs = sx_epi_ref(x, ws[0], bs[0], flags=("res",), dil=1, res=x, islope=0.1)["out"]
    xs = sx_epi_ref(x, ws[1], bs[1], flags=("res", "acc"), dil=2, res=x, old_out=xs, islope=0.1)["out"]
    last = sx_epi_ref(x, ws[2], bs[2], flags=("res", "acc", "div", "no_raw_store"), dil=3, res=x, old_out=xs, div=3.0, islope=0.1,
                      planes=True, oslope2=0.1, sentinel=7.0)
    assert np.abs(last["planes"] - np.where(mean >= 0, mean, mean * 0.1)).max() < 1e-12
    assert np.abs(last["value"] - mean).max() < 1e-12
    # no_raw_store: the raw tensor is the accumulate operand and keeps every element
    assert not last["own"].any() and np.array_equal(last["out"], xs)
    # the order matters: dividing before accumulating is another number
    assert np.abs((rb[2].numpy() / 3 + xs) - mean).max() > 1e-2
    # the raw slope is applied behind the division
    both = sx_epi_ref(x, ws[2], bs[2], flags=("res", "acc", "div"), dil=3, res=x, old_out=xs, div=3.0, islope=0.1, oslope=0.5)
    assert np.abs(both["out"] - np.where(mean >= 0, mean, mean * 0.5)).max() < 1e-12


def test_ends():
    assert sx_ends(3, 100).tolist() == [100, 100, 100]
    assert sx_ends(4, 100, [100, 30, 0, 1], 2, 3).tolist() == [100, 96, 0, 9]
    assert sx_ends(2, 100, [40, 0], -50, 1).tolist() == [-10, 0]      # (an end in front of the tensor: nothing lives)


@pytest.mark.parametrize("stride,K", [(1, 5), (4, 8)])
def test_ragged_ends_are_zero_the_input_crop_the_output(stride, K):
    B, Cin, Cout, T = 3, 16, 32, 50
    r, x, w, b = _data(9 + stride, B, Cin, Cout, T, K, stride=stride)
    lens, add, mul = [25, 7, 0], 2, 2
    ends = [50, 18, 0]
    assert sx_ends(B, T, lens, add, mul).tolist() == ends
    x[1, :, 18:] = 1e3
    x[2] = 1e3
    old = r.standard_normal((B, Cout, T * stride))
    got = sx_epi_ref(x, w, b, flags=("acc",), stride=stride, dil=1, old_out=old, lens=lens, rag_add=add, rag_mul=mul, planes=True,
                     oslope2=0.1, sentinel=-5.0)
    for bi in range(B):
        xz = x[bi:bi + 1].copy()
        xz[:, :, ends[bi]:] = 0.0                                              # zero the input ...
        full = sx_epi_ref(xz, w, b, flags=("acc",), stride=stride, dil=1, old_out=old[bi:bi + 1], planes=True, oslope2=0.1)
        n = ends[bi] * stride                                                   # ... crop the output
        assert np.array_equal(got["out"][bi, :, :n], full["out"][0, :, :n])
        assert np.array_equal(got["planes"][bi, :, :n], full["planes"][0, :, :n])
        assert np.array_equal(got["out"][bi, :, n:], old[bi, :, n:])
        assert (got["planes"][bi, :, n:] == -5.0).all()
        assert got["own"][bi, :, :n].all() and not got["own"][bi, :, n:].any()
        assert np.array_equal(got["own"][bi], got["own_pl"][bi])
    assert not got["own"][2].any()


def test_ownership_masks():
    r, x, w, b = _data(3, 2, 16, 32, 20, 3)
    a = sx_epi_ref(x, w, b, raw=True, planes=False)
    assert a["own"].all() and a["own_pl"] is None and a["planes"] is None
    a = sx_epi_ref(x, w, b, raw=False, planes=True)
    assert a["own_pl"].all() and a["own"] is None and a["out"] is None
    a = sx_epi_ref(x, w, b, flags=("acc", "no_raw_store"), old_out=np.ones((2, 32, 20)), planes=True, sentinel=3.0)
    assert not a["own"].any() and (a["out"] == 1.0).all() and a["own_pl"].all()
    a = sx_epi_ref(x, w, b, lens=[20, 5], rag_add=1, rag_mul=2, sentinel=3.0)
    assert a["own"][0].all() and a["own"][1, :, :12].all() and not a["own"][1, :, 12:].any()
    assert (a["out"][1, :, 12:] == 3.0).all()
    with pytest.raises(AssertionError):
        sx_epi_ref(x, w, b, flags=("mask",))
