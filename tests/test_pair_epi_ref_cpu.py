"""tests/pair_epi_ref.py, the float64 statement of one fused ResBlock-step launch, against independent statements of the same
operation (no GPU): two composed launches of tests/sx_epi_ref.py, torch's conv1d wired as the modules wire it, its ownership
masks by hand - and the size of what fp32 accumulation may move in the single-plane arithmetic, for the seeds the GPU test uses."""
import numpy as np
import pytest

from pair_epi_ref import pair_epi_ref
from sx_epi_ref import sx_epi_ref

S = 0.1


def _data(seed, B, C, T, K):
    r = np.random.default_rng(seed)
    n = lambda *s: r.standard_normal(s)
    return n(B, C, T), n(C, C, K) / np.sqrt(C * K), n(C), n(C, C, K) / np.sqrt(C * K) * 2, n(C), n(B, C, T)


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("lens,add,mul", [(None, 0, 1), ([0, 23, 50], 0, 1), ([3, 1, 0], 2, 8)])
def test_reference_is_two_composed_single_conv_launches(chain, lens, add, mul):
    B, C, T, K, d1, d2 = 3, 8, 50, 5, 2, 3
    x, w1, b1, w2, b2, old = _data(1, B, C, T, K)
    rag = dict(lens=lens, rag_add=add, rag_mul=mul)
    for flags, div in ((("raw",), 1.0), (("acc", "raw"), 1.0), (("acc", "div", "raw", "planes"), 3.0), (("acc", "div", "planes"), 2.0)):
        got = pair_epi_ref(x, w1, b1, w2, b2, flags=flags, dil1=d1, dil2=d2, chain=chain, slope=S, div=div, old_out=old, sentinel=-7.5,
                           **rag)
        # step 1 with lens; step 2 with lens, res, old_out and div (its input is taken as zero behind the ends, as mid is)
        s1 = sx_epi_ref(x, w1, b1, flags=("res",) if chain else (), res=x, dil=d1, islope=S, **rag)["value"]
        f2 = ("res",) + tuple(f for f in flags if f in ("acc", "div")) + (() if "raw" in flags else ("no_raw_store",))
        s2 = sx_epi_ref(s1, w2, b2, flags=f2, res=s1 if chain else x, old_out=old, div=div, dil=d2, islope=S, oslope2=S,
                        planes="planes" in flags, sentinel=-7.5, **rag)
        assert np.array_equal(got["own"], s2["own"])
        for o in ("out", "planes"):
            if got[o] is None:
                assert s2[o] is None
                continue
            np.testing.assert_allclose(got[o], s2[o], rtol=1e-12, atol=0)
        if got["planes"] is not None:
            assert np.array_equal(got["own_pl"], s2["own_pl"])


@pytest.mark.parametrize("chain", [False, True])
def test_reference_is_the_modules_wiring_of_torch_conv1d(chain):
    import torch
    import torch.nn.functional as F
    B, C, T, K, d1, d2 = 2, 8, 61, 7, 3, 2
    x, w1, b1, w2, b2, _ = _data(2, B, C, T, K)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    c = lambda v, w, b, d: F.conv1d(v, t(w), t(b), dilation=d, padding=d * (K - 1) // 2)
    xt = t(x)
    if chain:   # modules.py ResBlock2, two steps: xt = c(leaky_relu(x)); x = xt + x
        for w, b, d in ((w1, b1, d1), (w2, b2, d2)):
            xt = c(F.leaky_relu(xt, S), w, b, d) + xt
        want = xt
    else:       # modules.py ResBlock1, one step: xt = c1(leaky_relu(x)); xt = c2(leaky_relu(xt)); x = xt + x
        want = c(F.leaky_relu(c(F.leaky_relu(xt, S), w1, b1, d1), S), w2, b2, d2) + xt
    got = pair_epi_ref(x, w1, b1, w2, b2, dil1=d1, dil2=d2, chain=chain, slope=S)
    np.testing.assert_allclose(got["out"], want.numpy(), rtol=1e-12, atol=1e-13)
    assert got["own"].all() and got["planes"] is None


def test_ownership_masks():
    B, C, K, BNo = 3, 8, 3, 20
    T = 2 * BNo + 1
    x, w1, b1, w2, b2, old = _data(3, B, C, T, K)
    # a length of 0, an end one column behind a seam, an end at T
    got = pair_epi_ref(x, w1, b1, w2, b2, flags=("raw", "planes"), lens=[0, BNo + 1, T], sentinel=5.0)
    for own in (got["own"], got["own_pl"]):
        assert not own[0].any() and own[1, :, :BNo + 1].all() and not own[1, :, BNo + 1:].any() and own[2].all()
    assert (got["out"][~got["own"]] == 5.0).all() and (got["planes"][~got["own_pl"]] == 5.0).all()
    assert not got["mid"][0].any() and not got["mid"][1, :, BNo + 1:].any()
    # frames of 8 columns with a margin of 2: (len + 2) * 8, capped at T; 0 stays 0
    got = pair_epi_ref(x, w1, b1, w2, b2, flags=("raw",), lens=[0, 1, 4], rag_add=2, rag_mul=8)
    assert [int(got["own"][b, 0].sum()) for b in range(B)] == [0, 24, T]
    # without "raw" the raw tensor owns nothing and keeps the old contents
    got = pair_epi_ref(x, w1, b1, w2, b2, flags=("acc", "div", "planes"), old_out=old, div=2.0)
    assert not got["own"].any() and np.array_equal(got["out"], old) and got["own_pl"].all()
    # what lies behind an end does not matter
    y = x.copy()
    y[1, :, BNo + 1:] = 1e4
    a, b = (pair_epi_ref(v, w1, b1, w2, b2, lens=[0, BNo + 1, T])["out"] for v in (x, y))
    assert np.array_equal(a, b)


def test_what_no_call_site_forms_is_rejected():
    x, w1, b1, w2, b2, old = _data(4, 1, 8, 10, 3)
    with pytest.raises(ValueError, match="div without acc"):
        pair_epi_ref(x, w1, b1, w2, b2, flags=("div", "raw"), div=2.0)
    with pytest.raises(ValueError, match="acc without old_out"):
        pair_epi_ref(x, w1, b1, w2, b2, flags=("acc", "raw"))
    with pytest.raises(ValueError, match="even K"):
        pair_epi_ref(x, w1[:, :, :2], b1, w2[:, :, :2], b2)


def test_fp32_accumulation_stays_inside_the_single_plane_cap():
    """tests/test_gpu_pair16_epilogue.py allows at most 0.1 % of a case's owned elements to differ from the `quantized`
    reference by more than 1e-4 (an intermediate on a rounding boundary of its fp16 plane that falls the other way).  The same
    roundings evaluated with float32 products and sums - the size of what the kernel's accumulation may move - stay inside that
    cap and inside the rms figure, for every f16 case and seed of the GPU test's edge, form and ragged groups."""
    import test_gpu_pair16_epilogue as g
    worst = (0.0, 0.0, "")
    n = 0

    def hold(name, x, wb, **kw):
        nonlocal worst, n
        a = pair_epi_ref(x, *wb, quantized=True, **kw)
        b = pair_epi_ref(x, *wb, quantized=True, acc32=True, **kw)
        sel = a["own"]
        if not sel.any():
            return
        err = np.abs(a["value"] - b["value"])[sel]
        share, rms = float((err > 1e-4).mean()), float(np.sqrt((err ** 2).mean()))
        worst = max(worst, (share, rms, name))
        n += 1
        assert share <= 1e-3 and rms < 1e-4, (name, share, rms, float(err.max()))

    for case in g.edge_cases():
        name, C, p, K, d1, d2, chain, T, _ = case
        if p == "f16":
            x, wb = g.edge_data(case)
            hold(name, x, wb, dil1=d1, dil2=d2, chain=chain, slope=g.SLOPE)
    for C, p, chain in g.INST:
        if p != "f16":
            continue
        K, d1, d2 = 3, 1, (2 if chain else 1)
        T = g.plan(C, p, K, d1, d2)[1] + 1
        hold(f"forms C{C} chain {chain}", g.normal(40 + C, 2, C, T), g.weights(41 + C + chain, C, K, s2=g.w2_scale(p)), dil1=d1, dil2=d2, chain=chain, slope=g.SLOPE)
        K, d1, d2, BNo, T, x, wb, sets = g.ragged_data(C, p, chain)
        for lens, add, mul, _ in sets:
            hold(f"ragged C{C} chain {chain} {lens}", x, wb, dil1=d1, dil2=d2, chain=chain, slope=g.SLOPE, lens=lens, rag_add=add, rag_mul=mul)
    print(f"{n} cases; worst share of owned elements off by > 1e-4: {100 * worst[0]:.4f} % (rms {worst[1]:.2e}) in {worst[2]}")
    assert n >= 56
