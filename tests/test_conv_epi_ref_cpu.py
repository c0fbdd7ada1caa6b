"""The float64 reference of the f32 conv engine's launches (tests/conv_epi_ref.py) checked on the CPU: its conv against
torch's, its folded update rules against the module formulas written out literally (WN layers, mean-only coupling, the
generator's multi-receptive-field mean), and its ownership masks."""
import numpy as np
import pytest

from conv_epi_ref import conv1d, conv_epi_ref, conv_transpose1d, lrelu

SENT = -1234.5678


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("Cin,Cout,T,K,dil,pad_l", [(5, 7, 33, 3, 2, 2), (4, 3, 20, 1, 1, 0), (6, 2, 17, 5, 3, 4), (3, 4, 9, 4, 1, 3)])
def test_conv_part_equals_torch_conv1d(Cin, Cout, T, K, dil, pad_l):
    import torch
    import torch.nn.functional as F
    r = _rng(T)
    x, w, b = r.standard_normal((2, Cin, T)), r.standard_normal((Cout, Cin, K)), r.standard_normal(Cout)
    pad_r = dil * (K - 1) - pad_l
    want = F.conv1d(F.pad(torch.from_numpy(x), (pad_l, pad_r)), torch.from_numpy(w), torch.from_numpy(b), dilation=dil).numpy()
    np.testing.assert_allclose(conv1d(x, w, dil, pad_l) + b[None, :, None], want, atol=1e-12, rtol=0)
    got = conv_epi_ref(x, w, b, dil=dil, pad_l=pad_l)
    np.testing.assert_allclose(got["out"], want, atol=1e-12, rtol=0)
    assert got["own"].all() and got["out2"] is None and got["planes"] is None


@pytest.mark.parametrize("Cin,Cout,T,K,u", [(5, 3, 11, 4, 2), (4, 2, 7, 16, 8), (3, 3, 5, 6, 2)])
def test_conv_part_equals_torch_conv_transpose1d(Cin, Cout, T, K, u):
    import torch
    import torch.nn.functional as F
    r = _rng(K)
    x, w, b = r.standard_normal((2, Cin, T)), r.standard_normal((Cin, Cout, K)), r.standard_normal(Cout)
    want = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=u, padding=(K - u) // 2).numpy()
    np.testing.assert_allclose(conv_transpose1d(x, w, u) + b[None, :, None], want, atol=1e-12, rtol=0)
    got = conv_epi_ref(x, w, b, stride=u, out2=True, oslope2=0.1)
    np.testing.assert_allclose(got["out"], want, atol=1e-12, rtol=0)
    np.testing.assert_allclose(got["out2"], np.where(want >= 0, want, 0.1 * want), atol=1e-12, rtol=0)


def test_folded_wn_layers_equal_the_module_on_ragged_lengths():
    # the module (first, middle, last layer): x_in = in_i(x) + g_i; acts = tanh(x_in[:H]) * sigmoid(x_in[H:]);
    # rs = res_skip_i(acts); not last: x = (x + rs[:H]) * mask, output += rs[H:]; last: output += rs; result output * mask
    r = _rng(1)
    B, H, T, n = 3, 8, 13, 3
    lens = np.array([13, 4, 0])
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)[:, None, :]
    x0 = r.standard_normal((B, H, T)) * mask   # (h = pre(x0) * mask enters the stack masked)
    in_w = [r.standard_normal((2 * H, H, 3)) / 5 for _ in range(n)]
    rs_w = [r.standard_normal(((2 * H if i < n - 1 else H), H, 1)) / 3 for i in range(n)]
    rs_b = [r.standard_normal(w.shape[0]) for w in rs_w]
    g = r.standard_normal((B, n * 2 * H))

    def acts_of(x, i):
        x_in = conv1d(x, in_w[i], 1, 1) + g[:, i * 2 * H:(i + 1) * 2 * H, None]
        return np.tanh(x_in[:, :H]) * (1.0 / (1.0 + np.exp(-x_in[:, H:])))

    x, output = x0.copy(), np.zeros_like(x0)
    for i in range(n):
        rs = conv1d(acts_of(x, i), rs_w[i], 1, 0) + rs_b[i][None, :, None]
        if i < n - 1:
            x = (x + rs[:, :H]) * mask
            output = output + rs[:, H:]
        else:
            output = output + rs
    want_skip, want_x = output * mask, x

    # the folded form, launch by launch: the skip tensor starts as garbage and the first layer stores it
    fx, fskip = x0.copy(), r.standard_normal((B, H, T)) * 1e6
    for i in range(n):
        last = i == n - 1
        flags = ("wn", "mask") + (("wn_first",) if i == 0 else ())
        got = conv_epi_ref(acts_of(fx, i), rs_w[i], rs_b[i], flags=flags, lens=lens, old_out=fx, old_out2=fskip,
                           wn_split=0 if last else H, out_rows=H, pl_rows=0, sentinel=SENT)
        if last:
            assert np.array_equal(got["out"], fx) and not got["own"].any()     # x keeps every bit
        assert got["own2"].all()
        fx, fskip = got["out"], got["out2"]
    np.testing.assert_allclose(fskip, want_skip, atol=1e-12, rtol=0)
    np.testing.assert_allclose(fx, want_x, atol=1e-12, rtol=0)


def test_coupling_rule_equals_the_module_and_leaves_the_other_half_alone():
    # reverse, mean only: stats = post(h) * mask; x1 = (x1 - stats) * mask; x = cat(x0, x1)
    r = _rng(2)
    B, Hh, half, T = 2, 6, 4, 11
    lens = np.array([11, 3])
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)[:, None, :]
    h, z = r.standard_normal((B, Hh, T)), r.standard_normal((B, 2 * half, T))
    w, b = r.standard_normal((half, Hh, 1)), r.standard_normal(half)
    stats = (conv1d(h, w, 1, 0) + b[None, :, None]) * mask
    want = np.concatenate([z[:, :half], (z[:, half:] - stats) * mask], 1)
    got = conv_epi_ref(h, w, b, flags=("coupling",), lens=lens, old_out=z, out_rows=2 * half, out_row0=half, sentinel=SENT)
    np.testing.assert_allclose(got["out"], want, atol=1e-12, rtol=0)
    assert got["own"][:, half:].all() and not got["own"][:, :half].any()
    assert np.array_equal(got["out"][:, :half], z[:, :half])


def test_mrf_forms_sum_to_the_mean_of_the_resblocks():
    # xs = (rb_0 + rb_1 + rb_2) / 3 with rb_j = c_j(a) + x_j (the last step of each ResBlock), then leaky_relu(0.01)
    r = _rng(3)
    B, C, T = 2, 5, 19
    a = [r.standard_normal((B, C, T)) for _ in range(3)]
    xr = [r.standard_normal((B, C, T)) for _ in range(3)]
    w = [r.standard_normal((C, C, 3)) / 4 for _ in range(3)]
    b = [r.standard_normal(C) for _ in range(3)]
    rb = [conv1d(a[j], w[j], 1, 1) + b[j][None, :, None] + xr[j] for j in range(3)]
    want = lrelu((rb[0] + rb[1] + rb[2]) / 3, 0.01)
    xs = None
    for j, flags in enumerate([("res",), ("res", "acc"), ("res", "acc", "div")]):
        got = conv_epi_ref(a[j], w[j], b[j], flags=flags, res=xr[j], old_out=xs, div=3.0, oslope=0.01 if j == 2 else 1.0, sentinel=SENT)
        xs = got["out"]
    np.testing.assert_allclose(xs, want, atol=1e-12, rtol=0)


def test_mask_comes_before_the_residual_and_pro_mask_hides_what_lies_behind_the_length():
    r = _rng(4)
    B, C, T = 2, 4, 12
    lens = np.array([12, 5])
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float64)[:, None, :]
    x, res = r.standard_normal((B, C, T)), r.standard_normal((B, C, T))
    w, b = r.standard_normal((C, C, 3)), r.standard_normal(C)
    y = conv1d(x, w, 1, 1) + b[None, :, None]
    got = conv_epi_ref(x, w, b, flags=("mask", "res"), lens=lens, res=res)
    np.testing.assert_allclose(got["out"], y * mask + res, atol=1e-12, rtol=0)
    assert np.abs(res[1, :, 5:]).min() > 0 and np.array_equal(got["out"][1, :, 5:], res[1, :, 5:])
    got = conv_epi_ref(x, w, b, flags=("pro_mask", "relu"), lens=lens)
    np.testing.assert_allclose(got["out"], np.maximum(conv1d(x * mask, w, 1, 1) + b[None, :, None], 0), atol=1e-12, rtol=0)
    # the tap that reaches across len[b] sees zero: column len - 1 differs from the unmasked conv, column len - 2 does not
    assert not np.allclose(conv1d(x * mask, w, 1, 1)[1, :, 4], conv1d(x, w, 1, 1)[1, :, 4])
    np.testing.assert_allclose(conv1d(x * mask, w, 1, 1)[1, :, 3], conv1d(x, w, 1, 1)[1, :, 3], atol=1e-12)


def test_ownership_covers_the_pitch_columns_and_nothing_outside_the_window():
    r = _rng(5)
    B, Cin, Cout, T = 2, 3, 4, 10
    x, w = r.standard_normal((B, Cin, T)), r.standard_normal((Cout, Cin, 1))
    got = conv_epi_ref(x, w, None, out2=True, oslope2=0.1, out_cstride=12, out_rows=7, out_row0=2, pl_rows=0, sentinel=SENT)
    for name, own in (("out", got["own"]), ("out2", got["own2"])):
        assert own[:, 2:6].all() and not own[:, :2].any() and not own[:, 6:].any()
        assert np.array_equal(got[name][:, 2:6, T:], np.zeros((B, 4, 2)))
        assert np.array_equal(got[name][~own], np.full((~own).sum(), np.float64(np.float32(SENT))))
    # planes are the stored rows
    got = conv_epi_ref(x, np.concatenate([w] * 8), None, oslope=0.1, pl_rows=32)
    assert np.array_equal(got["planes"], got["out"][:, :32])
