"""tests/g2p_kernels_ref.py (the float64 references behind tests/test_gpu_g2p_kernels.py) pinned on the CPU: the attention
reference against T5Oracle.attention and transformers' T5Attention, and every claim the GPU file makes about its input families
checked on the reference's own float32 evaluation - those are conditions on the inputs, so the reference alone must meet them.
The float32 - float64 gaps that set the GPU file's bounds are measured here, over the same arrays."""
import numpy as np
import pytest

import g2p_kernels_ref as gr


def ulps(got, want):
    """|got - want| in units of the float32 spacing at want"""
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the attention reference
def _oracle(heads, dk, bias_enc, bias_dec):
    """T5Oracle with identity projections: its attention() is then attention of (xq, xkv, xkv) itself"""
    from t5_oracle import T5Oracle
    o = T5Oracle.__new__(T5Oracle)
    eye = np.eye(heads * dk)
    o.w = {"a.q": eye, "a.k": eye, "a.v": eye, "a.o": eye,
           "encoder.0.0.SelfAttention.relative_attention_bias": bias_enc.astype(np.float64),
           "decoder.0.0.SelfAttention.relative_attention_bias": bias_dec.astype(np.float64)}
    o.dtype, o.heads, o.d_kv, o.inner, o.num_buckets, o.max_distance = np.float64, heads, dk, heads * dk, gr.NUM_BUCKETS, 128
    return o


def _plain_case(rng, heads, dk, Tq, Tk, lut, causal, q_off, bias):
    """[C][T] activations, one sequence"""
    C = heads * dk
    q, k, v = rng.standard_normal((C, Tq)), rng.standard_normal((C, Tk)), rng.standard_normal((C, Tk))
    return dict(q=q.astype(np.float32).reshape(-1), out=np.zeros(C * Tq, np.float32), q_cs=Tq, q_ts=1, k=k.astype(np.float32).reshape(-1),
                v=v.astype(np.float32).reshape(-1), kp=Tk, kv_bs=0, bias=bias, lut=lut, heads=heads, dk=dk, cols=Tq, seg=Tq, lens=None,
                Tk=Tk, q_off=q_off, causal=causal)


@pytest.mark.parametrize("dk", [64, 20])
def test_attention_reference_is_the_oracles_attention(dk):
    """An encoder case, a causal prefill and a one-query step with q_off = t: the same numbers as T5Oracle.attention with
    T5Oracle.position_bias (float64) to 1e-12."""
    heads = 2
    rng = np.random.default_rng(dk)
    be, bd = rng.uniform(-2, 2, (gr.NUM_BUCKETS, heads)).astype(np.float32), rng.uniform(-2, 2, (gr.NUM_BUCKETS, heads)).astype(np.float32)
    o = _oracle(heads, dk, be, bd)
    for what, Tq, Tk, stack, causal, q_off in (("encoder", 70, 70, "encoder", False, 0), ("prefill", 45, 45, "decoder", True, 0),
                                              ("step", 1, 301, "decoder", True, 300), ("cross", 9, 33, None, False, 0)):
        c = _plain_case(rng, heads, dk, Tq, Tk, None if stack is None else gr.lut_of(stack[:3]), causal, q_off,
                        None if stack is None else (be if stack == "encoder" else bd))
        got = gr.attention_ref(c).reshape(heads * dk, Tq)
        bias = np.zeros((heads, Tq, Tk)) if stack is None else o.position_bias(stack, Tq, Tk, q_off)
        if causal:
            bias = bias + np.where(np.arange(Tk)[None, :] > np.arange(Tq)[:, None] + q_off, -np.inf, 0.0)[None]
        xq, xkv = c["q"].reshape(-1, Tq).T.astype(np.float64), c["k"].reshape(-1, Tk).T.astype(np.float64)
        want = _oracle_attention(o, xq, xkv, c["v"].reshape(-1, Tk).T.astype(np.float64), bias)
        err = float(np.abs(got - want.T).max())
        print(f"dk {dk} {what}: |reference - T5Oracle.attention| {err:.2e}")
        assert err <= 1e-12, (what, err)


def _oracle_attention(o, xq, xk, xv, bias):
    """T5Oracle.attention projects ONE memory into keys and values; here they are separate arrays, so the memory is [k | v]
    and the k / v projections select its halves"""
    n = o.inner
    o.w["a.k"] = np.concatenate((np.eye(n), np.zeros((n, n))))
    o.w["a.v"] = np.concatenate((np.zeros((n, n)), np.eye(n)))
    o.w["a.q"] = np.concatenate((np.eye(n), np.zeros((n, n))))
    return o.attention("a", np.concatenate((xq, np.zeros_like(xq)), 1), np.concatenate((xk, xv), 1), bias)


def test_attention_reference_is_transformers_t5_attention():
    transformers = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    from transformers.models.t5.modeling_t5 import T5Attention
    heads, dk = 2, 16
    n = heads * dk
    rng = np.random.default_rng(3)
    for decoder, Tq in ((False, 40), (True, 33)):
        cfg = transformers.T5Config(d_model=2 * n, d_kv=dk, num_heads=heads, relative_attention_num_buckets=gr.NUM_BUCKETS,
                                    relative_attention_max_distance=128, dropout_rate=0.0, is_decoder=decoder)
        att = T5Attention(cfg, has_relative_attention_bias=True, layer_idx=0).double().eval()
        bias = rng.uniform(-2, 2, (gr.NUM_BUCKETS, heads)).astype(np.float32)
        c = _plain_case(rng, heads, dk, Tq, Tq, gr.lut_of("dec" if decoder else "enc"), decoder, 0, bias)
        half = lambda first: torch.from_numpy(np.concatenate((np.eye(n), np.zeros((n, n))) if first else (np.zeros((n, n)), np.eye(n)), 1))
        with torch.no_grad():
            att.q.weight.copy_(half(True))
            att.k.weight.copy_(half(True))
            att.v.weight.copy_(half(False))
            att.o.weight.copy_(torch.from_numpy(np.concatenate((np.eye(n), np.zeros((n, n))), 0)))
            att.relative_attention_bias.weight.copy_(torch.from_numpy(bias.astype(np.float64)))
            c["k"] = c["q"].copy()   # (self attention projects one input: queries and keys are the same array here)
            q, v = (c[name].reshape(n, Tq).T.astype(np.float64) for name in ("q", "v"))
            x = torch.from_numpy(np.concatenate((q, v), 1))[None]
            mask = None
            if decoder:
                mask = torch.triu(torch.full((Tq, Tq), -np.inf, dtype=torch.float64), 1)[None, None]
            y = att(x, mask=mask)[0][0].numpy()
        got = gr.attention_ref(c).reshape(n, Tq).T
        err = float(np.abs(got - y[:, :n]).max())
        print(f"decoder {decoder}: |reference - T5Attention| {err:.2e}")
        assert err <= 1e-12 and not y[:, n:].any()


# ------------------------------------------------------------------------------------------------ float32 gaps (the GPU bounds)
def attention_gaps(dk):
    """max over every random launch of the GPU file at this head width of |float32 evaluation - float64 reference| / max|v|"""
    worst = 0.0
    for form in gr.FORMS:
        for Tk in gr.DK_TKS[dk]:
            for c in gr.random_cases(form, Tk, dk):
                own = gr.owned(c)
                gap = float(np.abs(gr.attention_ref(c, np.float32)[own].astype(np.float64) - gr.attention_ref(c)[own]).max())
                worst = max(worst, gap / float(np.abs(c["v"]).max()))
    return worst


@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
def test_recorded_attention_gap_is_the_measured_one(dk):
    """ATT_F32_GAP of the GPU file is what NumPy float32 is away from float64 on that file's own random inputs.  The constant
    is the measurement of one host rounded up; another host's BLAS and vectorised exp round differently in the last bits, so
    the measurement here has to meet it within a factor 1.5 either way: a recorded gap that is padded, or one that the inputs
    have outgrown, fails."""
    from test_gpu_g2p_kernels import ATT_F32_GAP
    gap = attention_gaps(dk)
    print(f"dk {dk}: measured float32 gap {gap:.3e} of max|v|, recorded {ATT_F32_GAP[dk]:.3e}")
    assert gap <= 1.5 * ATT_F32_GAP[dk] and ATT_F32_GAP[dk] <= 1.5 * gap


def test_recorded_rmsnorm_gap_is_the_measured_one():
    from test_gpu_g2p_kernels import RMS_F32_GAP
    worst = 0.0
    for C in gr.RMS_C:
        for T in gr.RMS_T:
            x, g, y, eps = gr.rms_case(C, T)
            ref = gr.rmsnorm_ref(x, g, y, T, eps)
            f32 = gr.rmsnorm_ref(x, g, y, T, eps, np.float32)
            assert np.array_equal(f32[:, T:], y[:, T:]) and np.array_equal(ref[:, T:], y[:, T:])
            worst = max(worst, float(np.abs(f32[:, :T] - ref[:, :T]).max() / np.abs(ref[:, :T]).max()))
    print(f"rmsnorm: measured float32 gap {worst:.3e} of max|y|, recorded {RMS_F32_GAP:.3e}")
    assert worst <= 1.5 * RMS_F32_GAP and RMS_F32_GAP <= 1.5 * worst


# ------------------------------------------------------------------------------------------------ the families' claims
@pytest.mark.parametrize("dk", [64, 40])
def test_poison_lies_outside_what_the_reference_reads(dk):
    for form in gr.FORMS:
        for Tk in (1, 2, 65, 257):
            for c in gr.random_cases(form, Tk, dk):
                p = gr.poisoned(c)
                assert np.isnan(p["k"]).any() and np.isnan(p["v"]).any()
                a, b = gr.attention_ref(c), gr.attention_ref(p)
                assert np.array_equal(a, b) and np.isfinite(b).all(), (form, Tk)
                own = gr.owned(c)
                rest = np.ones(a.size, bool)
                rest[own.reshape(-1)] = False
                assert np.unique(own).size == own.size and np.all(a[rest] == gr.SENTINEL) and not np.any(a[own] == gr.SENTINEL)


@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
def test_selected_key_is_returned_bit_for_bit_in_float32(dk):
    n = 0
    for form in gr.FORMS:
        for Tk in gr.DK_TKS[dk]:
            for c, want in gr.selected_key_cases(form, Tk, dk):
                got = gr.attention_ref(c, np.float32)[gr.owned(c)]
                assert got.dtype == np.float32 and np.array_equal(got, want) and np.abs(want).min() >= 1, (form, Tk)
                n += 1
    assert n > 3 * len(gr.FORMS) * len(gr.DK_TKS[dk]) / 2


@pytest.mark.parametrize("dk", sorted(gr.DK_TKS))
def test_uniform_and_bucket_means_hold_to_two_ulp_in_float32(dk):
    nb = 0
    for form in gr.FORMS:
        for Tk in gr.DK_TKS[dk]:
            for c, sums, cnt in gr.uniform_cases(form, Tk, dk):
                got = gr.attention_ref(c, np.float32)[gr.owned(c)]
                lim = gr.limits(c).reshape(-1)
                assert np.array_equal(cnt, np.repeat(lim[None], c["heads"], 0))
                u = ulps(got, (sums / np.repeat(cnt, dk, 0)).astype(np.float32))
                assert u.max() <= 2, (form, Tk, u.max())
                assert ulps(got[::dk], np.ones_like(got[::dk])).max() <= 2
                if dk > 1:
                    assert ulps(got[1::dk], ((lim - 1) / 2).astype(np.float32)[None]).max() <= 2
            if form in ("enc", "pre_self", "step_self_narrow", "step_self_wide"):
                for c, sums, cnt in gr.bucket_cases(form, Tk, dk):
                    got = gr.attention_ref(c, np.float32)[gr.owned(c)]
                    u = ulps(got, (sums / np.repeat(cnt, dk, 0)).astype(np.float32))
                    assert u.max() <= 2, (form, Tk, u.max())
                    lim = gr.limits(c).reshape(-1)
                    assert (cnt < lim[None]).any() or Tk <= 2     # (a real selection, not the mean of everything)
                    nb += 1
    assert nb >= len(gr.DK_TKS[dk]) - 1


def test_widened_case_has_the_same_float64_answer():
    for form in gr.FORMS:
        for Tk in (1, 65, 257):
            for c in gr.random_cases(form, Tk, 64):
                w, lo = gr.widened(c)
                a, b = gr.attention_ref(c)[gr.owned(c)], gr.attention_ref(w)[gr.owned(w)[lo]]
                assert float(np.abs(a - b).max()) <= 1e-12, (form, Tk)


def test_rmsnorm_exact_family_in_float32():
    for C in gr.RMS_C:
        for T in gr.RMS_T:
            x, g, y, eps = gr.rms_case(C, T, exact=True)
            f32 = gr.rmsnorm_ref(x, g, y, T, eps, np.float32)
            want = x[:, :T] * g[:, None]
            if C & (C - 1) == 0:
                assert np.array_equal(f32[:, :T], want), C
            else:
                assert ulps(f32[:, :T], want).max() <= 2, C
            assert np.array_equal(gr.rmsnorm_ref(x, g, y, T, eps)[:, :T], want)


def test_argmax_reference_and_its_rows():
    seen = set()
    for V in gr.ARGMAX_V:
        for NB in gr.ARGMAX_NB:
            rows, kinds = gr.argmax_rows(V, NB)
            for row, kind in zip(rows, kinds):
                a = gr.argmax_ref(row)
                assert 0 <= a < V
                if not np.isnan(row).any():
                    assert a == int(np.argmax(row))             # first maximum, as np.argmax
                else:
                    assert np.isnan(row).all() and a == 0 or (not np.isnan(row[a]) and row[a] == np.nanmax(row) and
                                                              not np.any(row[:a] == row[a]))
                if kind in (2, 3, 4):
                    assert a == 0
                if kind == 5 and V > 3:
                    assert a == 1 and np.isnan(row[0])
                if kind == 1 and V > 300:
                    assert a in (0, 5, 255)
                seen.add(kind)
    assert seen == set(range(8))
    assert gr.argmax_ref(np.array([np.nan, -np.inf, -np.inf], np.float32)) == 1
