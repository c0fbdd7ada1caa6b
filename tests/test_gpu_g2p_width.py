"""The ByT5 G2P engine (phoonnx_amd/csrc/g2p.hip) at the widths of the models it exists for - d_model 1472, d_ff 3584, 6 heads x 64
(g2p-mbyt5-12l, the ByT5-small shape) - where the fixtures of test_gpu_g2p.py (d_model 96 / 128) never enter whole code paths:
the second pass of the branch-free linear kernel's k loop (in > 2048), its clamped rows / steps / columns, the several-chunk
rows of the matrix-vector step kernel, and the wide decoder step (more than four sequences side by side) by value.

Three layers: the linear and step kernels through the engine's own dispatch (g2p_test_linear / g2p_test_step) against exact
integer products and float64; then the whole engine on seeded full-width models (phoonnx_amd.synth.write_t5, itself pinned to
transformers in test_g2p_oracle.py) against the float64 oracle - at the end also across the boundaries of the attention bodies
(more than 64 and 256 keys in one-query attention, a padded batch with a 700-byte input, 1023 keys), which
test_gpu_g2p_kernels.py tests launch by launch."""
import os

import numpy as np
import pytest

from bench import voice_cache

pytestmark = pytest.mark.gpu

CACHE = voice_cache()

LOGIT_TOL = 2e-3   # test_gpu_g2p.py's bound, for logits O(30)

# max |T5Oracle(float32) - T5Oracle(float64)| over every input of this file, per model (CPU, reference against reference;
# measured values in DESIGN.md): what ONE float32 evaluation of the graph is away from the exact one.  The engine's bound
# against the float64 oracle is 4 x that (its summation order, split reductions and online softmax differ from NumPy's, and
# the float32 oracle is itself one sample of fp32 rounding), and never looser than LOGIT_TOL x max|logits| / 30.
F32_GAP = {
    "w1472_2x2": 3.30e-5,    # measured 3.29e-5 (logits up to 37): bound 1.32e-4; engine: run 2.2e-5, narrow 1.5e-5, wide 2.3e-5
    "w1472_12x4": 3.70e-5,   # measured 3.69e-5 (logits up to 32): bound 1.48e-4; engine: run 2.2e-5, narrow 2.9e-5, wide 2.8e-5
    # (the two small models also run the long inputs below - LONG_LENS, LONG_RUN_SHAPES - where the gap is larger: 7.27e-6 and
    # 2.55e-5 over the short ones)
    "relu_tied": 8.2e-6,     # measured 8.18e-6 (logits up to 13): bound 3.3e-5; engine: run 2.4e-6, steps 2.1e-6, long steps 2.7e-6
    "gelu_erf": 3.55e-5,     # measured 3.54e-5 (logits up to 38): bound 1.42e-4; engine: run 1.0e-5, steps 1.3e-5, long steps 1.2e-5
}
MODELS = {
    "w1472_2x2": dict(d_model=1472, d_ff=3584, num_heads=6, d_kv=64, num_layers=2, num_decoder_layers=2),
    "w1472_12x4": dict(d_model=1472, d_ff=3584, num_heads=6, d_kv=64, num_layers=12, num_decoder_layers=4),
    "relu_tied": dict(d_model=256, d_ff=512, num_heads=4, d_kv=64, num_layers=2, num_decoder_layers=2, feed_forward_proj="relu",
                      tied=True),
    "gelu_erf": dict(d_model=256, d_ff=512, num_heads=4, d_kv=64, num_layers=2, num_decoder_layers=2, feed_forward_proj="gelu"),
}


def model_path(name):
    from phoonnx_amd.synth import write_t5
    path = os.path.join(CACHE, f"t5_{name}.onnx")
    if not os.path.exists(path):
        os.makedirs(CACHE, exist_ok=True)
        write_t5(path, seed=77, **MODELS[name])
    return path


def logits_bound(name, ref):
    return min(4 * F32_GAP[name], LOGIT_TOL * float(np.abs(ref).max()) / 30)


# ------------------------------------------------------------------------------------------------ inputs (shared with the
# CPU measurement of F32_GAP: the same arrays)
RUN_SHAPES = ((1, 1), (20, 12), (33, 17), (80, 40), (300, 9))
POOL_LENS = [3 + (37 * i) % 58 for i in range(64)]     # 64 different-looking input lengths in 3 .. 60
NARROW_STEPS, WIDE_STEPS = 40, 24


def run_cases(shapes=RUN_SHAPES, seed=101):
    rng = np.random.default_rng(seed)
    out = []
    for S, T in shapes:
        ids = rng.integers(3, 259, S).astype(np.int64)
        dec = np.concatenate(([0], rng.integers(3, 259, T - 1))).astype(np.int64)
        out.append((ids, dec))
    return out


def pool(seed=102):
    """64 inputs of different lengths and their given decoder inputs [64, NARROW_STEPS] (column 0 = the start token)"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(3, 259, n).astype(np.int64) for n in POOL_LENS]
    decs = np.concatenate((np.zeros((64, 1), np.int64), rng.integers(3, 259, (64, NARROW_STEPS - 1))), axis=1)
    return seqs, decs


# Across the boundaries of the attention bodies (the small models only: a case costs little on them).  Input lengths on both
# sides of 64 and 256 keys, one of 700 bytes beside one of 1 (the batched encoder pads to the longest; cross attention runs under
# `lens`), and enough forced steps that self attention crosses 64 and 256 keys too.
LONG_LENS = (300, 257, 256, 65, 64, 3, 1, 129, 700)
LONG_STEPS = 270
LONG_RUN_SHAPES = ((1023, 5), (40, 300))


def long_pool(seed=103):
    """the LONG_LENS inputs and their given decoder inputs [9, LONG_STEPS] (column 0 = the start token)"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(3, 259, n).astype(np.int64) for n in LONG_LENS]
    decs = np.concatenate((np.zeros((len(seqs), 1), np.int64), rng.integers(3, 259, (len(seqs), LONG_STEPS - 1))), axis=1)
    return seqs, decs


# ------------------------------------------------------------------------------------------------ linear kernels
def _ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


def _exact(W, x):
    """The integer product, exactly: operands are integers of magnitude <= 8 and in <= 3584, so every partial sum is an
    integer below 2^24 - float64 BLAS computes the int64 product without rounding (checked), and so must fp32 in any order."""
    y = W.astype(np.float64) @ x.astype(np.float64)
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max() < 2 ** 24
    return y.astype(np.int64)


LIN_T = (1, 15, 16, 17, 31, 32, 33, 128, 129, 200)
LIN_OUT = (16, 40, 384, 1000)


@pytest.mark.parametrize("n_in", [128, 144, 1472, 2048, 2064, 3584, 90, 136])
def test_linear_kernels_are_exact_on_integers(n_in):
    """W, x, res integers in -8 .. 8: |sum| <= 64 * 3584 + 8 < 2^24, so every fp32 sum is exact whatever its order and the
    kernel must equal the integer product BIT FOR BIT - a dropped, doubled or misplaced k-step, row or column cannot hide
    behind a tolerance.  in 128 .. 3584 in whole 16-steps select the branch-free kernel for T <= 32 (2048: exactly 16 steps
    per wave; 2064: waves with 16 and 17: the second pass of its loop with ONE real step; 3584: 28, second pass 12 real + 4
    clamped); T = 33 .. 200 and in = 90, 136 run the generic kernel (one and two column tiles).  out not a multiple of 16:
    the clamped rows.  Then: both kernels forced to agree, three jobs of different out over one x, a residual, x pitch = T
    and > T, and the strides with which the wide decoder step writes keys / values into the caches (untouched cache elements
    must stay untouched)."""
    from phoonnx_amd import g2p
    rng = np.random.default_rng(n_in)
    XP = 208
    W, x = _ints(rng, 1000, n_in), _ints(rng, n_in, XP)
    full = _exact(W, x)
    for T in LIN_T:
        for out in LIN_OUT:
            for mode in ((0, 1) if n_in % 16 == 0 and n_in >= 128 and T <= 32 else (0,)):
                y = g2p.test_linear([W[:out]], x, T=T, mode=mode, fill=-777.0)[0].reshape(out, T)
                assert np.array_equal(y.astype(np.int64), full[:out, :T]) and np.array_equal(y, np.rint(y)), (n_in, T, out, mode)
    # three jobs with different out, residuals on two of them, x pitch == T
    for T in (1, 16, 17, 32, 33, 129):
        xt = np.ascontiguousarray(x[:, :T])
        outs = (384, 40, 1000)
        Ws = [_ints(rng, o, n_in) for o in outs]
        res = [_ints(rng, outs[0], T), None, _ints(rng, outs[2], T)]
        ys = g2p.test_linear(Ws, xt, res=res)
        for Wj, rj, yj, o in zip(Ws, res, ys, outs):
            want = _exact(Wj, xt) + (0 if rj is None else rj.astype(np.int64))
            assert np.array_equal(yj.reshape(o, T).astype(np.int64), want), (n_in, T, o)
    # the cache-write strides of the wide step: row stride TM (a cache row), column stride out * TM (the next sequence's
    # cache); everything but position 0 of every (sequence, row) keeps the fill value
    TM = 25
    for T, out in ((8, 384), (16, 384), (24, 40), (32, 384), (40, 384)):
        Ws = [_ints(rng, out, n_in), _ints(rng, out, n_in)]
        ys = g2p.test_linear(Ws, x, T=T, y_rs=TM, y_cs=out * TM, fill=-777.0)
        for Wj, yj in zip(Ws, ys):
            buf = np.full(T * out * TM, -777.0, np.float32)
            buf[:yj.size] = yj
            buf = buf.reshape(T, out, TM)
            assert np.array_equal(buf[:, :, 0].T.astype(np.int64), _exact(Wj, x[:, :T])), (n_in, T, out)
            assert np.all(buf[:, :, 1:] == -777.0), (n_in, T, out)


def _fp32_grade(got, ref64, np32, what):
    """max-abs error against float64 <= 2 x the error of an independent float32 implementation (NumPy) on the same data
    + 1e-7 x the output's largest magnitude: the rule of test_conv_sx_engine_error_is_fp32_grade (the fp32 implementation
    sets the scale, the factor 2 covers a different summation order)."""
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    base = float(np.abs(np32.astype(np.float64) - ref64).max())
    bound = 2 * base + 1e-7 * float(np.abs(ref64).max())
    print(f"{what}: err {err:.3e}  numpy-f32 {base:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, err, base, bound)


@pytest.mark.parametrize("n_in", [128, 1472, 2064, 3584, 136])
def test_linear_kernels_are_fp32_grade_and_the_branch_free_one_is_the_generic_one(n_in):
    """Gaussian operands.  Wherever the branch-free kernel is chosen it equals the generic kernel bit for bit (its header:
    same products in the same order); both are within the fp32 grade of float64."""
    from phoonnx_amd import g2p
    rng = np.random.default_rng(1000 + n_in)
    W = (rng.standard_normal((1000, n_in)) / np.sqrt(n_in)).astype(np.float32)
    x = rng.standard_normal((n_in, 208)).astype(np.float32)
    ref = W.astype(np.float64) @ x.astype(np.float64)
    np32 = W @ x
    for T in (1, 15, 16, 17, 32, 33, 129, 200):
        for out in (40, 1000):
            y = g2p.test_linear([W[:out]], x, T=T)[0].reshape(out, T)
            _fp32_grade(y, ref[:out, :T], np32[:out, :T], f"linear in {n_in} T {T} out {out}")
            if n_in % 16 == 0 and n_in >= 128 and T <= 32:
                yg = g2p.test_linear([W[:out]], x, T=T, mode=1)[0].reshape(out, T)
                assert np.array_equal(y, yg), (n_in, T, out)


def test_kernel_hooks_check_their_arguments():
    from phoonnx_amd import _ffi, g2p
    from phoonnx_amd.session import SessionError
    W, x = np.ones((4, 16), np.float32), np.ones((16, 3), np.float32)
    assert np.array_equal(g2p.test_linear([W], x)[0], np.full(12, 16.0, np.float32))
    with pytest.raises(SessionError):
        g2p.test_linear([W], x, T=0)
    with pytest.raises(SessionError):
        g2p.test_linear([W], x, T=4)                      # more columns than the pitch
    with pytest.raises(SessionError):
        g2p.test_linear([W] * 4, x)
    with pytest.raises(SessionError):
        g2p.test_linear([W], x, y_rs=1, y_cs=1)           # overlapping output elements
    with pytest.raises(SessionError):
        g2p.test_linear([W], x, mode=2)
    with pytest.raises(SessionError):
        g2p.test_step([W], np.ones((3, 16), np.float32))  # NB 3 has no kernel
    with pytest.raises(SessionError):
        g2p.test_step([W], np.ones((1, 16), np.float32), act=3)
    lib = _ffi.load()
    assert lib.g2p_test_linear(0, 1, None, None, 16, None, 3, 3, None, 3, 1, 0, None) < 0
    assert lib.g2p_test_step(0, 1, 0, None, None, None, 16, None, None, -1, 1e-6, 1.0, None, None) < 0


# ------------------------------------------------------------------------------------------------ step kernel
STEP_IN = (90, 96, 256, 1472, 3584)
STEP_OUT = (3, 384, 1001)


@pytest.mark.parametrize("NB", [1, 2, 4])
def test_step_kernel_is_exact_on_integers(NB):
    """g2p_step_kernel<NB> without norm, gate or activation (post 1) on integers -8 .. 8, with a residual: bit for bit the
    integer product.  A row of in = 1472 is 368 float4 (five full wave loads and 48 lanes), of 3584 896 (fourteen): several
    chunks per lane with the last one clamped, at every UN the NB variants use; 90: the one-float-per-lane branch; 96 and
    256: less than / exactly one wave load.  out 3 and 1001: a last workgroup with rows past the end."""
    from phoonnx_amd import g2p
    rng = np.random.default_rng(50 + NB)
    for n_in in STEP_IN:
        x = _ints(rng, NB, n_in)
        Ws = [_ints(rng, o, n_in) for o in STEP_OUT]
        for Wj, o in zip(Ws, STEP_OUT):     # one job per launch
            r = _ints(rng, NB, o)
            y = g2p.test_step([Wj], x, res=[r])[0]
            assert np.array_equal(y.astype(np.int64), _exact(Wj, x.T).T + r.astype(np.int64)) and np.array_equal(y, np.rint(y)), (NB, n_in, o)
        res = [_ints(rng, NB, STEP_OUT[0]), None, _ints(rng, NB, STEP_OUT[2])]   # three jobs in one launch
        ys = g2p.test_step(Ws, x, res=res)
        for Wj, rj, yj in zip(Ws, res, ys):
            assert np.array_equal(yj.astype(np.int64), _exact(Wj, x.T).T + (0 if rj is None else rj.astype(np.int64))), (NB, n_in)


def _step_formula(Ws, W2s, x, g, act, eps, post, res, dt):
    """The kernel's header comment in NumPy at precision dt: y = post rs W (g x) [act; gated: act(.) * (post rs W2 (g x))] + res"""
    import math
    erf = np.vectorize(math.erf, otypes=[np.float64])

    def activation(a):
        if act == 1:
            return np.maximum(a, 0)
        if act == 2:
            return (0.5 * a * (1.0 + erf(a.astype(np.float64) / math.sqrt(2.0)))).astype(dt)
        return 0.5 * a * (1.0 + np.tanh(dt(0.7978845608028654) * (a + dt(0.044715) * a * a * a)))
    x = x.astype(dt)
    rs = dt(post) * (1.0 / np.sqrt(np.mean(x * x, axis=1, keepdims=True, dtype=dt) + dt(eps)) if g is not None else dt(1.0))
    xg = x * g.astype(dt) if g is not None else x
    out = []
    for j, W in enumerate(Ws):
        y = (xg @ W.astype(dt).T) * rs
        if W2s is not None and W2s[j] is not None:
            y = activation(y) * ((xg @ W2s[j].astype(dt).T) * rs)
        elif act >= 0:
            y = activation(y)
        if res is not None and res[j] is not None:
            y = y + res[j].astype(dt)
        out.append(y.astype(dt))
    return out


@pytest.mark.parametrize("n_in", [90, 256, 1472, 3584])
def test_step_kernel_matches_its_formula_in_float64(n_in):
    """Gaussian data through every launch-uniform variant: norm folded in or not, gate or not, act -1 / 0 / 1 / 2,
    post != 1, residual - against the float64 formula, fp32 grade, for NB = 1, 2 and 4.  (The NB variants add a lane's terms
    in the same order, but they are not bit-identical per sequence: measured on in = 256, the instantiations differ in the
    last bits of many outputs - the compiler contracts the multiply-adds of each instantiation on its own - so
    each is graded against float64, not against NB = 1.)"""
    from phoonnx_amd import g2p
    rng = np.random.default_rng(70 + n_in)
    outs = (384, 1001)
    x = (rng.standard_normal((4, n_in)) * np.array([[1.0], [0.3], [3.0], [1.5]])).astype(np.float32)
    g = (1 + 0.1 * rng.standard_normal(n_in)).astype(np.float32)
    Ws = [(rng.standard_normal((o, n_in)) / np.sqrt(n_in)).astype(np.float32) for o in outs]
    W2s = [(rng.standard_normal((o, n_in)) / np.sqrt(n_in)).astype(np.float32) for o in outs]
    res = [rng.standard_normal((4, o)).astype(np.float32) for o in outs]
    variants = [(None, None, -1, 1.0, False), (g, None, -1, 1.0, False), (g, None, -1, 1472 ** -0.5, False),
                (None, None, -1, 1.0, True), (g, W2s, 0, 1.0, False), (g, W2s, 1, 0.7, False), (g, W2s, 2, 1.0, True),
                (None, W2s, 0, 1.0, False), (g, None, 0, 1.0, False), (g, None, 1, 1.0, False), (g, None, 2, 1.3, True)]
    for gv, w2, act, post, with_res in variants:
        rr = res if with_res else None
        ref = _step_formula(Ws, w2, x, gv, act, 1e-6, post, rr, np.float64)
        n32 = _step_formula(Ws, w2, x, gv, act, 1e-6, post, rr, np.float32)
        for NB in (1, 2, 4):
            ys = g2p.test_step(Ws, x[:NB], W2s=w2, g=gv, act=act, eps=1e-6, post=post, res=None if rr is None else [r[:NB] for r in rr])
            for j in range(len(Ws)):
                what = f"step in {n_in} NB {NB} job {j} norm {gv is not None} gate {w2 is not None} act {act} post {post:.3g}"
                _fp32_grade(ys[j], ref[j][:NB], n32[j][:NB], what)


# ------------------------------------------------------------------------------------------------ whole engine
_SESS, _ORACLE, _REFS = {}, {}, {}


def _sess(name):
    if name not in _SESS:
        from phoonnx_amd.g2p import MiG2PSession
        _SESS[name] = MiG2PSession(model_path(name))
    return _SESS[name]


def _oracle(name):
    if name not in _ORACLE:
        from t5_oracle import T5Oracle
        _ORACLE[name] = T5Oracle(model_path(name), dtype=np.float64)
    return _ORACLE[name]


def _pool_ref(name, b, steps):
    """float64 logits [steps, vocab] of pool sequence b for its given decoder inputs (causal: a prefix of a longer run)"""
    key = (name, b)
    if key not in _REFS or _REFS[key].shape[0] < steps:
        seqs, decs = pool()
        _REFS[key] = _oracle(name).logits(seqs[b], decs[b, :steps])[0]
    return _REFS[key][:steps]


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for s in _SESS.values():
        s.close()
    _SESS.clear()
    _ORACLE.clear()
    _REFS.clear()


def _check(name, got, ref, what):
    assert float(np.abs(ref).max()) > 1, what            # (not vacuous)
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), logits_bound(name, ref)
    print(f"{name} {what}: max|logits| {np.abs(ref).max():.1f}  err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (name, what, err, bound)


def test_run_at_byt5_width_matches_the_float64_oracle():
    """Prefill through both linear kernels (T <= 32: the branch-free one with 92 and 224 k-steps; above: the generic one)."""
    s, o = _sess("w1472_2x2"), _oracle("w1472_2x2")
    assert (s.hparam("d_model"), s.hparam("d_ff"), s.hparam("heads"), s.hparam("d_kv")) == (1472, 3584, 6, 64)
    for ids, dec in run_cases():
        got = s.run(None, {"input_ids": ids[None], "decoder_input_ids": dec[None]})[0]
        _check("w1472_2x2", got, o.logits(ids, dec), f"run S {len(ids)} T {len(dec)}")


def test_narrow_decoder_steps_at_byt5_width_match_the_float64_oracle():
    """1, 2, 3, 4 sequences of different lengths, 40 steps: the NB = 1 / 2 / 4 matrix-vector kernels on rows of several
    chunks, the caches, one-query attention."""
    s = _sess("w1472_2x2")
    seqs, decs = pool()
    for B in (1, 2, 3, 4):
        got = s.forced_step_logits(seqs[:B], decs[:B, :NARROW_STEPS])
        for b in range(B):
            _check("w1472_2x2", got[b], _pool_ref("w1472_2x2", b, NARROW_STEPS), f"narrow B {B} seq {b}")


@pytest.mark.parametrize("B", [5, 8, 16, 17, 32, 33, 64])
def test_wide_decoder_steps_at_byt5_width_match_the_oracle_and_the_sequence_alone(B):
    """NB = 8 / 8 / 16 / 24 / 32 / 40 / 64 columns: the branch-free linear kernel at CB 1 and 2 and the generic kernel above 32,
    writing keys / values straight into the caches, attention with the [C][NB] query strides - every sequence against the
    float64 oracle and, tighter, against the same sequence decoded alone on the matrix-vector path (two fp32 evaluations of
    one graph, each about F32_GAP from the exact one: 2 x F32_GAP = 6.6e-5; measured at most 2.4e-5)."""
    s = _sess("w1472_2x2")
    seqs, decs = pool()
    got = s.forced_step_logits(seqs[:B], decs[:B, :WIDE_STEPS])
    for b in range(B):
        _check("w1472_2x2", got[b], _pool_ref("w1472_2x2", b, WIDE_STEPS), f"wide B {B} seq {b}")
        key = ("alone", b)
        if key not in _REFS:
            _REFS[key] = s.forced_step_logits([seqs[b]], decs[b:b + 1, :WIDE_STEPS])[0]
        d = float(np.abs(got[b] - _REFS[key]).max())
        print(f"w1472_2x2 wide B {B} seq {b} against the sequence alone: {d:.3e}  bound {2 * F32_GAP['w1472_2x2']:.3e}")
        assert d <= 2 * F32_GAP["w1472_2x2"], (B, b, d)


@pytest.mark.parametrize("B", [8, 16])
def test_generated_ids_are_the_argmax_of_the_forced_logits(B):
    """The feedback loop and the wide argmax: the ids generate_batch returns are, at every position, the argmax of the
    logits the step path computes when it is fed exactly those ids - no position left out, no dependence on the margins
    of a random model."""
    s = _sess("w1472_2x2")
    seqs, _ = pool()
    ids = s.generate_batch(seqs[:B], max_length=WIDE_STEPS, eos_id=-1)
    assert all(len(x) == WIDE_STEPS for x in ids)
    ids = np.asarray(ids, np.int64)
    dec = np.concatenate((np.zeros((B, 1), np.int64), ids[:, :-1]), axis=1)
    lg = s.forced_step_logits(seqs[:B], dec)
    assert np.array_equal(lg.argmax(-1), ids)


def test_full_depth_model_matches_the_float64_oracle():
    """12 + 4 layers at full width: run, the narrow and the wide step."""
    name = "w1472_12x4"
    s, o = _sess(name), _oracle(name)
    assert (s.hparam("n_enc"), s.hparam("n_dec")) == (12, 4)
    (ids, dec), = run_cases(((33, 17),))
    _check(name, s.run(None, {"input_ids": ids[None], "decoder_input_ids": dec[None]})[0], o.logits(ids, dec), "run S 33 T 17")
    seqs, decs = pool()
    got = s.forced_step_logits(seqs[:5], decs[:5, :12])
    one = s.forced_step_logits(seqs[:1], decs[:1, :12])
    for b in range(5):
        ref = o.logits(seqs[b], decs[b, :12])[0]
        _check(name, got[b], ref, f"wide B 5 seq {b}")
        if b == 0:
            _check(name, one[0], ref, "narrow B 1")


@pytest.mark.parametrize("name", ["relu_tied", "gelu_erf"])
def test_relu_tied_and_erf_gelu_models_match_the_float64_oracle(name):
    """The branches of G2PModel::build, g2p_run and the step paths that the gated-tanh fixtures never take: act 1 and 2, the
    non-gated feed-forward, the tied-embedding output scale (a kernel in the prefill and the wide step, `post` in the
    matrix-vector step)."""
    s, o = _sess(name), _oracle(name)
    want = dict(relu_tied=(0, 1, 1), gelu_erf=(0, 2, 0))[name]
    assert (s.hparam("gated"), s.hparam("act"), s.hparam("scale_out")) == want
    for ids, dec in run_cases(((20, 12), (80, 40))):
        got = s.run(None, {"input_ids": ids[None], "decoder_input_ids": dec[None]})[0]
        _check(name, got, o.logits(ids, dec), f"run S {len(ids)} T {len(dec)}")
    seqs, decs = pool()
    for B in (3, 9):
        got = s.forced_step_logits(seqs[:B], decs[:B, :WIDE_STEPS])
        for b in range(B):
            _check(name, got[b], _pool_ref(name, b, WIDE_STEPS), f"forced B {B} seq {b}")


def _long_ref(name, b):
    """float64 logits [LONG_STEPS, vocab] of long_pool sequence b (computed once, shared by every test below)"""
    key = (name, "long", b)
    if key not in _REFS:
        seqs, decs = long_pool()
        _REFS[key] = _oracle(name).logits(seqs[b], decs[b])[0]
    return _REFS[key]


@pytest.mark.parametrize("B", [1, 2, 4, 5, 9])
@pytest.mark.parametrize("name", ["relu_tied", "gelu_erf"])
def test_decoder_steps_across_64_and_256_keys_match_the_float64_oracle(name, B):
    """Inputs of 300, 257, 256, 65, 64, 3, 1, 129 and 700 bytes, 270 forced steps: one-query self attention from 1 to 270 keys
    (the second lane round, the whole value prefetch and the loop behind it, the second pass of the score loop), cross
    attention over 1 .. 700 keys under `lens`, and the batched encoder over a padded batch with its longest sequence beside its
    shortest - narrow (NB 1, 2, 4: the [NB][C] query strides) and wide (NB 8, 16: [C][NB])."""
    s = _sess(name)
    seqs, decs = long_pool()
    got = s.forced_step_logits(seqs[:B], decs[:B])
    for b in range(B):
        _check(name, got[b], _long_ref(name, b), f"long forced B {B} seq {b} (input {LONG_LENS[b]})")


@pytest.mark.parametrize("name", ["relu_tied", "gelu_erf"])
def test_run_across_the_far_end_of_the_bucket_table_matches_the_float64_oracle(name):
    """The prefill at (S, T) = (1023, 5) - the longest input the engine takes: encoder self attention and cross attention over
    1023 keys, relative positions to the ends of the bucket table - and (40, 300): causal self attention over 300 columns."""
    s, o = _sess(name), _oracle(name)
    for ids, dec in run_cases(LONG_RUN_SHAPES, seed=104):
        got = s.run(None, {"input_ids": ids[None], "decoder_input_ids": dec[None]})[0]
        _check(name, got, o.logits(ids, dec), f"run S {len(ids)} T {len(dec)}")


def test_the_one_launch_decoder_step_is_bit_identical_past_256_keys(monkeypatch):
    """The B = 2 case above once more through the opt-in persistent step (VITSMI_G2P_PERSIST=1): its LDS is sized by max(S, TM)
    (cross attention over 300 keys, self attention over up to 270), the attention phases are virtual blocks of the same bodies -
    the same logits bit for bit."""
    s = _sess("gelu_erf")
    seqs, decs = long_pool()
    want = s.forced_step_logits(seqs[:2], decs[:2])
    monkeypatch.setenv("VITSMI_G2P_PERSIST", "1")
    got = s.forced_step_logits(seqs[:2], decs[:2])
    assert np.array_equal(got, want)
