"""The kernels between the token domain and the waveform, by value, through their hooks (vits_test_durations,
vits_test_expand_prior, vits_test_fill_normal[_rows], vits_test_post_conv: the pipeline's kernels on the pipeline's grids)
against the float64 / int64 references of tests/glue_ref.py and tests/philox_ref.py - at the sizes where these kernels take
another path: the 256-token passes of the duration scans, a 4-frame group that straddles an utterance's end, channel
counts that are no multiple of 4, noise shorter than the frame axis, a tile an utterance ends in, a ragged prefetch round."""
import numpy as np
import pytest

from glue_ref import durations_ref, forced_durations_ref, post_conv_ref, regulate_ref
from philox_ref import flat_noise64, row_noise, row_noise64

pytestmark = pytest.mark.gpu

DUR_T = (1, 255, 256, 257, 512, 513, 1000)
# the documented-stream test's seeds (tests/test_gpu_utterance_settings.py)
SEEDS = np.array([1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0, 42], np.uint64)


def _dur_lens(T):
    return np.array([T, 1, min(T, 257), max(T - 1, 1)], np.int64)


def _check_scan(w_ceil, cum, y_len, lens):
    """what holds whatever the values: cum is the running sum of the returned w_ceil, y_len its total (at least 1), and
    behind an utterance's end w_ceil is 0 and cum the total"""
    run = np.cumsum(w_ceil.astype(np.int64), axis=1)
    assert np.array_equal(cum, run)
    assert np.array_equal(y_len, np.maximum(run[:, -1], 1))
    for b, n in enumerate(lens):
        assert not w_ceil[b, n:].any(), b
        assert np.array_equal(cum[b, n:], np.full(w_ceil.shape[1] - n, run[b, -1])), b


# ------------------------------------------------------------------ durations

@pytest.mark.parametrize("T", DUR_T)
def test_durations_exact_family(T):
    """logw = 0 and settings whose products are exact in fp32: every output equals the reference bit for bit"""
    from phoonnx_amd.session import test_durations
    lens = _dur_lens(T)
    logw = np.zeros((4, T), np.float32)
    rng = np.random.default_rng(T)
    rate = rng.choice(np.array([0, 0.5, 1, 2, 3, 5], np.float32), (4, T))
    for ls in (0.5, 1.0, 2.0):
        for r in (None, rate):
            got = test_durations(logw=logw, lens=lens, length_scale=ls, token_rate=r)
            want = durations_ref(logw, lens, ls, r)
            for g, w, name in zip(got, want, ("w_ceil", "cum", "y_len")):
                assert np.array_equal(g, w), (name, ls, r is not None)
            _check_scan(*got, lens)
    # each utterance's own length_scale (column 1 of rows) wins over the call's
    rows = np.array([[0.667, 0.5, 0.8], [0.667, 1.0, 0.8], [0.667, 2.0, 0.8], [0.667, 1.0, 0.8]], np.float32)
    for r in (None, rate):
        got = test_durations(logw=logw, lens=lens, length_scale=7.0, rows=rows, token_rate=r)
        want = durations_ref(logw, lens, rows[:, 1], r)
        for g, w, name in zip(got, want, ("w_ceil", "cum", "y_len")):
            assert np.array_equal(g, w), (name, "rows", r is not None)
    if T > 256:
        assert got[0][0, 256:].any() and got[1][0, -1] > got[1][0, 255]      # the second pass had something to add


# chosen on the CPU: with it, at every T of DUR_T, no valid token's float64 value under the ceil lies within 1e-5 (relative) of
# an integer
RANDOM_SEED = 1
RANDOM_ROWS = np.array([[0.667, 0.8, 0.8], [0.667, 1.0, 0.8], [0.667, 1.25, 0.8], [0.667, 1.1, 0.8]], np.float32)


def _random_case(T, seed):
    rng = np.random.default_rng(seed)
    logw = rng.standard_normal((4, T)).astype(np.float32)
    rate = rng.uniform(0.5, 2.0, (4, T)).astype(np.float32)
    return logw, rate


def _clear_of_integers(pre, lens):
    valid = np.arange(pre.shape[1])[None, :] < lens[:, None]
    near = np.rint(pre)
    return bool((np.abs(pre - near)[valid] > 1e-5 * np.maximum(near, 1.0)[valid]).all())


@pytest.mark.parametrize("T", DUR_T)
def test_durations_random_family(T):
    from phoonnx_amd.session import test_durations
    lens = _dur_lens(T)
    logw, rate = _random_case(T, RANDOM_SEED)
    for kw, ls, r in (({"length_scale": 1.1}, 1.1, None), ({"length_scale": 1.0, "rows": RANDOM_ROWS}, RANDOM_ROWS[:, 1], rate)):
        w_ref, cum_ref, y_ref, pre = durations_ref(logw, lens, ls, r)
        assert _clear_of_integers(pre, lens)          # on the reference alone: the ceil cannot fall either way
        w_ceil, cum, y_len = test_durations(logw=logw, lens=lens, token_rate=r, **kw)
        _check_scan(w_ceil, cum, y_len, lens)         # (holds with or without the guard above)
        assert np.array_equal(w_ceil, w_ref)
        assert np.array_equal(cum, cum_ref) and np.array_equal(y_len, y_ref)


@pytest.mark.parametrize("T", DUR_T)
def test_forced_durations(T):
    from phoonnx_amd.session import test_durations
    lens = _dur_lens(T)
    rng = np.random.default_rng(100 + T)
    dur = rng.integers(0, 6, (4, T)).astype(np.int64)
    if T > 256:
        dur[0, 250:262] = 0                  # runs of dropped tokens across the pass boundary ...
        dur[2, 256:] = 0                     # ... and from it on
    dur[1, :lens[1]] = 0                     # a whole utterance of them: one masked frame
    dur[3, lens[3] - 1] = 1 << 20            # a count no 16-bit intermediate would hold
    for b in range(4):
        dur[b, lens[b]:] = 9                 # behind the utterance's end: not read
    got = test_durations(dur=dur, lens=lens)
    want = forced_durations_ref(dur, lens)
    for g, w, name in zip(got, want, ("w_ceil", "cum", "y_len")):
        assert np.array_equal(g, w), name
    _check_scan(*got, lens)
    assert got[2][1] == 1 and got[2][3] >= 1 << 20


# ------------------------------------------------------------------ length regulator + prior sample

def _regulator_case(T, ymax, seed):
    """B = 4 utterances whose longest has exactly `ymax` frames: row 0 over all T tokens with leading, inner and trailing
    dropped tokens, row 1 without any frame, rows 2 and 3 shorter"""
    rng = np.random.default_rng(seed)
    lens = np.array([T, min(T, 3), T // 2 + 1, max(T - 1, 1)], np.int64)
    dur = np.zeros((4, T), np.int64)
    allowed = np.ones(T, bool)
    allowed[[0, 2, T - 1]] = False           # (T >= 5)
    dur[0, allowed] = rng.multinomial(ymax, np.full(allowed.sum(), 1.0 / allowed.sum()))
    dur[2, :lens[2]] = rng.multinomial(ymax // 2, np.full(lens[2], 1.0 / lens[2]))
    dur[3, :lens[3]] = rng.multinomial(max(ymax - 1, 0), np.full(lens[3], 1.0 / lens[3]))
    _, cum, y_len = forced_durations_ref(dur, lens)
    assert int(y_len.max()) == ymax and y_len[1] == 1
    return dur, lens, cum.astype(np.int32), y_len.astype(np.int32)


REG_CASES = [(5, 1), (5, 3), (5, 255), (300, 256), (300, 257), (300, 1030)]
REG_BOUND = 2.0 ** -21    # three fp32 roundings (2^-24 each) + expf within 2 ulp (2^-22): 7 * 2^-24 of |m| + |noise term|
NOISE_BOUND = 2.0 ** -20  # of max(ra, 1): 2-ulp logf, cosf, sinf and a correctly rounded sqrtf, with a fourfold margin


@pytest.mark.parametrize("C", [1, 6, 192])
@pytest.mark.parametrize("T,ymax", REG_CASES)
def test_length_regulator(C, T, ymax):
    """z_p against the float64 regulator, to REG_BOUND of |m| + |noise term| (printed: the largest ratio seen; on an MI355X
    1.48e-7 over all cases, 0.31 of the bound)"""
    from phoonnx_amd.session import test_expand_prior
    dur, lens, cum, y_len = _regulator_case(T, ymax, 1000 * T + ymax)
    rng = np.random.default_rng(C * 7 + ymax)
    m_logs = np.concatenate([rng.standard_normal((4, C, T)), rng.uniform(-1.0, 1.0, (4, C, T))], 1).astype(np.float32)
    m_p, logs_p = m_logs[:, :C], m_logs[:, C:]
    worst = 0.0
    for F in (ymax, ymax + 5):
        valid = np.arange(F)[None, None, :] < y_len[:, None, None]
        zeros = np.zeros((4, C, F), np.float32)
        gathered = regulate_ref(m_p, logs_p, dur, zeros, 0.0, y_len, F=F)
        # noise_scale 0: z_p IS the gathered m_p, and exactly 0 where no token is
        z = test_expand_prior(m_logs, cum, lens, y_len, F, noise_scale=0.0)
        assert np.array_equal(z, gathered) and not z[~np.broadcast_to(valid, z.shape)].any()
        noise = rng.standard_normal((4, C, F)).astype(np.float32)
        assert np.array_equal(test_expand_prior(m_logs, cum, lens, y_len, F, noise=noise, noise_scale=0.0), gathered)
        # ... via rows on one row only: that row exactly, the others within the bound
        rows = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (4, 1))
        rows[2, 0] = 0.0
        for Fn, ns, rw in ((F, 0.667, None), (max(F - 3, 0), 0.667, None), (F, 0.3, rows)):
            z = test_expand_prior(m_logs, cum, lens, y_len, F, noise=noise[:, :, :Fn], noise_scale=ns, rows=rw)
            m, e = regulate_ref(m_p, logs_p, dur, noise[:, :, :Fn], ns if rw is None else rw[:, 0], y_len, F=F, parts=True)
            err, scale = np.abs(z - (m + e)), np.abs(m) + np.abs(e)
            assert (err <= REG_BOUND * scale).all(), (F, Fn, float((err / np.maximum(scale, 1e-30)).max()))
            worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max()))
            if rw is not None:
                assert np.array_equal(z[2], gathered[2])
            if Fn < F:
                assert np.array_equal(z[:, :, Fn:], gathered[:, :, Fn:])
        # seeds: each utterance's own stream 2, drawn in the kernel
        z = test_expand_prior(m_logs, cum, lens, y_len, F, seeds=SEEDS, noise_scale=0.667)
        drawn = np.stack([row_noise(int(s), 2, C, F) for s in SEEDS])
        ra = np.stack([row_noise64(int(s), 2, C, F)[1] for s in SEEDS])
        m, e = regulate_ref(m_p, logs_p, dur, drawn, 0.667, y_len, F=F, parts=True)
        gain = np.abs(regulate_ref(np.zeros_like(m_p), logs_p, dur, np.ones_like(drawn), 0.667, y_len, F=F))      # exp(logs) * noise_scale
        err, scale = np.abs(z - (m + e)), np.abs(m) + np.abs(e)
        assert (err <= REG_BOUND * scale + NOISE_BOUND * np.maximum(ra, 1.0) * gain).all(), F
        assert np.abs(e).max() > 0.01                      # (the bound leaves no room for a stream that was not drawn)
    print(f"length regulator C={C} T={T} y_len.max()={ymax}: largest |z_p - ref64| / (|m| + |noise term|) = {worst:.3e} "
          f"= {worst / REG_BOUND:.3f} of the bound")


# ------------------------------------------------------------------ noise

def _noise_ratio(got, ref, ra):
    return float((np.abs(got - ref) / np.maximum(ra, 1.0)).max())


def test_fill_normal_rows():
    """The per-utterance stream against the float64 Box-Muller of the same uniforms, to NOISE_BOUND of max(ra, 1) (printed:
    the largest ratio seen; on an MI355X 1.31e-7, 0.14 of the bound)"""
    from phoonnx_amd.session import test_fill_normal_rows as fill_rows
    rows = np.array([[0.667, 1.0, 0.8], [0.5, 1.2, 1.0], [0.667, 0.9, 0.0], [0.3, 1.0, 0.5]], np.float32)
    worst = 0.0
    for T in (1, 3, 4, 5, 257):
        got = fill_rows(T, 2, SEEDS, 1, rows, 2)
        assert got.shape == (4, 2, T)
        for b, s in enumerate(SEEDS):
            ref, ra = row_noise64(int(s), 1, 2, T)
            ref = ref * np.float64(rows[b, 2])
            ratio = _noise_ratio(got[b], ref, ra)
            assert ratio <= NOISE_BOUND, (T, b, ratio)
            worst = max(worst, ratio)
        assert not got[2].any() and not np.signbit(got[2]).any()         # noise_w 0 writes +0.0
        assert not np.array_equal(got[1], got[3] * 2)                    # two seeds, two streams (noise_w 1 and 0.5: exact)
        if T >= 5:
            assert (got[1][:, :T - 4] != got[1][:, 4:]).all()            # the block counter advances
    print(f"fill_normal_rows: largest |got - ref64| / max(ra, 1) = {worst:.3e} = {worst / NOISE_BOUND:.3f} of the bound")


def test_fill_normal():
    """The flat stream against the float64 Box-Muller of the same uniforms, to NOISE_BOUND of max(ra, 1) (printed: the
    largest ratio seen; on an MI355X 1.33e-7, 0.14 of the bound)"""
    from phoonnx_amd.session import test_fill_normal as fill
    worst = 0.0
    for n in (1, 4, 7, 1026):
        for stream in (1, 2, (5 << 32) | 3):
            got = fill(n, 1234, stream)
            ref, ra = flat_noise64(1234, stream, n)
            ratio = _noise_ratio(got, ref, ra)
            assert ratio <= NOISE_BOUND, (n, stream, ratio)
            worst = max(worst, ratio)
        assert not np.array_equal(fill(n, 1234, 1), fill(n, 1235, 1))    # two seeds, two streams
        assert not np.array_equal(fill(n, 1234, 1), fill(n, 1234, 1 << 32))
        if n >= 5:
            assert (got[:n - 4] != got[4:]).all()                         # the block counter advances
    print(f"fill_normal: largest |got - ref64| / max(ra, 1) = {worst:.3e} = {worst / NOISE_BOUND:.3f} of the bound")


# ------------------------------------------------------------------ vocoder tail

TAIL_KERNELS = ("planar", "blocked", "blocked_generic")
TAIL_CK = [(C, K) for C in (8, 16, 32) for K in (7, 3, 5)]


def _tail_inputs(C, K, B, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, T)).astype(np.float32)
    w = (rng.standard_normal((C, K)) / np.sqrt(C * K)).astype(np.float32)      # the sum under the tanh has unit variance
    return x, w


@pytest.mark.parametrize("C,K", TAIL_CK)
def test_vocoder_tail_matches_reference(C, K):
    """C = 32: (C / 8) * (256 + K - 1) = 1048 staged cells at K = 7, 1032 at K = 3 - a ragged second prefetch round"""
    from phoonnx_amd.session import test_post_conv
    for T in (1, 5, 255, 256, 257, 700):
        x, w = _tail_inputs(C, K, 2, T, 31 * C + K + T)
        for slope in (0.01, 1.0):           # (the two slopes the pipeline passes)
            want = post_conv_ref(x, w, slope)
            for kernel in TAIL_KERNELS:
                got = test_post_conv(x, w, slope, kernel=kernel)
                np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-5, err_msg=f"{kernel} T={T} slope={slope}")


@pytest.mark.parametrize("C,K", TAIL_CK)
def test_vocoder_tail_ragged_batch(C, K):
    """T = 700 samples of hop 4: an utterance over the whole row, one that ends inside a tile (300), one that ends on the
    256 boundary, an empty one.  Zeros at and behind each end, and nothing behind an end (plus the taps that reach over
    it) is read for a sample that is kept."""
    from phoonnx_amd.session import test_post_conv
    T, hop, vlen = 700, 4, np.array([175, 75, 64, 0], np.int64)
    x, w = _tail_inputs(C, K, 4, T, 77 * C + K)
    want = post_conv_ref(x, w, 0.01, vlen, hop)
    poisoned = x.copy()
    for b in range(4):
        poisoned[b, :, vlen[b] * hop + (K - 1) // 2:] = np.nan
    for kernel in TAIL_KERNELS:
        got = test_post_conv(x, w, 0.01, vlen, hop, kernel=kernel)
        np.testing.assert_allclose(got, want, atol=2e-5, rtol=1e-5, err_msg=kernel)
        for b in range(4):
            assert not got[b, vlen[b] * hop:].any(), (kernel, b)
        assert np.abs(got[1, :300]).max() > 0.1 and np.abs(got[2, :256]).max() > 0.1
        again = test_post_conv(poisoned, w, 0.01, vlen, hop, kernel=kernel)
        assert np.isfinite(again).all(), kernel
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), kernel


@pytest.mark.parametrize("C,K", [(8, 7), (16, 3), (32, 5), (32, 7)])
def test_vocoder_tail_single_tap(C, K):
    """One nonzero weight (1.0 at channel c, tap k) over a ramp in t: the sum under the tanh is the ramp shifted by
    k - pad, exactly - a reversed tap order or a wrong pad moves it.  Compared through arctanh where |sum| < 1."""
    from phoonnx_amd.session import test_post_conv
    T = 300
    rng = np.random.default_rng(C + K)
    for c, k in ((0, 0), (C - 1, K - 1), (C // 2 + 1, 1), (3, K // 2)):
        x = rng.standard_normal((2, C, T)).astype(np.float32)
        x[:, c, :] = (0.01 * (np.arange(T) - 150)).astype(np.float32)[None, :]
        w = np.zeros((C, K), np.float32)
        w[c, k] = 1.0
        acc = post_conv_ref(x, w, 0.5, acc=True)
        inside = np.abs(acc) < 1
        assert inside.sum() > 2 * 200
        for kernel in TAIL_KERNELS:
            got = test_post_conv(x, w, 0.5, kernel=kernel).astype(np.float64)
            np.testing.assert_allclose(np.arctanh(got[inside]), acc[inside], atol=1e-6, rtol=0, err_msg=f"{kernel} ({c}, {k})")
            np.testing.assert_allclose(got, np.tanh(acc), atol=2e-5, rtol=1e-5, err_msg=f"{kernel} ({c}, {k})")


# ------------------------------------------------------------------ what the hooks refuse

def test_hooks_refuse_what_a_kernel_could_leave_its_buffers_with():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import (SessionError, test_durations, test_expand_prior, test_fill_normal, test_fill_normal_rows,
                                     test_post_conv)
    logw = np.zeros((2, 8), np.float32)
    for lens in ([8, 9], [-1, 3]):                                    # lens outside [0, T]
        with pytest.raises(SessionError, match=r"outside \[0,8\]"):
            test_durations(logw=logw, lens=np.array(lens, np.int64))
    with pytest.raises(SessionError, match="negative"):
        test_durations(dur=np.array([[1, -2, 3]], np.int64), lens=np.array([3], np.int64))
    x, w = np.zeros((1, 12, 40), np.float32), np.zeros((12, 7), np.float32)
    with pytest.raises(SessionError, match="8 channels per cell"):      # C % 8 on the blocked tail
        test_post_conv(x, w, 0.01, kernel="blocked")
    # ... which the library refuses itself, whoever calls it
    out = np.zeros((1, 40), np.float32)
    rc = _ffi.load().vits_test_post_conv(0, _ffi.ptr(x), 1, 12, 40, _ffi.ptr(w), 7, 0.01, None, 1, 1, _ffi.ptr(out))
    assert rc == -3 and "8 channels per cell" in _ffi.last_error(None)
    for kernel, C in (("planar", 64), ("blocked", 64), ("blocked_generic", 64)):   # 64 * 262 * 4 bytes of LDS > 64 KiB
        with pytest.raises(SessionError, match="more than 64 KiB"):
            test_post_conv(np.zeros((1, C, 40), np.float32), np.zeros((C, 7), np.float32), 0.01, kernel=kernel)
    with pytest.raises(SessionError, match="not a frame count"):
        test_post_conv(np.zeros((1, 8, 40), np.float32), np.zeros((8, 7), np.float32), 0.01, vlen=np.array([-1], np.int64))
    # the length regulator: noise_frames beyond the noise array, y_len beyond F, y_len and cum that disagree, bad lens
    m_logs = np.zeros((1, 4, 3), np.float32)
    cum, lens, y_len = np.array([[2, 4, 6]], np.int32), np.array([3], np.int64), np.array([6], np.int32)
    assert test_expand_prior(m_logs, cum, lens, y_len, 6, noise_scale=0.0).shape == (1, 2, 6)
    with pytest.raises(SessionError, match="noise rows hold 4"):
        test_expand_prior(m_logs, cum, lens, y_len, 6, noise=np.zeros((1, 2, 4), np.float32), noise_frames=6)
    with pytest.raises(SessionError, match="F=5"):
        test_expand_prior(m_logs, cum, lens, y_len, 5, noise_scale=0.0)
    with pytest.raises(SessionError, match="y_len"):
        test_expand_prior(m_logs, cum, lens, np.array([5], np.int32), 6, noise_scale=0.0)
    with pytest.raises(SessionError, match="running sum"):
        test_expand_prior(m_logs, np.array([[2, 1, 6]], np.int32), lens, y_len, 6, noise_scale=0.0)
    with pytest.raises(SessionError, match=r"outside \[0,3\]"):
        test_expand_prior(m_logs, cum, np.array([4], np.int64), y_len, 6, noise_scale=0.0)
    # negative sizes
    with pytest.raises(SessionError):
        test_fill_normal(-1, 1, 1)
    with pytest.raises(SessionError):
        test_fill_normal_rows(-4, 2, SEEDS, 1, np.ones((4, 3), np.float32), 2)
    with pytest.raises(SessionError):
        test_fill_normal_rows(4, 2, SEEDS, 1, np.ones((4, 3), np.float32), 3)
    with pytest.raises(SessionError):
        test_expand_prior(m_logs, cum, lens, y_len, -6, noise_scale=0.0)
