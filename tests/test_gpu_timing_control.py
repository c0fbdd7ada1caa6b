"""Per-phoneme timing on the GPU: durations out (vits_last_durations), forced durations and per-token rates in
(vits_run_async_ctl / vits_run_chunked_ctl), phoneme alignments on TTSVoice.  Equality is np.array_equal unless a
tolerance is named; the only tolerance is the one tests/test_gpu_utterance_settings.py uses for these fixtures."""
import json
import os
import threading

import numpy as np
import pytest

from conftest import ALL_PRESETS, GOLDEN, case_get, golden_cases, zero_tails
from glue_ref import regulate_ref as _regulate   # (the NumPy length regulator + prior sample)

pytestmark = pytest.mark.gpu

KEYS = ("ids", "lens", "scales", "sid", "noise_dp", "noise_z")


def _tol(preset):   # (tests/test_gpu_utterance_settings.py's, for the same fixtures)
    return 1e-5 if preset.startswith("tiny") else 2e-5


def _path(preset):
    return os.path.join(GOLDEN, preset + ".onnx")


def _case(preset, case="b3_noise"):
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    return [case_get(g, case, k) for k in KEYS]


def _frames(dur):
    return np.maximum(dur.sum(axis=1), 1)


def _mixed_rows(B):
    rows = np.empty((B, 3), np.float32)
    for b in range(B):
        rows[b] = [(0.5, 0.667, 0.0, 0.8)[b % 4], (0.8, 1.0, 1.25)[b % 3], (0.6, 0.8, 0.0)[b % 3]]
    return rows


def _batch(rng, B, T, n_vocab):
    lens = rng.integers(max(2, T // 3), T + 1, B).astype(np.int64)
    lens[0] = T
    ids = rng.integers(1, n_vocab, (B, T)).astype(np.int64)
    for b in range(B):
        ids[b, lens[b]:] = 0
    return ids, lens


def _stream(s, *a, **kw):
    """synthesize_stream, concatenated: ([B, S] samples, what the consumer thread read after the first chunk)"""
    got, seen = None, None
    for first, samples, total in s.synthesize_stream(*a, **kw):
        if got is None:
            got = np.full((samples.shape[0], total), np.nan, np.float32)
            seen = (s.last_durations(), s.last_y_lengths(), threading.get_ident())   # while later chunks render
        got[:, first:first + samples.shape[1]] = samples
    return got, seen


# ------------------------------------------------------------------ 1. durations out = the oracle's w_ceil

@pytest.mark.parametrize("preset", ALL_PRESETS)
def test_durations_out_are_the_oracles(preset):
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession
    from vits_oracle import VitsOracle
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    s = MiSession(_path(preset))
    o = VitsOracle(_path(preset))
    p = PipelinedSession(s, parts=2)
    for case in golden_cases(g):
        ids, lens, sc, sid, ndp, nz = [case_get(g, case, k) for k in KEYS]
        ref = o.infer(ids, lens, sc, sid, ndp, nz)
        want = ref["w_ceil"].astype(np.int64)
        r = s.synthesize_batch(ids, lens, sc, sid, ndp, nz, taps=("w_ceil",), return_durations=True)
        assert r["durations"].dtype == np.int64 and r["durations"].shape == ids.shape, case
        assert np.array_equal(r["durations"], want), case
        assert np.array_equal(r["durations"], r["w_ceil"].astype(np.int64)), case
        assert np.array_equal(r["durations"], s.last_durations()), case
        assert np.array_equal(_frames(r["durations"]), r["y_lengths"]), case
        assert np.array_equal(r["y_lengths"], ref["y_lengths"]), case
        for b in range(ids.shape[0]):
            assert not r["durations"][b, lens[b]:].any(), (case, b)
        assert "durations" not in s.synthesize_batch(ids, lens, sc, sid, ndp, nz), case   # without the flag: today's keys
        # ... from the consumer thread of a chunked run, after the first chunk
        _, (dur, ylen, _) = _stream(s, ids, lens, sc, sid, chunk_frames=8, noise_dp=ndp, noise_z=nz)
        assert np.array_equal(dur, want) and np.array_equal(ylen, ref["y_lengths"]), case
        # ... and through PipelinedSession, with the same injected noise (each part gets its rows of it)
        rp = p.synthesize_batch(ids, lens, sc, sid, noise_dp=ndp, noise_z=nz, return_durations=True)
        assert np.array_equal(rp["durations"], want), case
        assert np.array_equal(rp["durations"], p.last_durations(ids.shape[0])), case
        assert np.array_equal(_frames(rp["durations"]), rp["y_lengths"]), case
        assert np.array_equal(rp["y_lengths"], ref["y_lengths"]), case
        assert "durations" not in p.synthesize_batch(ids, lens, sc, sid, noise_dp=ndp, noise_z=nz), case
    p.close()


def test_durations_follow_the_other_last_run_getters():
    """"no completed run" before the first run, after a reserve that grows the token workspace, and after a vocoder-only
    run (no tokens)."""
    from phoonnx_amd import MiSession, SessionError
    ids, lens, sc, sid, ndp, nz = _case("tiny_rb1")
    s = MiSession(_path("tiny_rb1"))
    with pytest.raises(SessionError, match="no completed run"):
        s.last_durations()
    s.synthesize_batch(ids, lens, sc, sid, ndp, nz)
    assert s.last_durations().shape == ids.shape
    s.reserve(8, 4 * ids.shape[1], 64)
    with pytest.raises(SessionError, match="no completed run"):
        s.last_durations()
    s.synthesize_batch(ids, lens, sc, sid, ndp, nz)
    assert s.last_durations().shape == ids.shape
    s.vocoder(np.zeros((1, s.hparam("inter"), 12), np.float32))
    with pytest.raises(SessionError, match="no completed run"):
        s.last_durations()
    s.close()


# ------------------------------------------------------------------ 2. forced = free, bit for bit

@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "tiny_dp", "sx_rb1", "sx_rb2_ms"])
def test_forced_run_is_the_free_run_bit_for_bit(preset):
    from phoonnx_amd import MiSession
    s = MiSession(_path(preset))
    rng = np.random.default_rng(21)
    B, T = 5, 40
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    sid = (np.arange(B) % s.hparam("n_speakers")).astype(np.int64) if s.hparam("gin") else None
    rows = _mixed_rows(B)
    seeds = np.arange(3, 3 + B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    free = s.synthesize_batch(ids, lens, rows, sid, taps=("z_p", "z", "w_ceil"), seeds=seeds, return_durations=True)
    free_stats = s.stats()
    assert free_stats["dp_flops"] > 0
    forced = s.synthesize_batch(ids, lens, rows, sid, taps=("z_p", "z", "w_ceil"), seeds=seeds, durations=free["durations"],
                                return_durations=True)
    forced_stats = s.stats()
    assert forced_stats["dp_flops"] == 0
    assert forced_stats["total_launches"] < free_stats["total_launches"]
    for k in ("y_lengths", "durations", "w_ceil", "z_p", "z", "output"):
        assert np.array_equal(free[k], forced[k]), k
    # the unused settings of a forced run really are unused: another length_scale / noise_w, the same bits
    other = rows.copy()
    other[:, 1] *= 1.7
    other[:, 2] = 0.3
    again = s.synthesize_batch(ids, lens, other, sid, seeds=seeds, durations=free["durations"])
    assert np.array_equal(again["output"], free["output"])
    # the same forced request, chunked
    got, (dur, ylen, _) = _stream(s, ids, lens, rows, sid, chunk_frames=24, seeds=seeds, durations=free["durations"])
    assert np.array_equal(dur, free["durations"]) and np.array_equal(ylen, free["y_lengths"])
    assert np.array_equal(got, free["output"][:, 0, 0, :])
    s.close()


def test_forced_rows_through_the_pipeline():
    """PipelinedSession deals the rows of `durations` to its parts like the rows of `scales`."""
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession
    s = MiSession(_path("sx_rb1"))
    rng = np.random.default_rng(22)
    B, T = 7, 36
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    dur = rng.integers(0, 6, (B, T)).astype(np.int64)
    for b in range(B):
        dur[b, lens[b]:] = 0
    rows = _mixed_rows(B)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(1 << 40)
    p = PipelinedSession(s, parts=2)
    two = p.synthesize_batch(ids, lens, rows, None, seeds=seeds, durations=dur, return_durations=True)
    assert np.array_equal(two["durations"], dur) and np.array_equal(two["y_lengths"], _frames(dur))
    rate = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), (B, T))
    free = s.synthesize_batch(ids, lens, rows, None, seeds=seeds, token_rate=rate, return_durations=True)
    piped = p.synthesize_batch(ids, lens, rows, None, seeds=seeds, token_rate=rate, return_durations=True)
    assert np.array_equal(free["durations"], piped["durations"])
    p.close()


# ------------------------------------------------------------------ 3. forced, edited = the graph at another length scale

@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "sx_rb2_ms"])
def test_forced_durations_of_another_length_scale_give_that_rendering(preset):
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    ids, lens, sc, sid, ndp, _ = _case(preset)
    s = MiSession(_path(preset))
    o = VitsOracle(_path(preset))
    slow = np.array([sc[0], 1.75, sc[2]], np.float32)
    F = int(o.infer(ids, lens, slow, sid, ndp, None)["y_lengths"].max())     # (frame counts: noise_dp and the scales only)
    nz = np.random.default_rng(31).standard_normal((ids.shape[0], s.hparam("inter"), F + 8)).astype(np.float32)
    ref = o.infer(ids, lens, slow, sid, ndp, nz)
    assert int(ref["y_lengths"].max()) == F
    plain = np.array([sc[0], 1.0, sc[2]], np.float32)
    got = s.synthesize_batch(ids, lens, plain, sid, None, nz, durations=ref["w_ceil"].astype(np.int64))
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    hop = s.hparam("hop")
    want = zero_tails(ref["output"], ref["y_lengths"], hop)
    assert got["output"].shape == want.shape
    err = float(np.abs(got["output"] - want).max())
    print(f"{preset}: forced at the oracle's length_scale 1.75 durations, max |gpu - oracle| = {err:.3e} (frames {ref['y_lengths']})")
    assert err < _tol(preset), err
    s.close()


# ------------------------------------------------------------------ 4. per-token rate

@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "tiny_dp", "sx_rb2_ms"])
def test_token_rate(preset):
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    ids, lens, sc, sid, ndp, nz = _case(preset)
    B, T = ids.shape
    s = MiSession(_path(preset))
    o = VitsOracle(_path(preset))
    # rate 1.0 everywhere: the bits of the run without rates
    base = s.synthesize_batch(ids, lens, sc, sid, ndp, nz, taps=("z",), return_durations=True)
    ones = s.synthesize_batch(ids, lens, sc, sid, ndp, nz, taps=("z",), token_rate=np.ones((B, T), np.float32),
                              return_durations=True)
    for k in ("durations", "y_lengths", "z", "output"):
        assert np.array_equal(base[k], ones[k]), k
    # length_scale 1.0, rate r1 on the first half of the tokens and r2 behind: the graph's durations at those length scales
    r1, r2, h = 1.75, 0.5, T // 2
    rate = np.full((B, T), r2, np.float32)
    rate[:, :h] = r1
    unit = np.array([sc[0], 1.0, sc[2]], np.float32)
    got = s.synthesize_batch(ids, lens, unit, sid, ndp, None, token_rate=rate, return_durations=True)["durations"]
    w1 = o.infer(ids, lens, np.array([sc[0], r1, sc[2]], np.float32), sid, ndp, None)["w_ceil"].astype(np.int64)
    w2 = o.infer(ids, lens, np.array([sc[0], r2, sc[2]], np.float32), sid, ndp, None)["w_ceil"].astype(np.int64)
    assert np.array_equal(got[:, :h], w1[:, :h])
    assert np.array_equal(got[:, h:], w2[:, h:])
    # ... the same rates through the chunked entry point
    _, (dur, ylen, _) = _stream(s, ids, lens, unit, sid, chunk_frames=32, noise_dp=ndp, token_rate=rate)
    assert np.array_equal(dur, got) and np.array_equal(ylen, _frames(got))
    # rate 0 on a span drops those tokens: zero durations there, and exactly their free durations fewer frames
    free = s.synthesize_batch(ids, lens, unit, sid, ndp, None, return_durations=True)
    rate = np.ones((B, T), np.float32)
    rate[:, 3:9] = 0.0
    cut = s.synthesize_batch(ids, lens, unit, sid, ndp, None, token_rate=rate, return_durations=True)
    assert not cut["durations"][:, 3:9].any()
    keep = np.ones(T, bool)
    keep[3:9] = False
    assert np.array_equal(cut["durations"][:, keep], free["durations"][:, keep])
    assert free["durations"][:, 3:9].sum() > 0
    assert np.array_equal(cut["y_lengths"], np.maximum(free["durations"].sum(1) - free["durations"][:, 3:9].sum(1), 1))
    s.close()


# ------------------------------------------------------------------ 4b. dropped tokens (0 frames) in the length regulator

@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_dp", "sx_rb2_ms"])
def test_dropped_tokens_render_what_the_length_regulator_gives(preset):
    """Tokens of 0 frames - forced 0, rate 0 - are the two cases a free run practically never produces: leading, trailing
    and inner ones, and a whole utterance of them.  z_p against a NumPy length regulator over the same run's m_p / logs_p
    (exactly at noise_scale 0, where z_p IS the gathered m_p; within the fixtures' tolerance with injected noise, whose
    product goes through the device's expf), and the chunked rendering against the whole one."""
    from phoonnx_amd import MiSession
    ids, lens, sc, sid, ndp, _ = _case(preset)
    B, T = ids.shape
    s = MiSession(_path(preset))
    rng = np.random.default_rng(41)
    nz = rng.standard_normal((B, s.hparam("inter"), 4 * T + 8)).astype(np.float32)
    dur = rng.integers(0, 4, (B, T)).astype(np.int64)
    for b in range(B):
        dur[b, lens[b]:] = 0
    dur[0, :3] = 0                       # leading
    dur[0, lens[0] - 2:lens[0]] = 0      # trailing
    dur[1, 5:11] = 0                     # a run inside
    dur[2, :] = 0                        # a whole utterance: one masked frame
    taps = ("m_p", "logs_p", "z_p")

    def check(r, d, noise_scale, what):
        assert np.array_equal(r["durations"], d), what
        assert np.array_equal(r["y_lengths"], _frames(d)), what
        want = _regulate(r["m_p"], r["logs_p"], d, nz, noise_scale, r["y_lengths"])
        for b in range(B):
            n = int(r["y_lengths"][b])
            got = r["z_p"][b, :, :n]
            if noise_scale == 0:
                assert np.array_equal(got, want[b, :, :n]), (what, b)
            else:
                err = float(np.abs(got - want[b, :, :n]).max())
                print(f"{preset}: {what}, row {b}: max |z_p - regulator| = {err:.3e}")
                assert err < _tol(preset), (what, b, err)
        assert np.isfinite(r["output"]).all(), what

    for noise_scale in (0.0, float(sc[0])):
        scales = np.array([noise_scale, 1.0, sc[2]], np.float32)
        forced = s.synthesize_batch(ids, lens, scales, sid, None, nz, taps=taps, durations=dur, return_durations=True)
        check(forced, dur, noise_scale, f"forced, noise_scale {noise_scale}")
        got, _ = _stream(s, ids, lens, scales, sid, chunk_frames=16, noise_z=nz, durations=dur)
        assert np.array_equal(got, forced["output"][:, 0, 0, :])
        # rate 0: the free durations with the same tokens dropped
        free = s.synthesize_batch(ids, lens, scales, sid, ndp, nz, return_durations=True)["durations"]
        rate = (dur > 0).astype(np.float32)
        cut = s.synthesize_batch(ids, lens, scales, sid, ndp, nz, taps=taps, token_rate=rate, return_durations=True)
        check(cut, np.where(dur > 0, free, 0), noise_scale, f"rate 0, noise_scale {noise_scale}")
        got, _ = _stream(s, ids, lens, scales, sid, chunk_frames=16, noise_dp=ndp, noise_z=nz, token_rate=rate)
        assert np.array_equal(got, cut["output"][:, 0, 0, :])
    s.close()


def test_stream_owns_the_arrays_its_call_reads():
    """synthesize_stream's C call runs on a worker thread after synthesize_stream has returned: converted copies of its
    arguments ([3] scales -> rows, int32 durations, float64 rates, list seeds, float64 noise) must live as long as the
    generator.  Garbage is collected and the allocator churned between the call and the first chunk."""
    import gc
    from phoonnx_amd import MiSession
    ids, lens, sc, sid, ndp, nz = _case("tiny_rb2_ms")
    B, T = ids.shape
    s = MiSession(_path("tiny_rb2_ms"))
    seeds = [7 + b for b in range(B)]
    free = s.synthesize_batch(ids, lens, sc, sid, ndp.astype(np.float64), nz.astype(np.float64), seeds=seeds,
                              return_durations=True)

    def run(**kw):
        gen = s.synthesize_stream(ids, lens, sc, sid, chunk_frames=16, noise_dp=ndp.astype(np.float64),
                                  noise_z=nz.astype(np.float64), seeds=list(seeds), **kw)
        gc.collect()
        junk = [np.full(n, 0x7F, np.uint8) for n in (36, 12 * B, 8 * B, 4 * B * T, 8 * B * T, ndp.nbytes, nz.nbytes) * 8]
        got = None
        for first, samples, total in gen:
            if got is None:
                got = np.full((B, total), np.nan, np.float32)
            got[:, first:first + samples.shape[1]] = samples
        del junk
        return got

    assert np.array_equal(run(), free["output"][:, 0, 0, :])
    assert np.array_equal(run(durations=free["durations"].astype(np.int32)), free["output"][:, 0, 0, :])
    assert np.array_equal(run(token_rate=np.ones((B, T), np.float64)), free["output"][:, 0, 0, :])
    s.close()


# ------------------------------------------------------------------ 5. rejections

def test_bad_durations_and_rates_are_rejected_on_the_host():
    """Nothing huge is allocated or rendered: every bad value is refused before anything is enqueued, by MiSession and -
    for callers of the C ABI - by the engine itself, and the previous run stays readable."""
    import ctypes as C
    from phoonnx_amd import MiSession, SessionError, _ffi
    ids, lens, sc, sid, ndp, nz = _case("tiny_rb1")
    B, T = ids.shape
    s = MiSession(_path("tiny_rb1"))
    before = s.synthesize_batch(ids, lens, sc, sid, ndp, nz, return_durations=True)
    ws = s.hparam("workspace_bytes")
    good = before["durations"]

    def bad(b, t, v, arr=good):
        a = np.array(arr, copy=True)
        a[b, t] = v
        return a

    rate = np.ones((B, T), np.float32)
    calls = [("durations[1,4]", dict(durations=bad(1, 4, -3))),
             ("durations[2,7]", dict(durations=bad(2, 7, 2 ** 40))),
             # (the ROW SUM passes the limit at that token: min(VITS_MAX_FORCED_FRAMES, INT_MAX / hop) frames)
             (f"durations[0,{min(2 ** 24, (2 ** 31 - 1) // s.hparam('hop')) // 2 ** 20}]",
              dict(durations=np.full((B, T), 2 ** 20, np.int64))),
             ("token_rate[1,0]", dict(token_rate=bad(1, 0, np.inf, rate))),
             ("token_rate[0,5]", dict(token_rate=bad(0, 5, np.nan, rate))),
             ("token_rate[2,2]", dict(token_rate=bad(2, 2, -1.0, rate)))]
    for name, kw in calls:
        with pytest.raises(SessionError) as ei:
            s.synthesize_batch(ids, lens, sc, sid, ndp, nz, **kw)
        assert name in str(ei.value), (name, str(ei.value))
        with pytest.raises(SessionError) as ei:
            list(s.synthesize_stream(ids, lens, sc, sid, **kw))
        assert name in str(ei.value), (name, str(ei.value))
        assert np.array_equal(s.last_y_lengths(), before["y_lengths"]), name
        assert np.array_equal(s.last_durations(), good), name
    # the engine's own checks (a caller that is not MiSession)
    rows = np.tile(sc, (B, 1)).astype(np.float32)
    noise = _ffi.VitsNoise()

    def ctl_call(durations=None, token_rate=None):
        ctl = _ffi.VitsControls()
        ctl.scales_rows = rows.ctypes.data
        ctl.durations = None if durations is None else durations.ctypes.data
        ctl.token_rate = None if token_rate is None else token_rate.ctypes.data
        rc = s._lib.vits_run_async_ctl(s._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(sid), C.byref(noise), C.byref(ctl))
        return rc, s._err()

    for name, kw in calls:
        rc, err = ctl_call(**{k: np.ascontiguousarray(v) for k, v in kw.items()})
        assert rc == -3 and name in err, (name, rc, err)
    rc, err = ctl_call(durations=good, token_rate=rate)
    assert rc == -3 and "contradictory" in err
    assert np.array_equal(s.last_y_lengths(), before["y_lengths"]) and np.array_equal(s.last_durations(), good)
    assert s.hparam("workspace_bytes") == ws                      # nothing was allocated for any of them
    assert np.array_equal(s.tap("w_ceil").astype(np.int64), good)    # the previous run's device results too
    # after a forced run there is no logw to tap; w_ceil holds the forced values
    forced = bad(0, 0, 0)     # (the first token dropped: shorter than before, so the fixture's noise_z still covers it)
    assert good[0, 0] > 0
    s.synthesize_batch(ids, lens, sc, sid, ndp, nz, durations=forced)
    with pytest.raises(SessionError, match="not computed in a forced-duration run"):
        s.tap("logw")
    assert np.array_equal(s.tap("w_ceil").astype(np.int64), forced)
    s.synthesize_batch(ids, lens, sc, sid, ndp, nz)
    assert s.tap("logw").shape == (B, 1, T)
    s.close()


# ------------------------------------------------------------------ 6. phoneme alignments on TTSVoice

LETTERS = "abcdefghijklmnopqrstuvwxyz"


@pytest.mark.parametrize("preset", ["tiny_rb1", "sx_rb2_ms"])
def test_voice_alignments(preset, tmp_path):
    from phoonnx_amd import MiSession
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.voice import TTSVoice
    probe = MiSession(_path(preset), host_only=True)
    n_vocab, n_spk = probe.hparam("n_vocab"), probe.hparam("n_speakers")
    rate = probe.meta("sample_rate")
    probe.close()
    id_map = {"_": [0], "^": [1], "$": [2], " ": [3]}
    id_map.update({c: [4 + i % (n_vocab - 4)] for i, c in enumerate(LETTERS)})
    cfg_path = tmp_path / (preset + ".onnx.json")
    cfg_path.write_text(json.dumps({
        "phoneme_type": "graphemes", "lang_code": "en", "audio": {"sample_rate": int(rate or 22050)},
        "num_symbols": n_vocab, "num_speakers": n_spk, "phoneme_id_map": id_map,
        "pad": "_", "blank": "_", "bos": "^", "eos": "$",
        "inference": {"noise_scale": 0.0, "length_scale": 1.1, "noise_w": 0.0}}), encoding="utf-8")
    voice = TTSVoice.load(_path(preset), config_path=str(cfg_path))
    voice.dedupe_sentences = True
    hop = voice.session.hparam("hop")
    text = "the quick brown fox. jumps over a lazy dog. hello"
    syn = SynthesisConfig(speaker_id=0, normalize_audio=False)
    plain = list(voice.synthesize(text, syn))
    groups = voice._sentence_groups(text, syn)
    assert len(plain) == len(groups) == 3
    runs = {}
    for batched in (False, True):
        chunks = list(voice.synthesize(text, syn, batch_sentences=batched, alignments=True))
        assert len(chunks) == len(plain)
        for c, p, g in zip(chunks, plain, groups):
            al = c.phoneme_alignments
            assert [(a.phoneme, a.phoneme_ids) for a in al] == [(t, i) for t, i in g]   # one entry per group
            assert sum(a.num_samples for a in al) == len(c.audio_float_array) > 0
            pos = 0
            for a in al:
                assert a.start_sample == pos and a.num_samples % hop == 0
                pos += a.num_samples
            if not batched:
                assert np.array_equal(c.audio_float_array, p.audio_float_array)   # asking for timing changes no sample
        runs[batched] = [[vars(a) for a in c.phoneme_alignments] for c in chunks]
    assert runs[False] == runs[True]                                              # batched and unbatched paths agree
    assert all(c.phoneme_alignments is None for c in plain)
    # synthesize_requests: the same alignments, request by request
    texts = [text, "one more request. with two sentences", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=i % n_spk, length_scale=(1.0, 1.3, 0.8)[i], normalize_audio=False) for i in range(3)]
    got = voice.synthesize_requests(list(zip(texts, cfgs)), max_batch=4, alignments=True)
    for r, (t, c) in enumerate(zip(texts, cfgs)):
        want = list(voice.synthesize(t, c, alignments=True))
        assert len(got[r]) == len(want) > 0
        for a, w in zip(got[r], want):
            assert [vars(x) for x in a.phoneme_alignments] == [vars(x) for x in w.phoneme_alignments], r
            assert sum(x.num_samples for x in a.phoneme_alignments) == len(a.audio_float_array)
    assert all(c.phoneme_alignments is None for req in voice.synthesize_requests(list(zip(texts, cfgs))) for c in req)
    # forced durations / rates as per-utterance lists, padded like the ids
    ids = [[i for _, grp in g for i in grp] for g in groups]
    durs = [[2 + (k % 3) for k in range(len(i))] for i in ids]
    audios, back = voice.phoneme_ids_batch_to_audio(ids, syn, durations=durs, return_durations=True)
    assert [len(a) for a in audios] == [sum(d) * hop for d in durs]
    assert [list(b) for b in back] == durs
    slow = voice.phoneme_ids_batch_to_audio(ids, syn, token_rate=[[2.0] * len(i) for i in ids])
    normal = voice.phoneme_ids_batch_to_audio(ids, syn)
    assert all(len(a) > len(b) for a, b in zip(slow, normal))
    voice.session.close()
