"""Fitted durations on the GPU (include/vitsmi.h, "fitted durations"): fit_duration_kernel by value against
tests/fit_ref.py, and fitted runs through the pipeline on the tiny fixture voices.  Every comparison is exact equality: the
definition is integers and IEEE double behind the fp32 weight, and a fitted run is the run with its durations forced."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fit_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODES = {1: "exact", 2: "at_most"}


def _path(preset):
    return os.path.join(GOLDEN, preset + ".onnx")


def _weights(rng, B, T):
    return np.exp(rng.normal(1.0, 1.0, (B, T))).astype(np.float32)


def _free(w, lens, rows):
    return int(sum(np.ceil(ref.clean(w[b, :lens[b]]).astype(np.float64)).sum() for b in rows))


def _kernel_equals_reference(w, lens, groups, targets, modes):
    """the kernel's six outputs against the reference; rows of no group keep the canary.  Returns (durations, scale, frames, status)."""
    from phoonnx_amd.session import Fit, test_fit_durations
    lens, groups = np.asarray(lens, np.int64), np.asarray(groups)
    w_ceil, cum, y_len, scale, frames, status = test_fit_durations(w, lens, Fit(groups, targets, modes))
    dur, rscale, rframes, rstatus = ref.fit(w, lens, groups, targets, modes)
    assert np.array_equal(scale.view(np.uint64), rscale.view(np.uint64)), (scale, rscale)
    assert np.array_equal(frames, rframes) and np.array_equal(status, rstatus), (frames, rframes, status, rstatus)
    fitted = groups >= 0
    want = ref.per_row(dur[fitted], lens[fitted])
    for got, exp in zip((w_ceil, cum, y_len), want):
        assert got.dtype == exp.dtype and np.array_equal(got[fitted], exp)
    for got in (w_ceil, cum, y_len):                                         # the canary: not one element was written
        assert (got[~fitted] == -1).all()
    return dur, scale, frames, status


# ------------------------------------------------------------------ 1. the kernel by value

@pytest.mark.parametrize("T", [1, 256, 257, 513])
def test_one_row_across_the_pass_boundary(T):
    """one row of 1, 256, 257 and 513 tokens: the 256-token pass and the carry of both scans"""
    rng = np.random.default_rng(T)
    w = _weights(rng, 1, T)
    free = _free(w, [T], [0])
    for F in (free, max(1, int(free * 0.5)), int(free * 1.7)):
        dur, _, frames, status = _kernel_equals_reference(w, [T], [0], [F], [1])
        if status[0] == ref.MET:
            assert dur.sum() == F == frames[0]
    # a target equal to the free count: the free durations, token for token
    dur, scale, _, _ = _kernel_equals_reference(w, [T], [0], [free], [1])
    assert np.array_equal(dur[0], np.ceil(w[0].astype(np.float64)).astype(np.int64)) and scale[0] >= 1.0
    # a shorter row inside the same T: nothing behind lens is counted, zeros are written there
    L = max(1, T - 3)
    dur, _, _, _ = _kernel_equals_reference(w, [L], [0], [max(1, _free(w, [L], [0]) - 2)], [1])
    assert not dur[0, L:].any()


def test_groups_of_rows_and_rows_left_alone():
    rng = np.random.default_rng(7)
    B, T = 5, 300
    w = _weights(rng, B, T)
    lens = np.array([300, 41, 120, 0, 257], np.int64)
    groups = [0, 1, -1, 0, 2]                                                # {0, 3}, {1}, {4}; row 2 is not fitted; row 3 is empty
    free = [_free(w, lens, [0, 3]), _free(w, lens, [1]), _free(w, lens, [4])]
    for k in (0.5, 1.0, 1.7):
        targets = [max(1, int(f * k)) for f in free]
        dur, _, frames, status = _kernel_equals_reference(w, lens, groups, targets, [1, 1, 1])
        assert status.tolist() == [ref.MET] * 3 and frames.tolist() == targets
        assert dur[0].sum() == targets[0] and not dur[3].any()
    # all five rows as one group: one multiplier, the extra frames go to the first candidates in (row, t) order
    _kernel_equals_reference(w, lens, [0] * B, [int(_free(w, lens, range(B)) * 0.8)], [1])


def test_a_group_longer_than_the_weights_kept_on_chip():
    """9000 tokens in one group: the last 808 are read from memory at every count, and the boundary falls inside row 2"""
    rng = np.random.default_rng(9)
    B, T = 3, 3000
    w = _weights(rng, B, T)
    free = _free(w, [T] * B, range(B))
    for F in (int(free * 0.8), int(free * 1.25)):
        dur, _, frames, status = _kernel_equals_reference(w, [T] * B, [0] * B, [F], [1])
        assert status[0] == ref.MET and dur.sum() == F


def test_ties_and_cleaned_values():
    T, F = 300, 700                                                          # all weights equal, F no multiple of T
    w = np.full((1, T), 1.3, np.float32)
    dur, _, _, status = _kernel_equals_reference(w, [T], [0], [F], [1])
    assert status[0] == ref.MET and (dur[0] == 3).sum() == F - 2 * T and np.array_equal(dur[0], np.sort(dur[0])[::-1])
    w = np.array([[0.0, -1.5, np.nan, np.inf, -np.inf, 2.0 ** 25, 2.0 ** 24, 3.7, 1e-30, 0.4]], np.float32)
    for F, mode in ((2 ** 22, 1), (2 ** 24, 1), (9, 1), (2 ** 24, 2)):
        dur, _, _, _ = _kernel_equals_reference(w, [10], [0], [F], [mode])
        assert not dur[0, :5].any()


def test_floor_ceiling_and_mode_2():
    rng = np.random.default_rng(3)
    w = _weights(rng, 2, 50)
    lens = [50, 50]
    free = [_free(w, lens, [0]), _free(w, lens, [1])]
    lo = int(ref.terms(ref.clean(w[0]), 2.0 ** -4).sum())
    hi = int(ref.terms(ref.clean(w[0]), 16.0).sum())
    for F0, m0, s0 in ((lo - 1, 1, ref.FLOOR), (hi + 5, 1, ref.CEIL), (hi, 1, ref.MET), (free[0] + 10, 2, ref.KEPT),
                       (free[0] - 10, 2, ref.MET), (lo - 1, 2, ref.FLOOR)):
        # (row 1 runs beside it in mode 2, once kept and once fitted)
        for F1, s1 in ((free[1], ref.KEPT), (free[1] - 1, ref.MET)):
            _, scale, frames, status = _kernel_equals_reference(w, lens, [0, 1], [F0, F1], [m0, 2])
            assert status.tolist() == [s0, s1]
            if s0 == ref.KEPT:
                assert scale[0] == 1.0 and frames[0] == free[0]


# ------------------------------------------------------------------ 2. through the pipeline

def _batch(rng, B, T, n_vocab):
    lens = rng.integers(max(2, T // 3), T + 1, B).astype(np.int64)
    lens[0] = T
    ids = rng.integers(1, n_vocab, (B, T)).astype(np.int64)
    for b in range(B):
        ids[b, lens[b]:] = 0
    return ids, lens


def _setup(preset, seed=21, B=3, T=40):
    from phoonnx_amd import MiSession
    s = MiSession(_path(preset))
    rng = np.random.default_rng(seed)
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    sid = (np.arange(B) % s.hparam("n_speakers")).astype(np.int64) if s.hparam("gin") else None
    rows = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (B, 1))
    rows[:, 1] = (1.0, 1.25, 0.8)[:B] if B <= 3 else 1.0
    seeds = np.arange(3, 3 + B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return s, ids, lens, sid, rows, seeds


def _stream(s, *a, **kw):
    got, seen = None, None
    for first, samples, total in s.synthesize_stream(*a, **kw):
        if got is None:
            got = np.full((samples.shape[0], total), np.nan, np.float32)
            seen = (s.last_durations(), s.last_fit())                        # from the first chunk on
        got[:, first:first + samples.shape[1]] = samples
    return got, seen


@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "tiny_dp"])
def test_a_target_equal_to_the_free_count_is_the_free_run(preset):
    from phoonnx_amd.session import Fit
    s, ids, lens, sid, rows, seeds = _setup(preset)
    B = ids.shape[0]
    free = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, return_durations=True)
    launches = s.stats()["total_launches"]
    per_row = free["durations"].sum(axis=1)
    for fit in (Fit(np.arange(B), per_row), Fit(np.zeros(B, np.int32), [int(per_row.sum())]), Fit([0, -1, 1], per_row[[0, 2]] + 5, "at_most")):
        got = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, return_durations=True, fit=fit)
        assert s.stats()["total_launches"] == launches + 2                   # the weights and the fit: nothing else
        for k in ("durations", "y_lengths", "output"):
            assert np.array_equal(got[k], free[k]), k
        G = len(fit.target_frames)
        kept = fit.modes[0] == 2
        assert got["fit_status"].tolist() == [ref.KEPT if kept else ref.MET] * G
        assert (got["fit_scale"] == 1.0).all() if kept else (got["fit_scale"] >= 1.0).all()
        assert np.array_equal(got["fit_frames"], [free["durations"][fit.groups == g].sum() for g in range(G)])
    s.close()


@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "tiny_dp"])
@pytest.mark.parametrize("k", [0.8, 1.25])
def test_a_fitted_run_is_the_run_with_its_durations_forced(preset, k):
    from phoonnx_amd.session import Fit
    s, ids, lens, sid, rows, seeds = _setup(preset)
    B = ids.shape[0]
    free = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, return_durations=True)
    per_row = free["durations"].sum(axis=1)
    # rows 0 and 2 as one group, row 1 as its own; then three sentences as one group
    for groups, targets in (([0, 1, 0], [int((per_row[0] + per_row[2]) * k), int(per_row[1] * k)]), ([0, 0, 0], [int(per_row.sum() * k)])):
        fit = Fit(groups, targets)
        got = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, return_durations=True, fit=fit, taps=("w", "w_ceil"))
        dur = got["durations"]
        assert got["fit_status"].tolist() == [ref.MET] * len(targets) and got["fit_frames"].tolist() == targets
        assert [int(dur[np.asarray(groups) == g].sum()) for g in range(len(targets))] == targets
        assert np.array_equal(got["y_lengths"], np.maximum(dur.sum(axis=1), 1))
        # ... the reference's plan over the weights the device fitted
        want, scale, frames, status = ref.fit(got["w"], lens, groups, targets, [1] * len(targets))
        assert np.array_equal(dur, want) and np.array_equal(got["w_ceil"].astype(np.int64), want)
        assert np.array_equal(got["fit_scale"].view(np.uint64), scale.view(np.uint64))
        assert np.array_equal(np.ceil(got["w"].astype(np.float64)).astype(np.int64), free["durations"])   # w is what ceilf took
        last = s.last_fit()
        assert np.array_equal(last[0], got["fit_scale"]) and np.array_equal(last[1], frames) and np.array_equal(last[2], status)
        # ... bit for bit the run with those durations forced: seeded noise is a function of seed, channel and frame
        forced = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, durations=dur)
        assert np.array_equal(forced["y_lengths"], got["y_lengths"]) and np.array_equal(forced["output"], got["output"])
        # ... and chunked
        chunks, (sdur, sfit) = _stream(s, ids, lens, rows, sid, chunk_frames=16, seeds=seeds, fit=fit)
        assert np.array_equal(chunks, got["output"][:, 0, 0, :]) and np.array_equal(sdur, dur)
        assert np.array_equal(sfit[0], got["fit_scale"]) and np.array_equal(sfit[2], status)
    s.close()


def test_the_encoded_stream_is_the_delivery_of_the_fitted_run():
    from phoonnx_amd.session import Fit
    s, ids, lens, sid, rows, seeds = _setup("tiny_rb2_ms")
    B = ids.shape[0]
    per_row = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, return_durations=True)["durations"].sum(axis=1)
    fit = Fit([0, 0, 0], [int(per_row.sum() * 0.8)])
    whole = s.synthesize_delivered(ids, lens, rows, sid, seeds=seeds, fit=fit, normalize=False, encoding="pcm16")
    assert whole["fit_status"].tolist() == [ref.MET] and int(whole["y_lengths"].sum()) == fit.target_frames[0]
    joined = [[] for _ in range(B)]
    for c in s.synthesize_stream_encoded(ids, lens, rows, sid, chunk_frames=16, encoding="pcm16", seeds=seeds, fit=fit):
        for b in range(B):
            joined[b].append(c.data[b, int(c.skip[b]):int(c.valid[b])])
    for b in range(B):
        assert np.array_equal(np.concatenate(joined[b]), whole["streams"][b]), b
    s.close()


def test_no_fit_is_the_entry_without_one():
    """fit == NULL, no groups, every row at -1: vits_run_async_ctl's bits and launches"""
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import _controls
    s, ids, lens, sid, rows, seeds = _setup("tiny_rb1")
    B, T = ids.shape
    rate = np.ones((B, T), np.float32)
    rate[:, ::3] = 1.5
    base = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, token_rate=rate)
    launches = s.stats()["total_launches"]
    noise = _ffi.VitsNoise()
    minus = np.full(B, -1, np.int32)
    for fit in (None, _ffi.VitsFit(None, 0, None, None), _ffi.VitsFit(minus.ctypes.data, 0, None, None)):
        ctl = _controls(rows, seeds, None, rate)
        with s._locked():
            rc = s._lib.vits_run_async_fitted(s._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(sid), C.byref(noise), C.byref(ctl),
                                              None if fit is None else C.byref(fit))
            assert rc == 0, s._err()
            out = np.empty_like(base["output"])
            s._fetch(out, 0, B)
        assert np.array_equal(out, base["output"]) and s.stats()["total_launches"] == launches
        assert s._lib.vits_last_fit(s._h, None, None, None, 0) < 0
        with pytest.raises(Exception, match="w is not computed in a run without a fit"):
            s.tap("w")
    s.close()


def test_a_fitted_run_after_reserve_allocates_nothing():
    from phoonnx_amd.session import Fit
    s, ids, lens, sid, rows, seeds = _setup("tiny_rb1")
    B, T = ids.shape
    s.reserve(B, T, 6 * T)
    ws = s.hparam("workspace_bytes")
    got = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, fit=Fit.one_group(B, 3 * T))
    assert got["fit_status"].tolist() == [ref.MET] and int(got["y_lengths"].sum()) == 3 * T
    assert s.hparam("workspace_bytes") == ws
    s.close()


LETTERS = "abcdefghijklmnopqrstuvwxyz"


@pytest.mark.parametrize("out_rate", [None, 16000])
def test_the_voice_fits_a_text_to_seconds(out_rate, tmp_path):
    from phoonnx_amd import MiSession
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.voice import TTSVoice
    preset = "tiny_rb1"
    probe = MiSession(_path(preset), host_only=True)
    n_vocab, n_spk, rate = probe.hparam("n_vocab"), probe.hparam("n_speakers"), int(probe.meta("sample_rate") or 22050)
    probe.close()
    id_map = {"_": [0], "^": [1], "$": [2], " ": [3]}
    id_map.update({c: [4 + i % (n_vocab - 4)] for i, c in enumerate(LETTERS)})
    cfg_path = tmp_path / (preset + ".onnx.json")
    cfg_path.write_text(json.dumps({
        "phoneme_type": "graphemes", "lang_code": "en", "audio": {"sample_rate": rate},
        "num_symbols": n_vocab, "num_speakers": n_spk, "phoneme_id_map": id_map,
        "pad": "_", "blank": "_", "bos": "^", "eos": "$",
        "inference": {"noise_scale": 0.0, "length_scale": 1.0, "noise_w": 0.0}}), encoding="utf-8")
    voice = TTSVoice.load(_path(preset), config_path=str(cfg_path), output_sample_rate=out_rate)
    voice.dedupe_sentences = True
    hop = voice.session.hparam("hop")
    text = "the quick brown fox. jumps over a lazy dog. hello"
    syn = SynthesisConfig(speaker_id=0, normalize_audio=False)
    free = voice.synthesize_encoded(text, syn, sentence_silence=0.01)
    out = voice.sample_rate
    assert free.fit_scale is None
    for k in (0.8, 1.25):
        seconds = k * len(free.data) / out
        got = voice.synthesize_encoded(text, syn, sentence_silence=0.01, duration=seconds)
        assert got.fit_status == ref.MET and (got.fit_scale < 1.0) == (k < 1.0)
        slack = 0.5 * hop * out / rate + (3 if out_rate else 0)              # half a frame; a sample per sentence at an output rate
        print(f"out_rate {out_rate}, k {k}: asked {seconds * out:.1f} samples, delivered {len(got.data)}, slack {slack:.1f}")
        assert abs(len(got.data) - seconds * out) <= slack
        pieces = b"".join(voice.stream_encoded(text, syn, sentence_silence=0.01, duration=seconds, chunk_frames=16))
        assert pieces == got.tobytes()
    # at most: a slot the free text fits into leaves it alone
    kept = voice.synthesize_encoded(text, syn, sentence_silence=0.01, duration=2.0 * len(free.data) / out, duration_mode="at_most")
    assert kept.fit_status == ref.KEPT and kept.fit_scale == 1.0 and kept.tobytes() == free.tobytes()
    voice.session.close()
