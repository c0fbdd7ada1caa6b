"""Per-utterance synthesis settings and noise seeds on the GPU (vits_run_*_rows, MiSession / PipelinedSession with [B, 3]
scales and seeds, TTSVoice.synthesize_requests).  "Interior": every sample of a row but its last gen_rf_frames frames - the
last receptive field keeps the padded batch's semantics (a longer neighbour's frames reach it), as vits_run always had."""
import os

import numpy as np
import pytest

from bench import voice_cache
from conftest import ALL_PRESETS, GOLDEN, case_get
from philox_ref import row_noise

pytestmark = pytest.mark.gpu

TAPS = ("logw", "w_ceil", "z_p", "z")


def _tol(preset):
    return 1e-5 if preset.startswith("tiny") else 2e-5


def _path(preset):
    if preset in ALL_PRESETS:
        return os.path.join(GOLDEN, preset + ".onnx")
    from phoonnx_amd.synth import write_voice
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", preset, seed=1234)
        os.replace(path + ".tmp", path)
    return path


def _interior(out, b, ylen, hop, rf):
    n = max(int(ylen[b]) - rf, 0) * hop
    return out[b, 0, 0, :n]


# (the NumPy restatement of the documented stream, vitsmi.h: tests/philox_ref.py)


def _mixed_rows(B, base):
    """B distinct settings around `base` [noise_scale, length_scale, noise_w]"""
    rows = np.empty((B, 3), np.float32)
    for b in range(B):
        rows[b] = [(0.5, 0.667, 0.0, 0.8)[b % 4], base[1] * (0.8, 1.0, 1.25)[b % 3], (0.6, 0.8, 0.0)[b % 3]]
    return rows


def _batch(rng, B, T, n_vocab, lo=None):
    lens = rng.integers(lo or max(2, T // 3), T + 1, B).astype(np.int64)
    lens[0] = T
    ids = rng.integers(1, n_vocab, (B, T)).astype(np.int64)
    for b in range(B):
        ids[b, lens[b]:] = 0
    return ids, lens


# ------------------------------------------------------------------ 1. equal rows are the legacy run

@pytest.mark.parametrize("preset", ALL_PRESETS)
def test_equal_rows_are_the_legacy_run(preset):
    from phoonnx_amd import MiSession
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    ids, lens, sc, sid, ndp, nz = [case_get(g, "b3_noise", k) for k in ("ids", "lens", "scales", "sid", "noise_dp", "noise_z")]
    B = ids.shape[0]
    s = MiSession(_path(preset))
    a = s.synthesize_batch(ids, lens, sc, sid, ndp, nz, taps=TAPS)
    b = s.synthesize_batch(ids, lens, np.tile(sc, (B, 1)), sid, ndp, nz, taps=TAPS)
    for k in ("output", "y_lengths") + TAPS:
        assert np.array_equal(a[k], b[k]), k
    s.close()
    # the flat seeded stream: two fresh sessions, the same seed, the first call of each form
    outs = []
    for rows in (False, True):
        s = MiSession(_path(preset))
        s.set_seed(1234)
        outs.append(s.synthesize_batch(ids, lens, np.tile(sc, (B, 1)) if rows else sc, sid, taps=("w_ceil", "z")))
        s.close()
    for k in ("output", "y_lengths", "w_ceil", "z"):
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------ 2. each row follows its own settings

@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms", "tiny_dp", "sx_rb1"])
def test_each_row_follows_its_own_settings(preset):
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    s = MiSession(_path(preset))
    o = VitsOracle(_path(preset))
    rng = np.random.default_rng(7)
    B, T = 6, 24
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    sid = (np.arange(B) % s.hparam("n_speakers")).astype(np.int64) if s.hparam("gin") else None
    rows = _mixed_rows(B, [0.667, 1.0, 0.8])
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    F = int(s.synthesize_batch(ids, lens, rows, sid, ndp)["y_lengths"].max())   # (frame counts: noise_dp and the rows only)
    # (the oracle renders the batch under one row's settings for every row: up to 1.25 / 0.8 x the frames)
    nz = rng.standard_normal((B, s.hparam("inter"), 2 * F + 8)).astype(np.float32)
    got = s.synthesize_batch(ids, lens, rows, sid, ndp, nz, taps=("w_ceil",))
    hop, rf = s.hparam("hop"), s.hparam("gen_rf_frames")
    for b in range(B):
        ref = o.infer(ids, lens, rows[b], sid, ndp, nz)
        assert int(got["y_lengths"][b]) == int(ref["y_lengths"][b]), b
        assert np.array_equal(got["w_ceil"][b], ref["w_ceil"][b]), b
        d = np.abs(_interior(got["output"], b, got["y_lengths"], hop, rf) - _interior(ref["output"], b, ref["y_lengths"], hop, rf))
        assert d.size == 0 or float(d.max()) < _tol(preset), (b, float(d.max()))
    s.close()


def test_row_validation_in_the_engine():
    """The C ABI checks every row itself (a caller that is not MiSession): a non-finite value names its row."""
    import ctypes as C
    from phoonnx_amd import MiSession, _ffi
    s = MiSession(_path("tiny_rb1"))
    ids, lens = np.ones((3, 8), np.int64), np.array([8, 5, 3], np.int64)
    rows = np.array([[0.5, 1.0, 0.8], [0.5, 1.0, 0.8], [0.5, np.nan, 0.8]], np.float32)
    rc = s._lib.vits_run_async_rows(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 3, 8, _ffi.ptr(rows), None, C.byref(_ffi.VitsNoise()),
                                    None)
    assert rc == -3 and "row 2" in s._err()
    rows[2, 1] = 1.0
    assert s.synthesize_batch(ids, lens, rows, None)["y_lengths"].shape == (3,)   # the handle is fine afterwards
    s.close()


# ------------------------------------------------------------------ 3. seeded rows do not depend on the batch

@pytest.mark.parametrize("preset", ["sx_rb1", "medium"])
def test_seeded_rows_do_not_depend_on_the_batch(preset):
    from phoonnx_amd import MiSession
    s = MiSession(_path(preset))
    rng = np.random.default_rng(11)
    V, T0 = s.hparam("n_vocab"), 40
    hop, rf = s.hparam("hop"), s.hparam("gen_rf_frames")
    utt = rng.integers(1, V, T0).astype(np.int64)
    mine = np.array([0.667, 1.1, 0.8], np.float32)
    seed = 0xDEADBEEF12345678
    sid = (lambda n: np.zeros(n, np.int64)) if s.hparam("gin") else (lambda n: None)
    # alone
    alone = s.synthesize_batch(utt[None], np.array([T0], np.int64), mine, sid(1), taps=("w_ceil",),
                               seeds=np.array([seed], np.uint64))
    # first in a batch of 8 with a wider T (its neighbours: the bench settings, other seeds)
    T1 = 64
    ids1, lens1 = _batch(rng, 8, T1, V)
    ids1[0] = 0
    ids1[0, :T0], lens1[0] = utt, T0
    rows1 = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (8, 1))
    rows1[0] = mine
    seeds1 = np.arange(100, 108, dtype=np.uint64)
    seeds1[0] = seed
    first = s.synthesize_batch(ids1, lens1, rows1, sid(8), taps=("w_ceil",), seeds=seeds1)
    # last in another batch of 8 whose other rows have other settings
    T2 = 52
    ids2, lens2 = _batch(rng, 8, T2, V)
    ids2[7] = 0
    ids2[7, :T0], lens2[7] = utt, T0
    rows2 = _mixed_rows(8, [0.667, 1.0, 0.8])
    rows2[7] = mine
    seeds2 = np.arange(200, 208, dtype=np.uint64)
    seeds2[7] = seed
    last = s.synthesize_batch(ids2, lens2, rows2, sid(8), taps=("w_ceil",), seeds=seeds2)
    y = int(alone["y_lengths"][0])
    assert int(first["y_lengths"][0]) == y == int(last["y_lengths"][7])
    assert np.array_equal(alone["w_ceil"][0, :T0], first["w_ceil"][0, :T0])
    assert np.array_equal(alone["w_ceil"][0, :T0], last["w_ceil"][7, :T0])
    w0 = _interior(alone["output"], 0, alone["y_lengths"], hop, rf)
    assert w0.size > 0
    for res, b in ((first, 0), (last, 7)):
        d = float(np.abs(_interior(res["output"], b, res["y_lengths"], hop, rf) - w0).max())
        assert d < 2e-5, (b, d)
    # the same call again: bit for bit (the per-handle run counter does not enter a seeded row)
    again = s.synthesize_batch(ids2, lens2, rows2, sid(8), taps=("w_ceil",), seeds=seeds2)
    assert np.array_equal(again["output"], last["output"]) and np.array_equal(again["w_ceil"], last["w_ceil"])
    s.close()


# ------------------------------------------------------------------ 4. the stream is the documented one

@pytest.mark.parametrize("preset", ["tiny_rb1", "sx_rb1"])
def test_seeded_stream_is_the_documented_one(preset):
    from phoonnx_amd import MiSession
    s = MiSession(_path(preset))
    rng = np.random.default_rng(5)
    B, T = 4, 30
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    sid = np.zeros(B, np.int64) if s.hparam("gin") else None
    rows = np.array([[0.667, 1.0, 0.8], [0.5, 1.2, 0.6], [0.667, 0.9, 0.8], [0.3, 1.0, 0.7]], np.float32)
    seeds = np.array([1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0, 42], np.uint64)
    seeded = s.synthesize_batch(ids, lens, rows, sid, taps=("w_ceil", "z"), seeds=seeds)
    C, F = s.hparam("inter"), int(seeded["y_lengths"].max()) + 8
    ndp = np.stack([row_noise(int(sd), 1, 2, T) for sd in seeds])
    nz = np.stack([row_noise(int(sd), 2, C, F) for sd in seeds])
    inj = s.synthesize_batch(ids, lens, rows, sid, ndp, nz, taps=("w_ceil", "z"))
    assert np.array_equal(seeded["w_ceil"], inj["w_ceil"]) and np.array_equal(seeded["y_lengths"], inj["y_lengths"])
    assert float(np.abs(seeded["z"] - inj["z"]).max()) < 1e-5
    assert float(np.abs(seeded["output"] - inj["output"]).max()) < 1e-5
    s.close()


# ------------------------------------------------------------------ 5. chunked rows equal unchunked rows

def test_chunked_rows_equal_unchunked_rows():
    from phoonnx_amd import MiSession
    s = MiSession(_path("sx_rb1"))
    rng = np.random.default_rng(9)
    B, T = 5, 40
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    rows = _mixed_rows(B, [0.667, 1.0, 0.8])
    seeds = np.arange(7, 7 + B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    whole = s.synthesize_batch(ids, lens, rows, None, seeds=seeds)
    S = whole["output"].shape[3]
    got = np.full((B, S), np.nan, np.float32)
    for first, samples, total in s.synthesize_stream(ids, lens, rows, None, chunk_frames=24, seeds=seeds):
        assert total == S
        got[:, first:first + samples.shape[1]] = samples
    assert np.array_equal(s.last_y_lengths(), whole["y_lengths"])
    assert np.array_equal(got, whole["output"][:, 0, 0, :])
    s.close()


# ------------------------------------------------------------------ 6. pipelined equals a single handle

def test_pipelined_rows_equal_a_single_handle():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession
    path = _path("sx_rb1")
    s = MiSession(path)
    rng = np.random.default_rng(13)
    B, T = 7, 36
    ids, lens = _batch(rng, B, T, s.hparam("n_vocab"))
    rows = _mixed_rows(B, [0.667, 1.0, 0.8])
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(1 << 40)
    one = s.synthesize_batch(ids, lens, rows, None, seeds=seeds)
    hop, rf = s.hparam("hop"), s.hparam("gen_rf_frames")
    p = PipelinedSession(s, parts=2)
    two = p.synthesize_batch(ids, lens, rows, None, seeds=seeds)
    assert np.array_equal(one["y_lengths"], two["y_lengths"])
    for b in range(B):
        d = np.abs(_interior(one["output"], b, one["y_lengths"], hop, rf) - _interior(two["output"], b, two["y_lengths"], hop, rf))
        assert d.size == 0 or float(d.max()) < 2e-5, (b, float(d.max()))
    p.close()


# ------------------------------------------------------------------ 7. synthesize_requests matches synthesize

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def test_synthesize_requests_matches_synthesize():
    from phoonnx_amd import MiSession
    from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    s = MiSession(_path("sx_rb2_ms"))
    n_vocab, n_spk = s.hparam("n_vocab"), s.hparam("n_speakers")
    letters = "abcdefghijklmnopqrstuvwxyz "
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate(letters)},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    voice = TTSVoice(session=s, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long. quietly",
             "hello there", "one more request. with two sentences"]
    hop, rf = s.hparam("hop"), s.hparam("gen_rf_frames")

    def cfgs(normalize):
        return [SynthesisConfig(speaker_id=i % n_spk, length_scale=(0.9, 1.0, 1.2, 1.1)[i], noise_scale=0.0,
                                noise_w_scale=0.0, volume=(1.0, 0.5, 0.8, 1.0)[i], normalize_audio=normalize)
                for i in range(len(texts))]

    raw_cfgs = cfgs(False)
    got = voice.synthesize_requests(list(zip(texts, raw_cfgs)), max_batch=4)
    for r, (text, c) in enumerate(zip(texts, raw_cfgs)):
        want = list(voice.synthesize(text, c))
        assert len(got[r]) == len(want) > 0, r
        for a, w in zip(got[r], want):
            assert a.audio_float_array.shape == w.audio_float_array.shape, r
            n = max(len(w.audio_float_array) - rf * hop, 0)
            d = np.abs(a.audio_float_array[:n] - w.audio_float_array[:n])
            assert d.size == 0 or float(d.max()) < 2e-5 * max(c.volume, 1.0), (r, float(d.max()))
    # normalised chunks: _postprocess of the float audio the same rows render (noise off: the same batches, the same bits)
    plain = voice.synthesize_requests([(t, SynthesisConfig(speaker_id=c.speaker_id, length_scale=c.length_scale,
                                                           noise_scale=0.0, noise_w_scale=0.0, normalize_audio=False))
                                       for t, c in zip(texts, raw_cfgs)], max_batch=4)
    norm_cfgs = cfgs(True)
    norm = voice.synthesize_requests(list(zip(texts, norm_cfgs)), max_batch=4)
    for r, c in enumerate(norm_cfgs):
        assert len(norm[r]) == len(plain[r])
        for a, p in zip(norm[r], plain[r]):
            assert np.array_equal(a.audio_float_array, voice._postprocess(p.audio_float_array, c)), r
    s.close()
