"""The output-rate resampler on the GPU (include/vitsmi.h, "output rate"): the kernel by value, tones, the chunked entry,
and the feature end to end through MiSession and TTSVoice.

Reference: a float64 NumPy evaluation of the definition from its own float64 table (tests/resample_ref.py).  Tolerance,
derived, computed from that table: (K + 2) * 2^-24 * max_p sum_j |h[p][j]| * max|x| - K fused multiply-adds give at most K
roundings of partial sums bounded by sum |h||x|; the table's own rounding and the final store give the other two."""
import json
import math
import os

import numpy as np
import pytest

import resample_ref as ref
from conftest import ALL_PRESETS, GOLDEN, case_get

pytestmark = pytest.mark.gpu

PAIRS = [(22050, 8000), (22050, 48000), (22050, 44100), (16000, 8000)]
B, S = 3, 700
# A row of 37 samples is shorter than every pair's filter (K = 104, 38, 38, 76): each of its outputs sees an edge, and at
# the two downsampling pairs (37 < K / 2) both.  Upsampling has K = 2 ceil(16 / 0.85) = 38 whatever the rates, so there a row
# whose every output sees both edges has at most K / 2 - 1 = 18 samples: test_a_row_shorter_than_half_the_filter.
LENS = np.array([700, 37, 0], np.int64)


def _inputs(lens):
    """name -> x [B, S]; every input carries non-zero garbage behind lens[b], which must not show"""
    rng = np.random.default_rng(2024)
    out = {}
    for name in ("impulse_first", "impulse_last", "noise"):
        x = np.zeros((B, S), np.float32)
        for b, n in enumerate(lens):
            n = int(n)
            if name == "impulse_first" and n:
                x[b, 0] = 1.0
            elif name == "impulse_last" and n:
                x[b, n - 1] = 1.0
            elif name == "noise":
                x[b, :n] = rng.standard_normal(n).astype(np.float32)
            x[b, n:] = 1000.0 + rng.standard_normal(S - n).astype(np.float32)
        out[name] = x
    return out


INPUTS = _inputs(LENS)
_ONE_SHOT = {}


def _one_shot(fi, fo):
    """the noise input through the whole-row entry, once per pair (the pieces tests compare against it)"""
    from phoonnx_amd.session import test_resample
    if (fi, fo) not in _ONE_SHOT:
        _ONE_SHOT[fi, fo] = test_resample(INPUTS["noise"], LENS, fi, fo)
    return _ONE_SHOT[fi, fo]


def _check_rows(y, counts, x, lens, fi, fo, what):
    """y [B, S_out] against the reference on each row's valid samples; exactly 0.0 behind N_b"""
    worst = 0.0
    for b in range(y.shape[0]):
        n, N = int(lens[b]), int(counts[b])
        assert N == math.ceil(n * ref.plan(fi, fo)[0] / ref.plan(fi, fo)[1])
        assert not y[b, N:].any(), (what, b, "samples behind N_b are not exactly 0.0")
        if not N:
            continue
        want = ref.resample64(x[b, :n], fi, fo)
        tol = ref.tolerance(fi, fo, np.abs(x[b, :n]).max())
        err = float(np.abs(y[b, :N].astype(np.float64) - want).max())
        worst = max(worst, err / tol if tol else (0.0 if err == 0 else np.inf))
        print(f"{what} {fi}->{fo} row {b}: n={n} N={N} max|err|={err:.3e} tol={tol:.3e}")
        assert err <= tol, (what, fi, fo, b, err, tol)
    return worst


@pytest.mark.parametrize("fi,fo", PAIRS)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_kernel_by_value(name, fi, fo):
    from phoonnx_amd.session import test_resample
    L, M, K = ref.plan(fi, fo)[:3]
    assert LENS[1] < K and (L > M or LENS[1] < K // 2)
    x = INPUTS[name]
    y, counts = _one_shot(fi, fo) if name == "noise" else test_resample(x, LENS, fi, fo)
    assert y.shape == (B, math.ceil(S * L / M)) and counts[2] == 0 and not np.isnan(y).any()
    _check_rows(y, counts, x, LENS, fi, fo, name)


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_a_row_shorter_than_half_the_filter(fi, fo):
    """lens[1] = K / 2 - 1 (51, 18, 18, 37 samples): the window of every output of that row hangs over both of its edges"""
    from phoonnx_amd.session import test_resample
    L, M, K = ref.plan(fi, fo)[:3]
    lens = np.array([700, K // 2 - 1, 0], np.int64)
    for name, x in sorted(_inputs(lens).items()):
        y, counts = test_resample(x, lens, fi, fo)
        assert y.shape == (B, math.ceil(S * L / M)) and counts[2] == 0 and not np.isnan(y).any()
        _check_rows(y, counts, x, lens, fi, fo, name + "/short")


def _amplitude(y, f_norm):
    """least-squares amplitude of a tone of f_norm cycles per sample in y"""
    n = np.arange(len(y), dtype=np.float64)
    A = np.stack([np.sin(2 * np.pi * f_norm * n), np.cos(2 * np.pi * f_norm * n)], axis=1)
    c, *_ = np.linalg.lstsq(A, y.astype(np.float64), rcond=None)
    return float(np.hypot(*c))


def _tone(fi, fo, f_hz, n=8192):
    from phoonnx_amd.session import test_resample
    x = np.sin(2 * np.pi * f_hz / fi * np.arange(n, dtype=np.float64)).astype(np.float32)[None, :]
    y, counts = test_resample(x, np.array([n], np.int64), fi, fo)
    N = int(counts[0])
    return y[0, N // 4:N - N // 4]      # the middle half


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_a_tone_in_the_pass_band_comes_through_at_amplitude_one(fi, fo):
    f = 0.2 * min(fi, fo)
    mid = _tone(fi, fo, f)
    amp = _amplitude(mid, f / fo)
    print(f"{fi}->{fo}: tone at {f:.0f} Hz, amplitude {amp:.6f}")
    assert abs(amp - 1.0) <= 1e-3


@pytest.mark.parametrize("fi,fo", [(22050, 8000), (22050, 16000)])
def test_a_tone_above_the_output_nyquist_is_removed(fi, fo):
    f = 0.6 * fo
    mid = _tone(fi, fo, f)
    amp = _amplitude(mid, f / fo)      # (the alias sits at 0.4 fo: sin(2 pi 0.6 n) = -sin(2 pi 0.4 n), the same fit)
    print(f"{fi}->{fo}: tone at {f:.0f} Hz, residual amplitude {amp:.3e}, max|y| {float(np.abs(mid).max()):.3e}")
    assert amp < 1e-4


@pytest.mark.parametrize("fi,fo", PAIRS)
@pytest.mark.parametrize("piece", [5, 64, 257, 700])
def test_pieces_equal_the_whole_row_bit_for_bit(piece, fi, fo):
    from phoonnx_amd.session import test_resample_pieces
    want, _ = _one_shot(fi, fo)
    got, ranges = test_resample_pieces(INPUTS["noise"], LENS, fi, fo, piece)
    assert got.shape == want.shape and np.array_equal(got, want)
    pos = 0
    for first, n in ranges:          # contiguous, in order, never empty
        assert first == pos and n > 0
        pos += n
    assert pos == want.shape[1]
    n_pieces = -(-S // piece)
    assert len(ranges) <= n_pieces
    if piece == 5:                   # shorter than the filter's look-ahead: pieces that complete nothing make no delivery
        assert len(ranges) < n_pieces


# ------------------------------------------------------------------ end to end

def _case(preset, c="b3_noise"):
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    return tuple(case_get(g, c, k) for k in ("ids", "lens", "scales", "sid", "noise_dp", "noise_z"))


def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _voice_rate(s):
    return int(s.meta("sample_rate") or 22050)


@pytest.mark.parametrize("tails", ["zero", "reference"])
@pytest.mark.parametrize("preset", ALL_PRESETS)
def test_batch_end_to_end(preset, tails):
    ids, lens, scales, sid, ndp, nz = _case(preset)
    s = _session(preset, tails=tails)
    hop, fi = s.hparam("hop"), _voice_rate(s)
    native = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
    assert "sample_lengths" not in native
    x = native["output"][:, 0, 0, :].copy()
    n_in = native["y_lengths"] * hop
    if tails == "reference" and len(set(n_in.tolist())) > 1:
        assert any(x[b, int(n_in[b]):].any() for b in range(len(n_in)))     # a non-zero native tail: it must be masked
    for fo in (8000, 48000):
        s.set_output_rate(fo)
        r = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
        assert np.array_equal(r["y_lengths"], native["y_lengths"])          # frames stay frames
        assert np.array_equal(r["sample_lengths"], ref.count(n_in, fi, fo))
        assert np.array_equal(s.last_sample_counts(), r["sample_lengths"])
        assert r["output"].shape == (len(lens), 1, 1, int(r["sample_lengths"].max()))
        _check_rows(r["output"][:, 0, 0, :], r["sample_lengths"], x, n_in, fi, fo, f"{preset}/{tails}")
    s.set_output_rate(fi)       # the voice's own rate: the native path
    same = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
    assert "sample_lengths" not in same and np.array_equal(same["output"], native["output"])
    s.set_output_rate(None)
    assert np.array_equal(s.synthesize_batch(ids, lens, scales, sid, ndp, nz)["output"], native["output"])
    s.close()


@pytest.mark.parametrize("fo", [8000, 48000])
@pytest.mark.parametrize("preset", ["tiny_rb1", "sx_rb2_ms"])
def test_streams_equal_the_batch_bit_for_bit(preset, fo):
    ids, lens, scales, sid, ndp, nz = _case(preset)
    s = _session(preset, output_rate=fo)
    want = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)["output"][:, 0, 0, :].copy()
    for chunk_frames in (1, 4):
        parts, pos = [], 0
        for first, samples, total in s.synthesize_stream(ids, lens, scales, sid, chunk_frames=chunk_frames, noise_dp=ndp, noise_z=nz):
            assert first == pos and total == want.shape[1] and samples.shape[1] > 0
            parts.append(samples)
            pos += samples.shape[1]
        assert pos == want.shape[1]
        assert np.array_equal(np.concatenate(parts, axis=1), want), chunk_frames
    s.close()


def test_vocoder_and_vocoder_stream_with_a_rate():
    preset = "tiny_rb1"
    s = _session(preset)
    hop, fi = s.hparam("hop"), _voice_rate(s)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((2, s.hparam("inter"), 23)).astype(np.float32)
    x = s.vocoder(z)[:, 0, 0, :]
    s.set_output_rate(8000)
    y = s.vocoder(z)[:, 0, 0, :]
    N = int(ref.count(23 * hop, fi, 8000))
    assert y.shape == (2, N)
    _check_rows(y, np.array([N, N]), x, np.array([23 * hop] * 2), fi, 8000, "vocoder")
    for chunk_frames in (3, 64):
        got = list(s.vocoder_stream(z, chunk_frames=chunk_frames))
        assert all(total == N for _, _, total in got)
        assert np.array_equal(np.concatenate([smp for _, smp, _ in got], axis=1), y)
    s.close()


@pytest.mark.parametrize("normalize,volume", [(True, 1.0), (False, 2.5)])
def test_device_pcm16_of_the_resampled_waveform(normalize, volume):
    """synthesize_batch_pcm16 with a rate set = the NumPy post-processing of voice.py:271-282 (TTSVoice._postprocess +
    AudioChunk) applied to the same run's resampled float rows."""
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.voice import AudioChunk, TTSVoice
    s = _session("tiny_rb1", output_rate=8000)
    rng = np.random.default_rng(12)
    ids = np.zeros((3, 40), np.int64)
    lens = np.array([40, 21, 9], np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, 200, lens[b])
    scales = np.array([0.0, 1.4, 0.0], np.float32)      # (no noise: the two runs below render the same audio)
    r = s.synthesize_batch(ids, lens, scales)
    pcm, counts = s.synthesize_batch_pcm16(ids, lens, scales, normalize=normalize, volume=volume)
    assert np.array_equal(counts, r["sample_lengths"]) and pcm.shape == (3, int(counts.max())) and pcm.dtype == np.int16
    # ... and of the SAME run: the float rows fetched behind the PCM
    rows = np.empty((3, 1, 1, pcm.shape[1]), np.float32)
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])
    syn = SynthesisConfig(normalize_audio=normalize, volume=volume)
    for b in range(3):
        n = int(counts[b])
        want = AudioChunk(8000, 2, 1, TTSVoice._postprocess(None, rows[b, 0, 0, :n], syn)).audio_int16_array
        assert np.array_equal(pcm[b, :n], want), (b, np.abs(pcm[b, :n].astype(int) - want.astype(int)).max())
        assert not pcm[b, n:].any()
    s.close()


def test_device_pointer_runs_are_refused_with_a_rate_set():
    from phoonnx_amd.session import SessionError
    s = _session("tiny_rb1", output_rate=8000)
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.run_device(0, 0, 1, 4, np.array([0.667, 1.0, 0.8], np.float32))
    s.close()


LETTERS = "abcdefghijklmnopqrstuvwxyz"


def test_voice_writes_the_output_rate(tmp_path):
    import io
    import wave
    from phoonnx_amd import MiSession
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.voice import TTSVoice
    preset = "tiny_rb1"
    path = os.path.join(GOLDEN, preset + ".onnx")
    probe = MiSession(path, host_only=True)
    n_vocab, n_spk, rate = probe.hparam("n_vocab"), probe.hparam("n_speakers"), _voice_rate(probe)
    probe.close()
    id_map = {"_": [0], "^": [1], "$": [2], " ": [3]}
    id_map.update({c: [4 + i % (n_vocab - 4)] for i, c in enumerate(LETTERS)})
    cfg_path = tmp_path / (preset + ".onnx.json")
    cfg_path.write_text(json.dumps({
        "phoneme_type": "graphemes", "lang_code": "en", "audio": {"sample_rate": rate},
        "num_symbols": n_vocab, "num_speakers": n_spk, "phoneme_id_map": id_map,
        "pad": "_", "blank": "_", "bos": "^", "eos": "$",
        "inference": {"noise_scale": 0.0, "length_scale": 1.1, "noise_w": 0.0}}), encoding="utf-8")
    voice = TTSVoice.load(path, config_path=str(cfg_path), output_sample_rate=16000)
    voice.dedupe_sentences = True
    assert voice.session.output_rate == 16000 and voice.session.input_rate == rate
    hop = voice.session.hparam("hop")
    text = "the quick brown fox. jumps over a lazy dog. hello"
    syn = SynthesisConfig(speaker_id=0, normalize_audio=False)
    ids = voice._sentence_ids(text, syn)
    want = []      # sample_lengths, sentence by sentence (a batch of one each, as synthesize renders them)
    for q in ids:
        r = voice.session.synthesize_batch(np.array([q], np.int64), np.array([len(q)], np.int64), voice._scales(syn),
                                           np.zeros(1, np.int64) if n_spk > 1 else None)
        assert np.array_equal(r["sample_lengths"], ref.count(r["y_lengths"] * hop, rate, 16000))
        want.append(int(r["sample_lengths"][0]))
    for kw in ({}, {"batch_sentences": True}, {"device_pcm16": True}):
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            voice.synthesize_wav(text, w, syn_config=syn, **kw)
        with wave.open(io.BytesIO(buf.getvalue())) as rd:
            assert (rd.getframerate(), rd.getsampwidth(), rd.getnchannels()) == (16000, 2, 1), kw
            assert rd.getnframes() == sum(want), kw
    for batched in (False, True):
        chunks = list(voice.synthesize(text, syn, batch_sentences=batched, alignments=True))
        assert [len(c.audio_float_array) for c in chunks] == want
        for c in chunks:
            assert c.sample_rate == 16000
            pos = 0
            for a in c.phoneme_alignments:
                assert a.start_sample == pos
                pos += a.num_samples
            assert pos == len(c.audio_float_array) > 0
    got = voice.synthesize_requests([(text, syn)], alignments=True)[0]
    assert [len(c.audio_float_array) for c in got] == want and all(c.sample_rate == 16000 for c in got)
    assert all(sum(a.num_samples for a in c.phoneme_alignments) == len(c.audio_float_array) for c in got)
    voice.session.close()


def test_the_rate_survives_the_bf16x6_fallback():
    """_fall_back_to_bf16x6 driven directly (no range error is provoked on the device): the reopened handle resamples."""
    from phoonnx_amd.session import RangeError
    ids, lens, scales, sid, ndp, nz = _case("tiny_rb1")
    s = _session("tiny_rb1", output_rate=8000, tails="reference")
    before = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
    s._fall_back_to_bf16x6(RangeError("driven by the test"))
    assert s.gen_precision == "bf16x6" and s.range_fallbacks == 1
    assert s.output_rate == 8000 and s.tails == "reference"
    after = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
    assert np.array_equal(after["sample_lengths"], before["sample_lengths"])
    assert after["output"].shape == before["output"].shape
    np.testing.assert_allclose(after["output"], before["output"], atol=1e-3)     # the two arithmetics' distance (waveform bound)
    s.close()
