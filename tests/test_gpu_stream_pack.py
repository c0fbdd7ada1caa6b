"""Encoded streaming on the GPU (include/vitsmi.h, "encoded streaming"): the kernel by value through vits_test_stream_pack at
the smallest shapes at which cells, row ends and pieces can disagree, then the feature through MiSession and TTSVoice.

Reference: tests/stream_pack_ref.py (over tests/delivery_ref.py) applied to the float waveform of the same run.  Everything is
exact: integer encodings byte for byte, F32 and the peaks bit for bit (the bytes are compared)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import delivery_ref as dref
import stream_pack_ref as ref
from conftest import GOLDEN
from delivery_ref import Seg

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
PIECES = (1, 7, 16, 40)
VOLUMES = (1.0, 0.5, 2.5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ by value

def _small():
    """B = 7 rows of S = 96 with 0, 1, 15, 16, 17, 40 and 96 valid samples, values in (-1.2, 1.2), NaN behind every row's end;
    the volumes cycle over the rows"""
    rng = np.random.default_rng(96)
    counts = np.array([0, 1, 15, 16, 17, 40, 96], np.int64)
    x = rng.uniform(-1.2, 1.2, (7, 96)).astype(np.float32)
    x[6, :4] = [1.0, -1.0, 0.0, -0.0]
    for b in range(7):
        x[b, int(counts[b]):] = np.nan
    return x, counts, np.array([VOLUMES[b % 3] for b in range(7)], np.float32)


def _long():
    """rows of 40 000 samples in pieces of 16 384: several workgroups per row, a last piece that is shorter"""
    rng = np.random.default_rng(40000)
    counts = np.array([40000, 39999, 12345], np.int64)
    x = rng.uniform(-1.1, 1.1, (3, 40000)).astype(np.float32)
    for b in range(3):
        x[b, int(counts[b]):] = np.nan
    return x, counts, np.array([1.0, 0.5, 2.5], np.float32)


SMALL, LONG = _small(), _long()
_WANT = {}


def _want(name, case, piece, encoding, ref_peak=None):
    key = (name, piece, encoding)
    if key not in _WANT:
        x, counts, volume = case
        _WANT[key] = ref.stream_ref(x, counts, ref.pieces(x.shape[1], piece), encoding, ref_peak, volume)
    return _WANT[key]


def _compare(got, want, encoding, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.data.shape == (len(w.data), w.pitch) and g.first_sample == w.first, (what, k)
        assert np.array_equal(g.valid, w.valid), (what, k, g.valid, w.valid)
        for b in range(len(w.data)):
            if g.data[b].tobytes() != w.data[b]:
                bad = np.flatnonzero(g.data[b] != np.frombuffer(w.data[b], np.uint8))
                raise AssertionError(f"{what} piece {k} row {b}: {bad.size} of {w.pitch} bytes differ, first at {bad[:8]}")
            pad = g.data[b].tobytes()[ref.WIDTH[encoding] * int(w.valid[b]):]
            assert pad == ref.SILENCE[encoding] * (len(pad) // ref.WIDTH[encoding]), (what, k, b)
        assert not np.isnan(g.peak).any() and np.array_equal(_bits(g.peak), _bits(w.peak)), (what, k, g.peak, w.peak)
        if encoding == "f32":
            assert not np.isnan(g.data.view(np.float32)).any(), (what, k)


def test_the_small_case_holds_every_situation():
    """What the pieces and counts of the by-value case put in front of the kernel (no GPU work: it guards the case itself)."""
    x, counts, volume = SMALL
    seen = set()
    for enc in ENCODINGS:
        w = ref.WIDTH[enc]
        for piece in PIECES:
            for f, n in ref.pieces(96, piece):
                pitch = ref.pitch_of(n, enc)
                if pitch != w * n:
                    seen.add("pitch beyond the elements")
                for c in counts:
                    v = min(max(int(c) - f, 0), n)
                    if 0 < v < n and (w * v) % 16:
                        seen.add("ends inside a cell")
                    if 0 < v < n and (w * v) % 16 == 0:
                        seen.add("ends on a cell boundary")
                    if c <= f:
                        seen.add("ended before the piece")
                    if c >= f + n:
                        seen.add("ends behind the piece")
    assert seen == {"pitch beyond the elements", "ends inside a cell", "ends on a cell boundary", "ended before the piece",
                    "ends behind the piece"}
    assert set(volume.tolist()) == set(VOLUMES) and np.nanmax(np.abs(x)) > 1.0 and np.nanmin(np.abs(x[x != 0])) > 2e-8


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("piece", PIECES)
def test_kernel_by_value(piece, encoding):
    from phoonnx_amd.session import test_stream_pack
    x, counts, volume = SMALL
    got = test_stream_pack(x, counts, piece, encoding, volume=volume)
    _compare(got, _want("small", SMALL, piece, encoding), encoding, f"{encoding}/{piece}")
    # the running peaks are the NumPy maxima, piece by piece
    for g in got:
        n = np.minimum(counts, min(96, g.first_sample + piece))
        want = np.array([np.max(np.abs(x[b, :int(n[b])])) if n[b] else 0 for b in range(7)], np.float32)
        assert np.array_equal(_bits(g.peak), _bits(want))


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_reference_peaks_on_either_side_of_the_threshold(encoding):
    """`ref_peak < 1e-8f ? 0 : v / ref_peak` from both sides: 1e-9 gives silence, 2e-8 full scale (every |x| above 2e-8 clips);
    and a row's own peak gives the normalised delivery"""
    from phoonnx_amd.session import test_stream_pack
    x, counts, volume = SMALL
    own = np.array([np.max(np.abs(x[b, :int(counts[b])])) if counts[b] else 0 for b in range(7)], np.float32)
    peaks = np.array([1e-9, 2e-8, 1e-9, 2e-8, 1e-9, 2e-8, 1e-9], np.float32)
    w = ref.WIDTH[encoding]
    for piece in (7, 40):
        got = test_stream_pack(x, counts, piece, encoding, ref_peak=peaks, volume=volume)
        _compare(got, ref.stream_ref(x, counts, ref.pieces(96, piece), encoding, peaks, volume), encoding, f"{encoding}/{piece}/threshold")
        full = {"pcm16": {32767, -32767}, "f32": {1.0, -1.0}, "ulaw": {0x80, 0x00}, "alaw": {0xAA, 0x2A}}[encoding]
        for b in range(1, 7):
            row = np.frombuffer(b"".join(g.data[b].tobytes()[:w * int(g.valid[b])] for g in got), ref.DTYPE[encoding])
            assert len(row) == counts[b]
            if peaks[b] < 1e-8:
                assert row.tobytes() == ref.SILENCE[encoding] * int(counts[b]), b
            elif volume[b] == 1.0:
                assert set(row.tolist()) <= full, b
        got = test_stream_pack(x, counts, piece, encoding, ref_peak=own, volume=volume)
        want = dref.deliver_ref(x, counts, [Seg(b, b, 0, 1, volume[b]) for b in range(7)], 7, encoding)
        for b in range(7):
            assert b"".join(g.data[b].tobytes()[:w * int(g.valid[b])] for g in got) == want[b], b


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_kernel_by_value_over_several_workgroups(encoding):
    from phoonnx_amd.session import test_stream_pack
    x, counts, volume = LONG
    got = test_stream_pack(x, counts, 16384, encoding, volume=volume)
    assert [g.data.shape[1] for g in got] == [ref.pitch_of(n, encoding) for n in (16384, 16384, 40000 - 32768)]
    _compare(got, _want("long", LONG, 16384, encoding), encoding, f"{encoding}/long")


# ------------------------------------------------------------------ through a session

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _batch(s, seed=12):
    """B = 3 rows of 40, 21 and 9 ids, with per-row seeds (and speakers, where the voice has them)"""
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64)


VOL3 = np.array([1.0, 0.5, 2.5], np.float32)


def _rows_of(r, s):
    counts = np.asarray(r["sample_lengths"] if "sample_lengths" in r else r["y_lengths"] * s.hparam("hop"), np.int64)
    return r["output"][:, 0, 0, :].copy(), counts


def _joined(chunks, b):
    return b"".join(c.data[b, :int(c.valid[b])].tobytes() for c in chunks)


def _delivered(x, counts, normalize, encoding, volume=VOL3):
    B = len(counts)
    return dref.deliver_ref(x, counts, [Seg(b, b, 0, normalize, volume[b]) for b in range(B)], B, encoding)


def _check_stream(chunks, x, counts, encoding, normalize, ranges=None, volume=VOL3):
    """chunks of an encoded stream against the rows x / counts of the whole run: layout, valid, joined bytes, final peak"""
    B, total = len(counts), int(counts.max())
    assert chunks and chunks[0].first_sample == 0
    pos = 0
    for c in chunks:
        n = c.data.shape[1]
        assert c.first_sample == pos and c.total_samples == total and c.data.dtype == np.dtype(ref.DTYPE[encoding]) and n > 0
        assert np.array_equal(c.valid, np.clip(counts - pos, 0, n))
        for b in range(B):   # silence behind the row's end, inside the chunk
            assert c.data[b, int(c.valid[b]):].tobytes() == ref.SILENCE[encoding] * (n - int(c.valid[b]))
        pos += n
    assert pos == total
    if ranges is not None:
        assert [(c.first_sample, c.data.shape[1]) for c in chunks] == ranges
    want = _delivered(x, counts, normalize, encoding, volume)
    for b in range(B):
        assert _joined(chunks, b) == want[b], (encoding, normalize, b)
    own = np.array([np.max(np.abs(x[b, :int(counts[b])])) for b in range(B)], np.float32)
    assert np.array_equal(_bits(chunks[-1].peak), _bits(own))
    peaks = np.stack([c.peak for c in chunks])
    assert (np.diff(peaks, axis=0) >= 0).all()
    return own


_RUNS = {}


def _reference_run(preset, **kw):
    """one whole-batch run per preset and rate: the fp32 rows every stream of that preset is compared with"""
    key = (preset, tuple(sorted(kw.items())))
    if key not in _RUNS:
        s = _session(preset, **kw)
        ids, lens, scales, sid, seeds = _batch(s)
        r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
        _RUNS[key] = _rows_of(r, s) + (np.asarray(r["y_lengths"], np.int64),)
        s.close()
    return _RUNS[key]


@pytest.mark.parametrize("chunk_frames", [1, 3, 64])
@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_stream_of_a_run(preset, chunk_frames):
    x, counts, ylen = _reference_run(preset)
    assert len(set(counts.tolist())) == 3
    if chunk_frames == 64:
        assert any(int(f) % 64 for f in ylen if f < ylen.max()), "no row ends strictly inside a chunk"
    s = _session(preset)
    ids, lens, scales, sid, seeds = _batch(s)
    # the fp32 stream of the same run: its chunk ranges, and its valid samples encoded by the reference
    plain = list(s.synthesize_stream(ids, lens, scales, sid, chunk_frames=chunk_frames, seeds=seeds))
    ranges = [(f, a.shape[1]) for f, a, _ in plain]
    xs = np.concatenate([a for _, a, _ in plain], axis=1)
    own = None
    for enc in ENCODINGS:
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  seeds=seeds))
        own = _check_stream(chunks, x, counts, enc, 0, ranges)
        assert [_joined(chunks, b) for b in range(3)] == _delivered(xs, counts, 0, enc)
        assert np.array_equal(s.last_y_lengths(), ylen) and np.array_equal(s.last_sample_counts(), counts)
    # a second stream normalised by the reported peaks is the normalised delivery
    enc = ENCODINGS[chunk_frames % 4]
    chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                              ref_peak=own, seeds=seeds))
    _check_stream(chunks, x, counts, enc, 1, ranges)
    s.close()


@pytest.mark.parametrize("chunk_frames", [1, 5])
def test_stream_at_an_output_rate(chunk_frames):
    x, counts, ylen = _reference_run("tiny_rb1", output_rate=8000)
    s = _session("tiny_rb1", output_rate=8000)
    ids, lens, scales, sid, seeds = _batch(s)
    plain = list(s.synthesize_stream(ids, lens, scales, sid, chunk_frames=chunk_frames, seeds=seeds))
    ranges = [(f, a.shape[1]) for f, a, _ in plain]
    xs = np.concatenate([a for _, a, _ in plain], axis=1)
    assert xs.shape[1] == counts.max() and len(set(counts.tolist())) == 3
    for enc in ("ulaw", "alaw"):
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  seeds=seeds))
        own = _check_stream(chunks, x, counts, enc, 0, ranges)
        assert [_joined(chunks, b) for b in range(3)] == _delivered(xs, counts, 0, enc)
        assert np.array_equal(s.last_sample_counts(), counts)
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  ref_peak=own, seeds=seeds))
        _check_stream(chunks, x, counts, enc, 1, ranges)
    s.close()


def test_vocoder_stream_encoded():
    s = _session("tiny_rb1")
    hop, F = s.hparam("hop"), 23
    z = np.random.default_rng(5).standard_normal((2, s.hparam("inter"), F)).astype(np.float32)
    vol = np.array([0.5, 2.5], np.float32)
    for rate in (None, 8000):
        s.set_output_rate(rate)
        x = s.vocoder(z)[:, 0, 0, :]
        n = x.shape[1]
        counts = np.array([n, n], np.int64)
        for chunk_frames in (37, 4):
            ranges = [(f, a.shape[1]) for f, a, _ in s.vocoder_stream(z, chunk_frames=chunk_frames)]
            assert (len(ranges) == 1) == (chunk_frames == 37)
            for enc in ("pcm16", "f32"):
                chunks = list(s.vocoder_stream_encoded(z, chunk_frames=chunk_frames, encoding=enc, volume=vol))
                own = _check_stream(chunks, x, counts, enc, 0, ranges, vol)
                chunks = list(s.vocoder_stream_encoded(z, chunk_frames=chunk_frames, encoding=enc, volume=vol, ref_peak=own))
                _check_stream(chunks, x, counts, enc, 1, ranges, vol)
    s.close()


def test_a_refusal_leaves_the_run_and_a_stream_leaves_none():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import Segment, SessionError
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = _rows_of(r, s)
    segs = [Segment(b, b, 0, 1, float(VOL3[b])) for b in range(3)]
    # refused by the session's own checks, and by the engine's (the C ABI called directly): no callback, the run stays
    for kw in (dict(encoding="mp3"), dict(volume=[1.0, float("nan"), 1.0]), dict(ref_peak=[0.5, 0.5, -1.0])):
        with pytest.raises(SessionError):
            s.synthesize_stream_encoded(ids, lens, scales, sid, seeds=seeds, **kw)
    calls = []

    @_ffi.ENC_CHUNK_FN
    def cb(*args):
        calls.append(args)
        return 0

    rows = np.ascontiguousarray(scales)
    ctl = _ffi.VitsControls()
    ctl.scales_rows, ctl.seeds = rows.ctypes.data, seeds.ctypes.data
    noise = _ffi.VitsNoise()
    bad = np.array([1.0, np.inf, 1.0], np.float32)
    for enc, pk, vol, word in ((5, None, None, "unknown encoding 5"), (0, None, bad, "volume[1]"), (1, bad, None, "ref_peak[1]")):
        fmt = _ffi.VitsStreamFormat()
        fmt.encoding = enc
        fmt.ref_peak = None if pk is None else pk.ctypes.data
        fmt.volume = None if vol is None else vol.ctypes.data
        rc = s._lib.vits_run_chunked_enc(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 3, 40, _ffi.ptr(sid), C.byref(noise), C.byref(ctl),
                                         C.byref(fmt), 4, cb, None)
        assert rc == -3 and word in s._err(), (rc, s._err())
    assert calls == []
    for enc in ("ulaw", "f32"):
        got = [np.ascontiguousarray(a).tobytes() for a in s.deliver(segs, 3, enc)]
        assert got == _delivered(x, counts, 1, enc), enc
    # after an encoded stream there is no whole waveform to deliver
    chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=16, encoding="alaw", volume=VOL3, seeds=seeds))
    _check_stream(chunks, x, counts, "alaw", 0)
    with pytest.raises(SessionError, match="no completed run"):
        s.deliver(segs, 3, "pcm16")
    s.close()


def test_closing_the_generator_ends_the_run():
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds = _batch(s)
    x, counts, ylen = _reference_run("tiny_rb1")
    before = threading.active_count()
    gen = s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=1, encoding="ulaw", seeds=seeds)
    first = next(gen)
    assert first.first_sample == 0 and first.data.shape == (3, s.hparam("hop")) and first.total_samples == counts.max()
    gen.close()
    assert threading.active_count() == before      # the worker has been joined: the engine stopped after the chunk in flight
    # the session is free again, and the next run is a whole one
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    assert np.array_equal(r["output"][:, 0, 0, :], x)
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_a_reservation_covers_the_stream(rate):
    """The recipe of test_a_reservation_covers_the_delivery: forced durations of 120 frames per id make the rows long enough for
    the stream's chunk buffer to need room of its own; a reservation that left it out would grow here."""
    s = _session("tiny_rb1", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 120, 0).astype(np.int64)
    F = 40 * 120
    s.reserve(3, 40, F)
    cap = s.hparam("workspace_bytes")
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=dur)
    assert int(r["y_lengths"].max()) == F and s.hparam("workspace_bytes") == cap
    x, counts = _rows_of(r, s)
    for enc, chunk_frames in (("f32", F), ("pcm16", 1024), ("ulaw", 64)):
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  seeds=seeds, durations=dur))
        assert s.hparam("workspace_bytes") == cap, (enc, "an encoded stream allocated behind a reservation that covers the request")
        _check_stream(chunks, x, counts, enc, 0)
    s.close()


# ------------------------------------------------------------------ the voice layer

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(preset):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    s = _session(preset)
    n_vocab, n_spk = s.hparam("n_vocab"), s.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=s, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


TEXT = "the quick brown fox. jumps over. a lazy dog"


@pytest.mark.parametrize("encoding", ["pcm16", "ulaw"])
def test_stream_encoded_equals_synthesize_encoded(encoding):
    from phoonnx_amd.config import SynthesisConfig
    voice = _voice("tiny_rb2_ms")
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=False)
    for silence, chunk_frames in ((0.0, 64), (0.05, 7)):
        want = voice.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=silence)
        assert len(want.sentence_samples) == 3
        got = list(voice.stream_encoded(TEXT, cfg, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=silence))
        assert b"".join(got) == want.tobytes(), (silence, chunk_frames)
        # sentence 0 goes out chunk by chunk (behind its pause), the later ones once their predecessor is complete
        n0 = want.sentence_samples[0]
        assert n0 == max(want.sentence_samples) and all(got)
        assert len(got) == (1 if silence else 0) + -(-n0 // (chunk_frames * voice.session.hparam("hop"))) + 2, (silence, chunk_frames)
        if chunk_frames == 7:
            assert len(got) > 4
    with pytest.raises(ValueError, match="cannot know its own peak"):
        voice.stream_encoded(TEXT, SynthesisConfig(speaker_id=1), encoding=encoding)
    voice.session.close()
