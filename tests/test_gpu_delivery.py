"""Delivery on the GPU (include/vitsmi.h, "delivery"): the packer by value through vits_test_deliver at the smallest shapes at
which it can go wrong, then the feature through MiSession and TTSVoice.

Reference: tests/delivery_ref.py applied to the float waveform of the same run.  Everything is exact: integer encodings byte
for byte, F32 bit for bit (the bytes are compared)."""
import os

import numpy as np
import pytest

import delivery_ref as ref
from conftest import GOLDEN
from delivery_ref import Seg

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")


def _segments(segs):
    from phoonnx_amd.session import Segment
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _bytes(streams):
    return [np.ascontiguousarray(a).tobytes() for a in streams]


# ------------------------------------------------------------------ by value

def _dense():
    """B = 24 rows of up to 91 samples (one empty), 22 of them in a permuted order over 3 streams; leads, normalisation and
    volume cycle, each with its own period, so that every stream sees every volume; NaN behind every row's end.  The row at
    1e-9 is normalised by its own peak whatever the permutation: its segment's mode is pinned to 1."""
    B, S = 24, 96
    rng = np.random.default_rng(96)
    counts = np.array([(7 * b) % 97 for b in range(B)], np.int64)
    assert counts.min() == 0 and counts.max() == 91
    x = rng.uniform(-1.2, 1.2, (B, S)).astype(np.float32)
    x[3, :4] = [1.0, -1.0, 0.0, -0.0]
    x[5, :int(counts[5])] = np.float32(1e-9) * rng.choice([-1.0, 1.0], int(counts[5])).astype(np.float32)   # peak < 1e-8
    for b in range(B):
        x[b, int(counts[b]):] = np.nan
    order = [int(r) for r in rng.permutation(B) if r not in (10, 17)]     # (22 rows; the empty, the tiny and the exact one take part)
    segs = [Seg(int(r), g % 3, (0, 1, 3, 16)[g % 4], 1 if r == 5 else (0, 1, 2)[(g // 3) % 3], (1.0, 0.5, 2.5)[(g + g // 3) % 3])
            for g, r in enumerate(order)]
    assert [s.normalize for s in segs if s.row == 5] == [1]
    for j in range(3):
        assert {s.volume for s in segs if s.stream == j} == {1.0, 0.5, 2.5} and {s.normalize for s in segs if s.stream == j} == {0, 1, 2}
    return x, counts, segs, 3


TINY, ABOVE = np.float32(1e-9), np.float32(2e-8)      # peaks on either side of the 1e-8 threshold


def _threshold():
    """`peak < 1e-8f ? 0 : v / peak` from both sides and in both scopes: rows at 1e-9 normalised by their own peak (1) and
    alone in a stream by the stream's (2) must come out as silence; a row at 2e-8 must come out at full scale; and a row at
    1e-9 that shares a normalize-2 stream with a loud row is divided by THAT peak, not zeroed by its own."""
    rng = np.random.default_rng(8)
    counts = np.array([37, 21, 30, 19, 26], np.int64)
    sign = rng.choice([-1.0, 1.0], (5, 40)).astype(np.float32)
    x = sign * TINY
    x[2] = rng.uniform(-0.9, 0.9, 40).astype(np.float32)
    x[4] = sign[4] * ABOVE
    for b in range(5):
        x[b, int(counts[b]):] = np.nan
    segs = [Seg(0, 0, 0, 2, 1.0),                              # alone in its stream, stream scope: silence
            Seg(1, 1, 3, 2, 2.5), Seg(2, 1, 0, 2, 2.5),        # with a loud row, stream scope: 1e-9 / peak(row 2) * 2.5
            Seg(3, 2, 1, 1, 2.5),                              # its own peak: silence, whatever the volume
            Seg(4, 3, 0, 1, 1.0)]                              # just above the threshold: +-1
    return x, counts, segs, 4


def _long():
    """rows of 40 000 samples: several workgroups per segment, and an odd start behind the row of 39 999"""
    rng = np.random.default_rng(40000)
    counts = np.array([40000, 39999, 12345], np.int64)
    x = rng.uniform(-1.1, 1.1, (3, 40000)).astype(np.float32)
    for b in range(3):
        x[b, int(counts[b]):] = np.nan
    return x, counts, [Seg(1, 0, 0, 2, 1.0), Seg(0, 0, 0, 2, 0.5), Seg(2, 1, 7, 1, 2.5)], 2


CASES = {"dense": _dense(), "long": _long(), "threshold": _threshold()}
_WANT = {}


def _want(case, encoding):
    if (case, encoding) not in _WANT:
        _WANT[case, encoding] = ref.deliver_ref(*CASES[case], encoding)
    return _WANT[case, encoding]


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_packer_by_value(case, encoding):
    from phoonnx_amd.session import test_deliver
    x, counts, segs, J = CASES[case]
    want = _want(case, encoding)
    if case == "dense":
        # many segments start at odd packed offsets, and several fit inside one 16-byte cell
        starts = np.cumsum([0] + [int(counts[s.row]) for j in range(J) for s in segs if s.stream == j])
        assert sum(int(v) % 2 for v in starts) >= 5 and sum(1 for s in segs if 0 < counts[s.row] < 8) >= 2
    got = _bytes(test_deliver(x, counts, _segments(segs), J, encoding))
    assert [len(g) for g in got] == [len(w) for w in want]
    for j in range(J):
        if got[j] != want[j]:
            a, b = np.frombuffer(got[j], np.uint8), np.frombuffer(want[j], np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{case}/{encoding} stream {j}: {bad.size} of {a.size} bytes differ, first at {bad[:8]}")


def _pieces(case, encoding):
    """the reference's bytes of a case, cut into {row: its audio's bytes}"""
    x, counts, segs, J = CASES[case]
    w, out = ref.WIDTH[encoding], {}
    for j, stream in enumerate(_want(case, encoding)):
        pos = 0
        for s in (s for s in segs if s.stream == j):
            pos += w * int(s.lead_samples)
            out[s.row] = stream[pos:pos + w * int(counts[s.row])]
            pos += w * int(counts[s.row])
        assert pos == len(stream)
    return out


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_cases_reach_the_peak_threshold(encoding):
    """What the reference says of the rows the by-value cases carry for the 1e-8 threshold: the comparison above then holds the
    kernel to it (no GPU work here; it guards the cases themselves)."""
    x, counts, segs, J = CASES["dense"]
    assert np.abs(x[5, :int(counts[5])]).max() == TINY and counts[5] > 0
    assert _pieces("dense", encoding)[5] == ref.SILENCE[encoding] * int(counts[5])
    x, counts, segs, J = CASES["threshold"]
    got = _pieces("threshold", encoding)
    for row in (0, 3):
        assert got[row] == ref.SILENCE[encoding] * int(counts[row]), row
    assert got[1] != ref.SILENCE[encoding] * int(counts[1]) or encoding != "f32"      # (1e-9 / 0.9 * 2.5: non-zero as a float)
    full = np.frombuffer(got[4], ref.DTYPE[encoding])
    want = {"pcm16": {32767, -32767}, "f32": {1.0, -1.0}, "ulaw": {0x80, 0x00}, "alaw": {0xAA, 0x2A}}[encoding]
    assert set(full.tolist()) == want


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_degenerate_plans(encoding):
    from phoonnx_amd.session import test_deliver
    x, counts = CASES["dense"][:2]
    assert _bytes(test_deliver(x, counts, [], 2, encoding)) == [b"", b""]
    assert counts[0] == 0
    for lead in (0, 5):
        segs = [Seg(0, 1, lead, 1, 2.0)]
        got = _bytes(test_deliver(x, counts, _segments(segs), 2, encoding))
        assert got == ref.deliver_ref(x, counts, segs, 2, encoding) == [b"", ref.SILENCE[encoding] * lead]


def _canary():
    return np.full(4096, 0xA5, np.uint8)


@pytest.mark.parametrize("name", sorted(ref.REFUSALS))
def test_refusals_write_nothing(name):
    from phoonnx_amd.session import SessionError, test_deliver
    segs, J, enc, index, word = ref.REFUSALS[name]
    x = np.ones((6, 16), np.float32)
    dst = _canary()
    with pytest.raises(SessionError, match=r"\[-3\]") as exc:
        test_deliver(x, ref.COUNTS, _segments(segs), J, enc, dst=dst)
    assert word in str(exc.value) and (index is None or f"segment {index}:" in str(exc.value))
    assert (dst == 0xA5).all()


def test_a_short_buffer_and_an_unknown_encoding_are_refused():
    import ctypes as C
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import SessionError, test_deliver
    x = np.ones((6, 16), np.float32)
    good = _segments(ref.GOOD)
    need = int(ref.plan_ref(ref.COUNTS, ref.GOOD, 2, "pcm16")[2])
    dst = _canary()
    with pytest.raises(SessionError, match=f"{need} needed"):
        test_deliver(x, ref.COUNTS, good, 2, "pcm16", dst=dst[:need - 1])
    assert (dst == 0xA5).all()
    arr = (_ffi.VitsSegment * 3)(*[_ffi.VitsSegment(s.row, s.stream, s.lead_samples, s.normalize, s.volume) for s in good])
    rc = _ffi.load().vits_test_deliver(0, _ffi.ptr(x), _ffi.ptr(ref.COUNTS), 6, 16, arr, 3, 2, 7, _ffi.ptr(dst), dst.nbytes, None, None)
    assert rc == -3 and "unknown encoding 7" in _ffi.last_error(None) and (dst == 0xA5).all()
    # ... and the same buffer, exactly large enough, is filled
    got = test_deliver(x, ref.COUNTS, good, 2, "pcm16", dst=dst[:need])
    assert _bytes(got) == ref.deliver_ref(x, ref.COUNTS, ref.GOOD, 2, "pcm16") and (dst[need:] == 0xA5).all()


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


def _plans(B):
    return {"one row per stream": ([Seg(b, b, 0, 1, 1.0) for b in range(B)], B),
            "two streams, leads, stream peak": ([Seg(2, 0, 11, 2, 0.5), Seg(0, 0, 0, 2, 0.5), Seg(1, 1, 3, 0, 2.5)], 2),
            "one row of three": ([Seg(1, 0, 0, 1, 1.0)], 1)}


def _rows_of(r, s):
    counts = np.asarray(r["sample_lengths"] if "sample_lengths" in r else r["y_lengths"] * s.hparam("hop"), np.int64)
    return r["output"][:, 0, 0, :].copy(), counts


@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_delivery_of_a_run(preset):
    s = _session(preset)
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = _rows_of(r, s)
    assert len(set(counts.tolist())) == 3
    for name, (segs, J) in _plans(3).items():
        for enc in ENCODINGS:
            got = s.deliver(_segments(segs), J, enc)
            assert [g.dtype for g in got] == [np.dtype(ref.DTYPE[enc])] * J
            assert _bytes(got) == ref.deliver_ref(x, counts, segs, J, enc), (name, enc)
    # PCM16, one row per stream = the rows of last_pcm16 cut to their lengths
    pcm = s.last_pcm16(True, 1.0, shape=x.shape)
    one = s.deliver(_segments(_plans(3)["one row per stream"][0]), None, "pcm16")
    for b in range(3):
        assert np.array_equal(one[b], pcm[b, :int(counts[b])]) and not pcm[b, int(counts[b]):].any()
    # after the deliveries the run is still there: taps, the float rows
    z = s.tap("z")
    assert z.shape[0] == 3 and np.isfinite(z).all()
    rows = np.empty_like(r["output"])
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])
    # run and delivery in one call, the same seeds: the same bytes
    segs, J = _plans(3)["two streams, leads, stream peak"]
    for enc in ENCODINGS:
        d = s.synthesize_delivered(ids, lens, scales, sid, segments=_segments(segs), n_streams=J, encoding=enc, seeds=seeds,
                                   return_durations=True)
        assert _bytes(d["streams"]) == ref.deliver_ref(x, counts, segs, J, enc), enc
        assert np.array_equal(d["y_lengths"], r["y_lengths"]) and np.array_equal(d["sample_lengths"], counts)
        assert np.array_equal(d["stream_samples"], ref.plan_ref(counts, segs, J, enc)[0]) and d["durations"].shape == ids.shape
    # the default plan: one stream per row, normalize / volume per row
    d = s.synthesize_delivered(ids, lens, scales, sid, seeds=seeds, normalize=[True, False, True], volume=[1.0, 2.5, 0.5])
    want = ref.deliver_ref(x, counts, [Seg(0, 0, 0, 1, 1.0), Seg(1, 1, 0, 0, 2.5), Seg(2, 2, 0, 1, 0.5)], 3, "pcm16")
    assert _bytes(d["streams"]) == want
    s.close()


def test_delivery_at_an_output_rate():
    s = _session("tiny_rb1", output_rate=8000)
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = _rows_of(r, s)
    assert "sample_lengths" in r and np.array_equal(s.last_sample_counts(), counts)
    for name, (segs, J) in _plans(3).items():
        for enc in ("ulaw", "alaw"):
            assert _bytes(s.deliver(_segments(segs), J, enc)) == ref.deliver_ref(x, counts, segs, J, enc), (name, enc)
    rows = np.empty_like(r["output"])
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])        # delivering did not move what it delivered
    s.close()


def test_delivery_after_the_vocoder():
    s = _session("tiny_rb1")
    hop, F = s.hparam("hop"), 23
    z = np.random.default_rng(5).standard_normal((2, s.hparam("inter"), F)).astype(np.float32)
    segs = [Seg(1, 0, 2, 1, 1.0), Seg(0, 0, 0, 0, 0.5)]
    for rate in (None, 8000):
        s.set_output_rate(rate)
        x = s.vocoder(z)[:, 0, 0, :]
        n = x.shape[1]
        assert n == (F * hop if rate is None else -(-F * hop * 8000 // int(s.meta("sample_rate") or 22050)))
        for enc in ENCODINGS:
            got = s.deliver(_segments(segs), 1, enc)
            assert len(got[0]) == 2 * n + 2 and _bytes(got) == ref.deliver_ref(x, [n, n], segs, 1, enc), (rate, enc)
    s.close()


def test_no_run_and_a_bad_plan():
    from phoonnx_amd.session import SessionError
    s = _session("tiny_rb1")
    good = _segments([Seg(0, 0, 0, 1, 1.0)])
    with pytest.raises(SessionError, match="no completed run"):
        s.deliver(good, 1, "pcm16")
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = _rows_of(r, s)
    bad = {"segment 0: row 3 outside": ([Seg(3, 0, 0, 1, 1.0)], 1), "segment 1: row 2 is already": ([Seg(2, 0, 0, 1, 1.0)] * 2, 1),
           "segment 1: stream 2 outside": ([Seg(0, 0, 0, 1, 1.0), Seg(1, 2, 0, 1, 1.0)], 2), "n_streams = 4": ([], 4),
           "segment 0: normalize 3": ([Seg(0, 0, 0, 3, 1.0)], 1), "segment 0: volume": ([Seg(0, 0, 0, 1, float("nan"))], 1),
           "segment 0: lead_samples -1": ([Seg(0, 0, -1, 1, 1.0)], 1), "n_segs = 4": ([Seg(b % 3, 0, 0, 1, 1.0) for b in range(4)], 1)}
    for word, (segs, J) in bad.items():
        with pytest.raises(SessionError, match=word):
            s.deliver(_segments(segs), J, "pcm16")
    with pytest.raises(SessionError, match="unknown encoding"):
        s.deliver(good, 1, "mp3")
    # a rejected plan leaves the run deliverable
    assert _bytes(s.deliver(good, 1, "ulaw")) == ref.deliver_ref(x, counts, [Seg(0, 0, 0, 1, 1.0)], 1, "ulaw")
    s.reserve(8, 64, 4 * int(r["y_lengths"].max()))      # grows the workspaces: the run's results are gone
    with pytest.raises(SessionError, match="no completed run"):
        s.deliver(good, 1, "pcm16")
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_a_reservation_covers_the_delivery(rate):
    """Forced durations of 120 frames per id make the rows long enough for the delivery's buffers to exceed what the staging
    slab holds without them (the 16-bit waveform, or the resampled waveform with its 16-bit rendering, plus the MiB every
    allocation adds): a reservation that left them out would grow here."""
    s = _session("tiny_rb1", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 120, 0).astype(np.int64)
    F = 40 * 120
    s.reserve(3, 40, F)
    cap = s.hparam("workspace_bytes")
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=dur)
    assert int(r["y_lengths"].max()) == F and s.hparam("workspace_bytes") == cap
    x, counts = _rows_of(r, s)
    assert x.size * (2 if rate is None else 4) > 1 << 20
    segs, J = _plans(3)["two streams, leads, stream peak"]
    for enc in ENCODINGS:
        assert _bytes(s.deliver(_segments(segs), J, enc)) == ref.deliver_ref(x, counts, segs, J, enc), enc
        assert s.hparam("workspace_bytes") == cap, (enc, "a delivery allocated behind a reservation that covers the request")
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
def test_synthesize_encoded_equals_the_host_join(encoding):
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.voice import TTSVoice
    voice = _voice("tiny_rb2_ms")

    def cfg(normalize):
        return SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=normalize)

    chunks = list(voice.synthesize(TEXT, cfg(True), batch_sentences=True))
    raw = [c.audio_float_array for c in voice.synthesize(TEXT, SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0,
                                                                               normalize_audio=False), batch_sentences=True)]
    assert len(chunks) == 3
    top = max(np.max(np.abs(a)) for a in raw)
    for silence in (0.0, 0.05):
        lead = int(22050 * silence * 2) // 2
        for scope in ("sentence", "text"):
            got = voice.synthesize_encoded(TEXT, cfg(True), encoding=encoding, sentence_silence=silence, normalize_scope=scope)
            pieces = [c.audio_float_array for c in chunks] if scope == "sentence" else [TTSVoice._scaled(a, top, 0.8) for a in raw]
            want = b"".join(ae.silence(lead, encoding).tobytes() + ae.encode(p, encoding).tobytes() for p in pieces)
            assert got.tobytes() == want, (silence, scope)
            assert got.sentence_samples == [len(p) for p in pieces] and got.sentence_starts[0] == lead
    voice.session.close()


def test_synthesize_requests_encoded_equals_the_encoded_requests():
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd.config import SynthesisConfig
    voice = _voice("tiny_rb2_ms")
    n_spk = voice.session.hparam("n_speakers")
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long. quietly", "hello there"]
    reqs = [(t, SynthesisConfig(speaker_id=i % n_spk, length_scale=(0.9, 1.0, 1.2)[i], volume=(1.0, 0.5, 2.0)[i],
                                normalize_audio=i != 1)) for i, t in enumerate(texts)]
    seeds = [7, 8, 9]
    chunks = voice.synthesize_requests(reqs, seeds=seeds, max_batch=4)
    lead = int(22050 * 0.01 * 2) // 2
    for enc in ("alaw", "f32"):
        got = voice.synthesize_requests_encoded(reqs, seeds=seeds, max_batch=4, encoding=enc, sentence_silence=0.01)
        for r, cs in enumerate(chunks):
            want = b"".join(ae.silence(lead, enc).tobytes() + ae.encode(c.audio_float_array, enc).tobytes() for c in cs)
            assert got[r].tobytes() == want, (enc, r)
            assert got[r].sentence_samples == [len(c.audio_float_array) for c in cs]
    voice.session.close()
