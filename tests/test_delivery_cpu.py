"""Delivery (include/vitsmi.h, "delivery") without a GPU: the encoders against audioop, the plan and its refusals through
vits_delivery_plan, the WAV container, the voice layer on stub sessions (the host encoder, and a stub that "delivers" by
the reference), and the delivery workspace walked by a stand-alone driver built with the host compiler.

Reference: tests/delivery_ref.py, an independent NumPy statement of the definition.  Everything is compared exactly."""
import io
import os
import shutil
import struct
import subprocess
import types
import wave

import numpy as np
import pytest

import delivery_ref as ref
from conftest import ROOT
from delivery_ref import COUNTS, REFUSALS, Seg

from phoonnx_amd import audio_encoding as ae
from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
from phoonnx_amd.session import Segment, SessionError, delivery_plan
from phoonnx_amd.voice import TTSVoice

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
ALL_INT16 = np.arange(-32768, 32768).astype(np.int16)


# ------------------------------------------------------------------ encoders

def test_encoders_equal_audioop_on_every_int16_value():
    audioop = pytest.importorskip("audioop")
    raw = ALL_INT16.astype("<i2").tobytes()
    want_u, want_a = audioop.lin2ulaw(raw, 2), audioop.lin2alaw(raw, 2)
    assert ref.ulaw(ALL_INT16).tobytes() == want_u and ref.alaw(ALL_INT16).tobytes() == want_a
    assert ae.ulaw_from_pcm16(ALL_INT16).tobytes() == want_u and ae.alaw_from_pcm16(ALL_INT16).tobytes() == want_a
    # ... and through encode(): floats that convert to every value in [-32767, 32767] (q / 32767 * 32767 truncates back to q)
    v = (ALL_INT16[1:].astype(np.float64) / 32767.0).astype(np.float32)
    q = ae.encode(v, "pcm16")
    back = q.astype("<i2").tobytes()
    assert ae.encode(v, "ulaw").tobytes() == audioop.lin2ulaw(back, 2) and ae.encode(v, "alaw").tobytes() == audioop.lin2alaw(back, 2)


def test_host_encoder_equals_the_reference():
    rng = np.random.default_rng(7)
    v = np.clip(rng.uniform(-1.2, 1.2, 5000), -1, 1).astype(np.float32)
    v[:6] = [1.0, -1.0, 0.0, -0.0, 1e-9, -3.0517578e-05]
    for enc in ENCODINGS:
        assert ae.encode(v, enc).tobytes() == ref.encode(v, enc), enc
        assert ae.silence(3, enc).tobytes() == ref.SILENCE[enc] * 3
        assert ae.encode(np.zeros(2, np.float32), enc).tobytes() == ref.SILENCE[enc] * 2     # silence = the encoding of 0
    with pytest.raises(ValueError, match="unknown encoding"):
        ae.encode(v, "mp3")


# ------------------------------------------------------------------ plan

PLANS = {
    "one row per stream": ([Seg(b, b, 0, 1, 1.0) for b in range(6)], 6),
    "empty streams, unused rows": ([Seg(4, 2, 3, 1, 1.0), Seg(0, 2, 0, 2, 0.5), Seg(2, 0, 1, 0, 2.5)], 4),
    "an empty row with a lead": ([Seg(1, 0, 4, 1, 1.0)], 1),
    "an empty row between two": ([Seg(0, 0, 0, 1, 1.0), Seg(1, 0, 0, 2, 1.0), Seg(3, 0, 0, 2, 1.0)], 2),
    "no segments": ([], 3),
    "the largest lead": ([Seg(5, 0, ref.INT_MAX, 0, 1.0), Seg(3, 0, ref.INT_MAX, 0, 1.0)], 1),
}


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_equals_the_reference(name, encoding):
    segs, J = PLANS[name]
    got = delivery_plan(COUNTS, [Segment(*s) for s in segs], J, encoding)
    samples, offsets, total = ref.plan_ref(COUNTS, segs, J, encoding)
    assert np.array_equal(got["stream_samples"], samples) and np.array_equal(got["stream_offsets"], offsets)
    assert got["total_bytes"] == total == offsets[-1]


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_plan_refusals_name_the_segment(name):
    segs, J, enc, index, word = REFUSALS[name]
    with pytest.raises(ValueError) as exc_ref:
        ref.plan_ref(COUNTS, segs, J, enc)
    with pytest.raises(SessionError) as exc:
        delivery_plan(COUNTS, [Segment(*s) for s in segs], J, enc)
    msg = str(exc.value)
    assert word in msg, msg
    if index is None:
        assert "segment -1" in str(exc_ref.value) and "segment" not in msg.split("]: ", 1)[1], msg
    else:
        assert f"segment {index}:" in msg and str(exc_ref.value) == f"segment {index}", (msg, str(exc_ref.value))


def test_an_unknown_encoding_is_refused_by_the_library():
    import ctypes as C
    from phoonnx_amd import _ffi
    lib = _ffi.load()
    total = C.c_int64(-1)
    seg = (_ffi.VitsSegment * 1)(_ffi.VitsSegment(0, 0, 0, 1, 1.0))
    for code in (-1, 4):
        assert lib.vits_delivery_plan(_ffi.ptr(COUNTS), 6, seg, 1, 1, code, None, None, C.byref(total)) == -3
        assert f"unknown encoding {code}" in _ffi.last_error(None) and total.value == -1
    assert lib.vits_delivery_plan(_ffi.ptr(COUNTS), 6, seg, 1, 1, 1, None, None, C.byref(total)) == 0 and total.value == 5
    with pytest.raises(SessionError, match="unknown encoding"):
        delivery_plan(COUNTS, [], 1, "mp3")
    assert C.sizeof(_ffi.VitsSegment) == 24      # int32, int32, int64, int32, float: the header's struct


# ------------------------------------------------------------------ WAV

def _chunks(b):
    """RIFF chunks of a WAVE file: [(id, payload)] and the RIFF size field"""
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE"
    size = struct.unpack("<I", b[4:8])[0]
    assert size == len(b) - 8
    out, pos = [], 12
    while pos < len(b):
        cid, n = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        out.append((cid, b[pos + 8:pos + 8 + n]))
        pos += 8 + n + (n & 1)
    assert pos == len(b)
    return out


def test_wav_bytes():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 1001).astype(np.float32)       # (1001: an odd data chunk for the one-byte encodings)
    pcm = ae.EncodedAudio(ae.encode(v, "pcm16"), "pcm16", 8000, [0], [1001])
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(8000)
        w.writeframes(pcm.tobytes())
    assert pcm.wav_bytes() == buf.getvalue() and pcm.tobytes() == ref.encode(v, "pcm16")
    for enc, tag, align in (("ulaw", 7, 1), ("alaw", 6, 1), ("f32", 3, 4)):
        for n in (1001, 1000, 0):
            a = ae.EncodedAudio(ae.encode(v[:n], enc), enc, 8000, [0], [n])
            (c0, fmt), (c1, fact), (c2, data) = _chunks(a.wav_bytes())
            assert (c0, c1, c2) == (b"fmt ", b"fact", b"data")
            assert struct.unpack("<HHIIHHH", fmt) == (tag, 1, 8000, 8000 * align, align, 8 * align, 0) and len(fmt) == 18
            assert struct.unpack("<I", fact) == (n,)
            assert data == a.tobytes() == ref.encode(v[:n], enc) and len(data) == n * align
            assert len(a.wav_bytes()) % 2 == 0


# ------------------------------------------------------------------ the voice layer on stub sessions

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


class _Stub:
    """A session without delivery: fixed waveforms - a row's audio depends on its ids, length scale, speaker and seed only -
    with garbage behind each row's end, and durations of 2 frames per id."""
    HOP = 3

    def __init__(self):
        self.batches = []

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": 4}[key]

    def last_durations(self):
        raise AssertionError("durations come back with the run")

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None, return_durations=False):
        B = ids.shape[0]
        self.batches.append(B)
        sc = np.broadcast_to(np.asarray(scales, np.float32), (B, 3))
        frames = lens.astype(np.int64) * 2
        out = np.full((B, 1, 1, int(frames.max()) * self.HOP + 4), 9.0, np.float32)
        for b in range(B):
            n = int(frames[b]) * self.HOP
            t = np.arange(n, dtype=np.float32)
            amp = np.float32(0.05 * (1 + int(ids[b, 0]) % 7) * sc[b, 1] + 0.01 * (0 if sid is None else int(sid[b])))
            out[b, 0, 0, :n] = amp * np.sin(t * np.float32(0.37) + (0 if seeds is None else int(seeds[b]) % 5))
        res = {"output": out, "y_lengths": frames}
        if return_durations:
            res["durations"] = np.where(np.arange(ids.shape[1])[None, :] < lens[:, None], 2, 0).astype(np.int64)
        return res


class _Delivering(_Stub):
    """... and one that delivers: the plan it is given, applied by the reference to the same waveforms"""

    def __init__(self):
        super().__init__()
        self.plans = []

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", seeds=None,
                             return_durations=False):
        r = self.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=return_durations)
        counts = r["y_lengths"] * self.HOP
        self.plans.append((list(segments), n_streams, encoding))
        streams = [np.frombuffer(b, ref.DTYPE[encoding]) for b in
                   ref.deliver_ref(r["output"][:, 0, 0, :], counts, segments, n_streams, encoding)]
        out = {"streams": streams, "stream_samples": np.array([len(a) for a in streams]), "y_lengths": r["y_lengths"],
               "sample_lengths": counts}
        if return_durations:
            out["durations"] = r["durations"]
        return out


def _voice(session):
    cfg = VoiceConfig(num_symbols=64, num_speakers=4, num_langs=1, sample_rate=16000, lang_code="en",
                      phoneme_id_map={c: [i + 1] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


TEXT = "the quick brown fox. jumps. over a lazy dog"


def _rows_of(voice, text, cfg):
    """the raw float rows of a text's sentences, as the stub renders them in one batch"""
    return voice.phoneme_ids_batch_to_audio(voice._sentence_ids(text, cfg), cfg)


@pytest.mark.parametrize("scope", ["sentence", "text"])
@pytest.mark.parametrize("silence", [0.0, 0.05, 0.00004])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_synthesize_encoded_on_stub_sessions(encoding, silence, scope):
    cfg = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=True)
    host, dev = _voice(_Stub()), _voice(_Delivering())
    rows = _rows_of(host, TEXT, cfg)
    lead = int(16000 * silence * 2) // 2
    assert lead == {0.0: 0, 0.05: 800, 0.00004: 0}[silence]
    # expected: the reference's bytes for this plan ("text": normalize 2 = the largest peak of the text)
    x = np.zeros((len(rows), max(map(len, rows))), np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    segs = [Seg(b, 0, lead, 2 if scope == "text" else 1, np.float32(0.8)) for b in range(len(rows))]
    want = ref.deliver_ref(x, counts, segs, 1, encoding)[0]
    a = host.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=silence, normalize_scope=scope, alignments=True)
    d = dev.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=silence, normalize_scope=scope, alignments=True)
    assert a.tobytes() == want == d.tobytes()
    assert a.data.dtype == d.data.dtype == ae.DTYPES[encoding] and a.encoding == encoding and a.sample_rate == 16000
    # the host path's bytes are the host encoder's
    peaks = [np.max(np.abs(r)) for r in rows]
    pieces = []
    for r, pk in zip(rows, peaks):
        v = TTSVoice._scaled(r, max(peaks) if scope == "text" else pk, cfg.volume)
        if scope == "sentence":
            assert np.array_equal(v, host._postprocess(r, cfg))
        pieces += [ae.silence(lead, encoding), ae.encode(v, encoding)]
    assert a.tobytes() == np.concatenate(pieces).tobytes()
    starts = [lead + sum(lead + c for c in counts[:k]) for k in range(len(counts))]
    for e in (a, d):
        assert e.sentence_starts == starts and e.sentence_samples == counts
        assert len(e.data) == sum(counts) + lead * len(counts)
        for k, al in enumerate(e.phoneme_alignments):       # shifted by the sentence's start, contiguous, covering it
            pos = starts[k]
            for p in al:
                assert p.start_sample == pos
                pos += p.num_samples
            assert pos == starts[k] + counts[k]
    # the device path asked for ONE stream with every sentence in it, in order
    (plan, J, enc), = dev.session.plans
    assert J == 1 and enc == encoding
    assert [(s.row, s.stream, s.lead_samples, s.normalize) for s in plan] == [(b, 0, lead, 2 if scope == "text" else 1) for b in range(len(rows))]


def test_text_scope_keeps_relative_levels_and_no_normalisation_is_normalize_0():
    cfg = SynthesisConfig(speaker_id=0, normalize_audio=True)
    voice = _voice(_Stub())
    rows = _rows_of(voice, TEXT, cfg)
    peaks = np.array([np.max(np.abs(r)) for r in rows])
    assert len(set(peaks.tolist())) > 1
    a = voice.synthesize_encoded(TEXT, cfg, encoding="f32", normalize_scope="text")
    got = [np.max(np.abs(a.data[s:s + n])) for s, n in zip(a.sentence_starts, a.sentence_samples)]
    assert np.array_equal(np.array(got, np.float32), (peaks / peaks.max()).astype(np.float32)) and max(got) == 1.0
    s = voice.synthesize_encoded(TEXT, cfg, encoding="f32", normalize_scope="sentence")
    assert all(np.max(np.abs(s.data[b:b + n])) == 1.0 for b, n in zip(s.sentence_starts, s.sentence_samples))
    raw = SynthesisConfig(speaker_id=0, normalize_audio=False, volume=1.0)
    dev = _voice(_Delivering())
    r = dev.synthesize_encoded(TEXT, raw, encoding="f32", normalize_scope="text")
    assert all(seg.normalize == 0 for seg in dev.session.plans[0][0])
    assert np.array_equal(r.data, np.concatenate(rows))
    with pytest.raises(ValueError, match="normalize_scope"):
        voice.synthesize_encoded(TEXT, cfg, normalize_scope="word")
    with pytest.raises(ValueError, match="unknown encoding"):
        voice.synthesize_encoded(TEXT, cfg, encoding="mp3")
    with pytest.raises(ValueError, match=r"speaker_id 9 is out of range \[0, 4\)"):
        dev.synthesize_encoded(TEXT, SynthesisConfig(speaker_id=9))
    assert len(dev.session.plans) == 1       # (refused before anything ran)
    empty = voice.synthesize_encoded("", cfg, encoding="ulaw")
    assert empty.tobytes() == b"" and empty.sentence_starts == []


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_synthesize_requests_encoded_on_stub_sessions(encoding):
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long. quietly", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=i, length_scale=(0.9, 1.0, 1.2)[i], volume=(1.0, 0.5, 2.0)[i], normalize_audio=i != 1)
            for i in range(3)]
    seeds = [11, 22, 33]
    reqs = list(zip(texts, cfgs))
    host, dev = _voice(_Stub()), _voice(_Delivering())
    lead = int(16000 * 0.01 * 2) // 2
    chunks = _voice(_Stub()).synthesize_requests(reqs, seeds=seeds, max_batch=4)
    a = host.synthesize_requests_encoded(reqs, seeds=seeds, max_batch=4, encoding=encoding, sentence_silence=0.01, alignments=True)
    d = dev.synthesize_requests_encoded(reqs, seeds=seeds, max_batch=4, encoding=encoding, sentence_silence=0.01, alignments=True)
    assert host.session.batches == dev.session.batches == [4, 2]        # synthesize_requests' batching: 6 sentences, 4 at a time
    for r, cs in enumerate(chunks):
        want = b"".join(ref.SILENCE[encoding] * lead + ae.encode(c.audio_float_array, encoding).tobytes() for c in cs)
        assert a[r].tobytes() == want == d[r].tobytes(), r
        counts = [len(c.audio_float_array) for c in cs]
        starts = [lead + sum(lead + c for c in counts[:k]) for k in range(len(counts))]
        for e in (a[r], d[r]):
            assert e.sentence_starts == starts and e.sentence_samples == counts and e.encoding == encoding
            assert [al[0].start_sample for al in e.phoneme_alignments] == starts
            assert [sum(p.num_samples for p in al) for al in e.phoneme_alignments] == counts
    # on the device: one stream per sentence, each with its request's own post-processing
    for plan, J, enc in dev.session.plans:
        assert J == len(plan) and [s.stream for s in plan] == list(range(J)) and all(s.lead_samples == 0 for s in plan)
        assert {(s.normalize, round(float(s.volume), 3)) for s in plan} <= {(1, 1.0), (0, 0.5), (1, 2.0)}
    with pytest.raises(ValueError, match="one seed per request"):
        dev.synthesize_requests_encoded(reqs, seeds=[1], encoding=encoding)


# ------------------------------------------------------------------ the delivery workspace

def test_the_delivery_workspace_is_the_size_its_walk_carves(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "delivery_driver")
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + csrc, os.path.join(ROOT, "tests", "delivery_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    BS, SS, KS = (1, 2, 3, 8, 32, 256), (1, 3, 96, 4097, 40000, 2000000), (38, 104)
    size = {}
    for ln in r.stdout.splitlines():
        b, s, k, verdict, rest = ln.split(" ", 4)
        assert verdict == "A", ln
        size[int(b), int(s), int(k)] = tuple(int(v) for v in rest.split())
    assert set(size) == {(b, s, k) for b in BS for s in SS for k in KS}
    for (b, s, k), (dlv, rs) in size.items():
        # the bound of the device side: 4 * B * S bytes of audio, B records of 32 bytes, 2 * B peaks (+ alignment)
        assert 4 * b * s + 32 * b + 8 * b <= dlv <= 4 * b * s + 16 + 32 * b + 8 * b + 3 * 256
        assert rs >= dlv + 6 * b * s          # behind the resampled waveform and its PCM
        for nb, ns in ((BS[min(BS.index(b) + 1, len(BS) - 1)], s), (b, SS[min(SS.index(s) + 1, len(SS) - 1)])):
            assert size[nb, ns, k][0] >= dlv and size[nb, ns, k][1] >= rs, (b, s, k, nb, ns)
