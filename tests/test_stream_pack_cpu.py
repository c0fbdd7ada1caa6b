"""Encoded streaming (include/vitsmi.h, "encoded streaming") without a GPU: the NumPy reference against the delivery's, every
refusal through a host-only session (Python's checks, and the engine's own through the C ABI) with no callback made, the
voice layer on stub sessions, and the stream's workspace walked by a stand-alone driver built with the host compiler.

Reference: tests/stream_pack_ref.py over tests/delivery_ref.py.  Everything is compared exactly."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import delivery_ref as dref
import stream_pack_ref as ref
from conftest import GOLDEN, ROOT
from delivery_ref import Seg

from phoonnx_amd import MiSession, SessionError, _ffi
from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
from phoonnx_amd.session import EncodedChunk
from phoonnx_amd.voice import TTSVoice

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")


# ------------------------------------------------------------------ the reference against the delivery's

def _rows():
    rng = np.random.default_rng(7)
    counts = np.array([0, 1, 15, 16, 17, 40, 96], np.int64)
    x = rng.uniform(-1.2, 1.2, (7, 96)).astype(np.float32)
    for b in range(7):
        x[b, int(counts[b]):] = np.nan
    return x, counts


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("piece", [1, 7, 16, 40, 96])
def test_pieces_rejoined_are_the_delivery_of_the_row(encoding, piece):
    x, counts = _rows()
    B = len(counts)
    volume = np.array([1.0, 0.5, 2.5, 1.0, 0.5, 2.5, 1.0], np.float32)
    own = np.array([np.max(np.abs(x[b, :int(counts[b])])) if counts[b] else 0 for b in range(B)], np.float32)
    for ref_peak, norm in ((None, 0), (own, 1)):
        chunks = ref.stream_ref(x, counts, ref.pieces(96, piece), encoding, ref_peak, volume)
        segs = [Seg(b, b, 0, norm, volume[b]) for b in range(B)]
        want = dref.deliver_ref(x, counts, segs, B, encoding)
        for b in range(B):
            assert ref.joined(chunks, b, encoding) == want[b], (b, norm)
        w = ref.WIDTH[encoding]
        for c in chunks:
            assert c.pitch % 16 == 0 and c.pitch - 16 < w * c.n <= c.pitch
            for b in range(B):
                assert c.valid[b] == min(max(int(counts[b]) - c.first, 0), c.n)
                pad = c.data[b][w * int(c.valid[b]):]
                assert pad == ref.SILENCE[encoding] * (len(pad) // w)
                assert encoding != "f32" or not np.isnan(np.frombuffer(c.data[b], "<f4")).any()
        peaks = np.stack([c.peak for c in chunks])
        assert (np.diff(peaks, axis=0) >= 0).all() and np.array_equal(peaks[-1], own) and not np.isnan(peaks).any()


# ------------------------------------------------------------------ refusals, in front of the handle and by the engine

@pytest.fixture(scope="module")
def host_session():
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    yield s
    s.close()


IDS = np.ones((2, 6), np.int64)
LENS = np.array([6, 4], np.int64)
SC = np.array([0.667, 1.0, 0.8], np.float32)
NAN, INF = float("nan"), float("inf")

# name the message carries -> keyword arguments
BAD = [
    ("unknown encoding", dict(encoding="mp3")),
    ("unknown encoding", dict(encoding=None)),
    ("volume[1]", dict(volume=[1.0, NAN])),
    ("volume[0]", dict(volume=INF)),
    ("ref_peak[1]", dict(ref_peak=[0.5, NAN])),
    ("ref_peak[0]", dict(ref_peak=[INF, 0.5])),
    ("ref_peak[1]", dict(ref_peak=[0.0, -0.25])),
    ("'volume'", dict(volume=[1.0, 1.0, 1.0])),
    ("'ref_peak'", dict(ref_peak=np.ones((2, 2), np.float32))),
]


@pytest.mark.parametrize("names,kw", BAD)
def test_bad_formats_are_named_before_the_handle_is_touched(host_session, names, kw):
    z = np.zeros((2, host_session.hparam("inter"), 5), np.float32)
    for call in (lambda: host_session.synthesize_stream_encoded(IDS, LENS, SC, **kw),
                 lambda: host_session.vocoder_stream_encoded(z, **kw)):
        with pytest.raises(SessionError) as ei:
            call()          # (raised by the call itself, not by the first next(): nothing was started)
        assert names in str(ei.value) and "host-only" not in str(ei.value), str(ei.value)


def test_valid_formats_reach_the_handle(host_session):
    """... and only then does a host-only handle refuse to run: the checks above are not what stopped the call.  A scalar
    broadcasts to the rows; a reference peak of 0 is a value (the row comes out as silence)."""
    for kw in (dict(), dict(encoding="ulaw", volume=0.5), dict(encoding="f32", ref_peak=[0.0, 0.7], volume=[1.0, 2.5]),
               dict(ref_peak=np.float64(0.3))):
        with pytest.raises(SessionError) as ei:
            list(host_session.synthesize_stream_encoded(IDS, LENS, SC, **kw))
        assert "host-only" in str(ei.value), str(ei.value)


def _c_format(encoding, ref_peak, volume):
    fmt = _ffi.VitsStreamFormat()
    fmt.encoding = encoding
    keep = [None if a is None else np.asarray(a, np.float32) for a in (ref_peak, volume)]
    fmt.ref_peak, fmt.volume = (None if a is None else a.ctypes.data for a in keep)
    fmt._keep = keep
    return fmt


C_BAD = [("unknown encoding 4", (4, None, None)), ("unknown encoding -1", (-1, None, None)),
         ("volume[1] = nan", (0, None, [1.0, NAN])), ("volume[0] = inf", (1, None, [INF, 1.0])),
         ("ref_peak[1] = nan", (2, [1.0, NAN], None)), ("ref_peak[0] = inf", (3, [INF, 1.0], None)),
         ("ref_peak[1] = -0.5", (0, [0.0, -0.5], [1.0, 1.0]))]


def test_the_engine_refuses_the_same_without_a_callback(host_session):
    """The C ABI's own validation (VITS_E_ARG = -3, the message naming row and value) answers before the handle needs a device,
    makes no callback, and comes in front of the chunked run's own checks: the ids below are out of range and T is 0."""
    lib, h = host_session._lib, host_session._h
    calls = []

    @_ffi.ENC_CHUNK_FN
    def cb(*args):
        calls.append(args)
        return 0

    rows = np.tile(SC, (2, 1))
    ctl = _ffi.VitsControls()
    ctl.scales_rows = rows.ctypes.data
    noise = _ffi.VitsNoise()
    z = np.zeros((2, host_session.hparam("inter"), 5), np.float32)
    bad_ids = np.full((2, 6), 10 ** 6, np.int64)

    def run(fmt, ids=IDS, T=6):
        return lib.vits_run_chunked_enc(h, _ffi.ptr(ids), _ffi.ptr(LENS), 2, T, None, C.byref(noise), C.byref(ctl), fmt, 4, cb, None)

    def voc(fmt):
        return lib.vits_run_vocoder_chunked_enc(h, _ffi.ptr(z), 2, 5, None, fmt, 4, cb, None)

    for word, args in C_BAD:
        fmt = _c_format(*args)
        for rc in (run(C.byref(fmt)), run(C.byref(fmt), bad_ids, 0), voc(C.byref(fmt))):
            assert rc == -3 and word in host_session._err(), (word, rc, host_session._err())
    for rc in (run(None), voc(None)):
        assert rc == -3 and "null stream format" in host_session._err()
    # a format that passes reaches the device check (fn == NULL is allowed: it is not what is refused)
    good = _c_format(1, [0.0, 0.5], [2.5, 1.0])
    assert run(C.byref(good)) != 0 and "host-only" in host_session._err()
    assert lib.vits_run_chunked_enc(h, _ffi.ptr(IDS), _ffi.ptr(LENS), 2, 6, None, C.byref(noise), C.byref(ctl), C.byref(good), 4,
                                    _ffi.ENC_CHUNK_FN(), None) != 0 and "host-only" in host_session._err()
    assert calls == []


def test_the_test_hook_checks_its_sizes_on_the_host():
    lib = _ffi.load()
    x, counts = _rows()
    fmt = _c_format(0, None, None)
    out = np.zeros(7 * 16 * 96, np.uint8)
    pitches, valid, peaks = np.zeros(96, np.int64), np.zeros((96, 7), np.int32), np.zeros((96, 7), np.float32)

    def hook(counts=counts, piece=16, fmt=fmt, cap=out.nbytes, max_pieces=96, S=96):
        return lib.vits_test_stream_pack(0, _ffi.ptr(x), _ffi.ptr(counts), 7, S, piece, C.byref(fmt) if fmt is not None else None,
                                         _ffi.ptr(out), cap, _ffi.ptr(pitches), _ffi.ptr(valid), _ffi.ptr(peaks), max_pieces)

    over = counts.copy()
    over[2] = 97
    for word, kw in (("counts[2] = 97", dict(counts=over)), ("bad stream pack test arguments", dict(piece=0)),
                     ("null stream format", dict(fmt=None)), ("unknown encoding 9", dict(fmt=_c_format(9, None, None))),
                     ("6 pieces", dict(max_pieces=5)), ("room for", dict(cap=7 * 32 * 6 - 1)),
                     ("bad stream pack test arguments", dict(S=0))):
        assert hook(**kw) == -3 and word in _ffi.last_error(None), (word, _ffi.last_error(None))
    assert not out.any()


def test_the_stream_closure_owns_its_arrays(host_session, monkeypatch):
    """The C call runs on _stream's worker thread after synthesize_stream_encoded has returned: the closure must own the
    converted copies the structs point into (a list of volumes, a scalar reference peak)."""
    import gc
    captured = []
    monkeypatch.setattr(host_session, "_stream", lambda start, wrap=None: captured.append((start, wrap)))
    host_session.synthesize_stream_encoded(IDS, LENS, SC, encoding="alaw", ref_peak=0.25, volume=[1.0, 2.5], seeds=[1, 2])
    gc.collect()
    (start, wrap), = captured
    cells = dict(zip(start.__code__.co_freevars, (c.cell_contents for c in start.__closure__)))
    fmt, ctl = cells["fmt"], cells["ctl"]
    peak, volume = fmt._keep
    assert fmt.encoding == 2 and peak.dtype == volume.dtype == np.float32
    assert peak.tolist() == [0.25, 0.25] and volume.tolist() == [1.0, 2.5]
    assert fmt.ref_peak == peak.ctypes.data and fmt.volume == volume.ctypes.data
    assert ctl._keep[1].tolist() == [1, 2] and wrap[0] is _ffi.ENC_CHUNK_FN


def test_a_chunk_is_copied_out_of_the_engines_buffer():
    """EncodedChunk.data must not alias the buffer the callback was given (valid during the call only) - also where the row
    pitch equals the row's bytes and the cut is the whole block."""
    fn_type, item = MiSession._encoded_items(np.int16)
    assert fn_type is _ffi.ENC_CHUNK_FN
    for n, pitch in ((8, 16), (5, 16)):
        buf = np.arange(2 * pitch, dtype=np.uint8)
        valid, peak = np.array([n, 2], np.int32), np.array([0.5, 0.25], np.float32)
        c = item(buf.ctypes.data, 2, pitch, 40, n, valid.ctypes.data_as(C.POINTER(C.c_int32)),
                 peak.ctypes.data_as(C.POINTER(C.c_float)), 99)
        want = buf.reshape(2, pitch)[:, :2 * n].copy().view(np.int16)
        buf[:], valid[:], peak[:] = 0xEE, -1, -1.0
        assert c.data.shape == (2, n) and c.data.dtype == np.int16 and np.array_equal(c.data, want)
        assert c.valid.tolist() == [n, 2] and c.peak.tolist() == [0.5, 0.25] and (c.first_sample, c.total_samples) == (40, 99)


# ------------------------------------------------------------------ the voice layer on stub sessions

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


HOP = 3


def _render(ids, lens, scales, sid):
    """fixed waveforms: a row's audio depends on its ids, length scale and speaker; garbage behind each row's end"""
    B = ids.shape[0]
    sc = np.broadcast_to(np.asarray(scales, np.float32), (B, 3))
    frames = lens.astype(np.int64) * 2
    out = np.full((B, 1, 1, int(frames.max()) * HOP + 4), 9.0, np.float32)
    for b in range(B):
        n = int(frames[b]) * HOP
        t = np.arange(n, dtype=np.float32)
        amp = np.float32(0.05 * (1 + int(ids[b, 0]) % 7) * sc[b, 1] + 0.01 * (0 if sid is None else int(sid[b])))
        out[b, 0, 0, :n] = amp * np.sin(t * np.float32(0.37))
    return out, frames


class _Ort:
    """the onnxruntime duck type: get_inputs() / run() only"""

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def run(self, names, feed):
        out, frames = _render(feed["input"], feed["input_lengths"], feed["scales"], feed.get("sid"))
        return [out[:, :, :, :int(frames[0]) * HOP]]


class _Batch:
    """A session that renders whole batches only"""
    HOP = HOP

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": 4}[key]

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None, return_durations=False):
        out, self.frames = _render(ids, lens, scales, sid)
        return {"output": out, "y_lengths": self.frames}


class _Streams(_Batch):
    """... one that streams fp32 chunks (the rows' padding included, as vits_run_chunked hands it over)"""

    def synthesize_stream(self, ids, lens, scales, sid=None, chunk_frames=64):
        r = self.synthesize_batch(ids, lens, scales, sid)
        total = int(r["y_lengths"].max()) * self.HOP
        x = r["output"][:, 0, 0, :total]
        step = chunk_frames * self.HOP
        return ((f, x[:, f:f + step].copy(), total) for f in range(0, total, step))

    def last_y_lengths(self):
        return self.frames


class _StreamsEncoded(_Streams):
    """... and one that streams encoded chunks: the reference applied to the same waveforms"""

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None):
        r = self.synthesize_batch(ids, lens, scales, sid)
        B = ids.shape[0]
        counts = r["y_lengths"] * self.HOP
        total = int(counts.max())
        self.formats = getattr(self, "formats", []) + [(encoding, ref_peak, volume)]
        vol = None if volume is None else np.broadcast_to(np.float32(volume), (B,))
        for c in ref.stream_ref(r["output"][:, 0, 0, :], counts, ref.pieces(total, chunk_frames * self.HOP), encoding, ref_peak, vol):
            w = ref.WIDTH[encoding]
            data = np.stack([np.frombuffer(row[:w * c.n], ref.DTYPE[encoding]) for row in c.data])
            yield EncodedChunk(c.first, data, c.valid, c.peak, total)


def _voice(session):
    cfg = VoiceConfig(num_symbols=64, num_speakers=4, num_langs=1, sample_rate=16000, lang_code="en",
                      phoneme_id_map={c: [i + 1] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


TEXT = "the quick brown fox. jumps. over a lazy dog"
SESSIONS = {"run only": _Ort, "whole batches": _Batch, "fp32 chunks": _Streams, "encoded chunks": _StreamsEncoded}


@pytest.mark.parametrize("kind", sorted(SESSIONS))
@pytest.mark.parametrize("silence", [0.0, 0.05])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_stream_encoded_on_stub_sessions(encoding, silence, kind):
    raw = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=False)
    norm = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=True)
    whole = _voice(_Batch())
    want_raw = whole.synthesize_encoded(TEXT, raw, encoding=encoding, sentence_silence=silence)
    want_norm = whole.synthesize_encoded(TEXT, norm, encoding=encoding, sentence_silence=silence)
    rows = whole.phoneme_ids_batch_to_audio(whole._sentence_ids(TEXT, raw), raw)
    assert len(rows) == 3 and len({len(r) for r in rows}) == 3
    peaks = [np.max(np.abs(r)) for r in rows]
    for chunk_frames in (1, 5, 64):
        voice = _voice(SESSIONS[kind]())
        got = list(voice.stream_encoded(TEXT, raw, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=silence))
        assert all(isinstance(p, bytes) and p for p in got)
        assert b"".join(got) == want_raw.data.tobytes(), (kind, chunk_frames)
        if kind in ("fp32 chunks", "encoded chunks") and chunk_frames == 1:
            # sentence 0 goes out as it arrives: a piece per chunk (behind the pause), not one piece per sentence
            assert len(got) >= len(rows[0]) // (HOP * chunk_frames)
        got = voice.stream_encoded(TEXT, norm, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=silence, ref_peak=peaks)
        assert b"".join(got) == want_norm.data.tobytes(), (kind, chunk_frames)
    if kind == "encoded chunks":      # the device path was asked for the config's volume and the peaks, per row
        enc, pk, vol = voice.session.formats[-1]
        assert enc == encoding and vol == pytest.approx(0.8) and np.array_equal(pk, np.asarray(peaks, np.float32))
        assert voice.session.formats[0][1] is None


def test_stream_encoded_needs_a_reference_peak_to_normalise():
    voice = _voice(_StreamsEncoded())
    with pytest.raises(ValueError, match="cannot know its own peak"):
        voice.stream_encoded(TEXT)                                    # (the default config normalises; raised by the call itself)
    with pytest.raises(ValueError, match="cannot know its own peak"):
        voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=True), encoding="ulaw")
    assert not hasattr(voice.session, "formats")
    with pytest.raises(ValueError, match="unknown encoding"):
        voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=False), encoding="mp3")
    with pytest.raises(ValueError, match="sentence_silence"):
        voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=False), sentence_silence=-1.0)
    with pytest.raises(ValueError, match="one per sentence"):
        list(voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=True), ref_peak=[0.5, 0.5]))
    # a scalar reference peak is every sentence's
    one = b"".join(voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=True), ref_peak=0.25))
    each = b"".join(voice.stream_encoded(TEXT, SynthesisConfig(normalize_audio=True), ref_peak=[0.25] * 3))
    assert one == each and one
    assert list(voice.stream_encoded("", SynthesisConfig(normalize_audio=False))) == []


# ------------------------------------------------------------------ the stream's workspace

def test_the_stream_workspace_is_the_size_its_walk_carves(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stream_pack_driver")
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + csrc, os.path.join(ROOT, "tests", "stream_pack_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    BS, NS, KS = (1, 2, 3, 7, 32, 256), (1, 3, 96, 4097, 16384, 2000000), (38, 104)
    size = {}
    for ln in r.stdout.splitlines():
        b, n, k, verdict, rest = ln.split(" ", 4)
        assert verdict == "A", ln
        size[int(b), int(n), int(k)] = tuple(int(v) for v in rest.split())
    assert set(size) == {(b, n, k) for b in BS for n in NS for k in KS}
    for (b, n, k), (sp, rs) in size.items():
        # the largest chunk as F32 at a 16-byte row pitch, a float per row in whole cells, two floats per row
        need = b * (-(-4 * n // 16) * 16) + -(-4 * b // 16) * 16 + 8 * b
        assert sp == need, (b, n, sp, need)
        assert rs >= sp + 10 * b * (n + 5)          # behind the resampled waveform, its PCM and its delivery buffers
        for nb, nn in ((BS[min(BS.index(b) + 1, len(BS) - 1)], n), (b, NS[min(NS.index(n) + 1, len(NS) - 1)])):
            assert size[nb, nn, k][0] >= sp and size[nb, nn, k][1] >= rs, (b, n, k, nb, nn)
