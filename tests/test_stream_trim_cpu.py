"""The leading trim of the encoded stream without a GPU (include/vitsmi.h, "trimmed streaming"): the reference against itself
and against the limited delivery's reference under the equivalent trim, the two pure host entries, the struct, the names,
and the host fallback (audio_encoding.stream_shaped(onsets=)) against the reference - bytes and skips."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import limit_ref as lref
import shape_ref as sref
import stream_pack_ref as pref
import stream_shape_ref as ssref
import stream_trim_ref as ref

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, THR, COUNTS = ref.B, ref.S, ref.THR, ref.COUNTS
VOLUME = np.array([1.0, 0.5, 3.0, 1.0, 0.5], np.float32)
CEILINGS = (0.7, 0.7, 0.7, 0.7, 0.0)
SHAPES = [sref.Shape(300, 500, 1, ((100, 1.0), (900, 0.25), (901, 2.0), (4000, 1.0))), sref.Shape(0, 0, 0, ((0, 2.0), (4096, 0.5))),
          sref.Shape(4, 4, 0, ()), sref.NONE, sref.Shape(64, 64, 0, ())]


X = ref.batch()
F_WANT = [1300, 0, None, None, 2048]


def onsets(keep_lead, thr=THR, mode=1):
    return [ref.Onset(mode, thr, keep_lead)] * B


def limits(L):
    return [lref.Limit(c, L) if c else None for c in CEILINGS] if L else None


def test_the_rows_are_what_the_cases_need():
    fs, _ = ref.starts(X, COUNTS, pref.pieces(S, S), onsets(0))
    assert fs == F_WANT
    assert abs(X[0, 1299]) == np.float32(THR) and (np.abs(X[0, :1300]) <= np.float32(THR)).all()
    assert (np.abs(X[2, 1:]) > THR).all() and (np.abs(X[3]) > THR).all()      # active only behind the rows' ends


@pytest.mark.parametrize("L", [0, 1, 255, 1024])
def test_chunking_invariance_of_the_start(L):
    """a_b is the delivery's max(0, f - keep_lead) for every piece size when keep_lead <= L or f lies in piece 0"""
    for keep_lead in (0, 100, 2000):
        for piece in (7, 256, 1000, 5000):
            fs, a = ref.starts(X, COUNTS, pref.pieces(S, piece), onsets(keep_lead), L)
            assert fs == F_WANT
            for b in (0, 1, 4):
                delivery = max(0, fs[b] - keep_lead)
                assert delivery <= a[b] <= fs[b]
                if keep_lead <= L or fs[b] < piece:
                    assert a[b] == delivery, (L, keep_lead, piece, b)
            assert a[2] == a[3] == ref.INT_MAX


def test_the_clamped_case():
    """keep_lead 2000, L 0, pieces of 256, f = 1300: the piece of f begins at 1280 and the stream has handed over all before"""
    _, a = ref.starts(X, COUNTS, pref.pieces(S, 256), onsets(2000), 0)
    assert a[0] == 1280 and max(0, 1300 - 2000) == 0
    assert a[4] == 2048                       # f on a piece boundary: nothing in front of it is left
    _, a = ref.starts(X, COUNTS, pref.pieces(S, 256), onsets(2000), 255)
    assert a[0] == 1280 - 255 and a[4] == 2048 - 255


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_reference_equals_the_limited_delivery_under_the_equivalent_trim(encoding):
    """the specification itself, where the delivery's reference can state it: no ref_peak (normalize 0)"""
    for L, piece, keep_lead in ((0, 256, 2000), (255, 1000, 100), (1024, 7, 0)):
        fs, a = ref.starts(X, COUNTS, pref.pieces(S, piece), onsets(keep_lead), L)
        rows = ref.rows_ref(X, COUNTS, a, encoding, None, VOLUME, SHAPES, limits(L))
        trim = ref.equivalent_trims(fs, a, COUNTS)
        for b in (0, 1, 4):
            segs = [lref.Seg(b, 0, 0, 0, float(VOLUME[b]))]
            shapes = [SHAPES[r] for r in range(B)]
            want, kept, _ = lref.deliver_ref(np.where(np.arange(S)[None, :] < COUNTS[:, None], X, 0), COUNTS, segs, [trim(b, THR)], None,
                                             [shapes[b]], None if not L else [limits(L)[b]], 1, encoding)
            assert kept[0] == (a[b], int(COUNTS[b]) - a[b]) and rows[b] == want[0], (L, piece, keep_lead, b)
        assert rows[2] == rows[3] == b""


def test_onset_start_against_the_reference():
    from phoonnx_amd.session import SessionError, stream_onset_start
    for f in (0, 1, 255, 256, 1300, 2 ** 31 - 2):
        for keep_lead in (0, 1, 100, 2000, 2 ** 31 - 1):
            for D in sorted({0, f // 2, max(f - 1, 0), f}):
                assert stream_onset_start(f, keep_lead, D) == ref.onset_start(f, keep_lead, D)
    for bad in ((-1, 0, 0), (5, -1, 0), (5, 0, -1), (5, 0, 6)):
        with pytest.raises(SessionError, match="bad onset start"):
            stream_onset_start(*bad)


REFUSALS = {
    "mode 3": ([(1, 0.1, 0, 0), (3, 0.1, 0, 0)], 1.0, "row 1: onset mode 3"),
    "mode -1": ([(-1, 0.1, 0, 0)], 1.0, "row 0: onset mode -1"),
    "threshold negative": ([(0, 0.0, 0, 0), (0, 0.0, 0, 0), (1, -0.5, 0, 0)], None, "row 2: onset threshold -0.5"),
    "threshold nan": ([(1, float("nan"), 0, 0)], None, "row 0: onset threshold nan"),
    "threshold inf": ([(2, float("inf"), 0, 0)], 1.0, "row 0: onset threshold inf"),
    "keep_lead negative": ([(1, 0.1, 0, 0), (1, 0.1, -7, 0)], None, "row 1: onset keep_lead -7"),
    "reserved": ([(1, 0.1, 0, 9)], None, "row 0: onset reserved 9"),
    "mode 2 without ref_peak": ([(1, 0.1, 0, 0), (2, 0.1, 0, 0)], None, "row 1: onset mode 2 needs ref_peak"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_onset_check_refuses(name):
    from phoonnx_amd.session import RawOnset, SessionError, stream_onset_check
    raw, peak, word = REFUSALS[name]
    with pytest.raises(ValueError):
        ref.check_onsets(raw, peak)
    with pytest.raises(SessionError, match=re.escape(word)):
        stream_onset_check([RawOnset(*r) for r in raw], len(raw), peak)


def test_onset_check_accepts():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import Onset, stream_onset_check
    stream_onset_check(None, 3)
    stream_onset_check([Onset(1, 0.0, 0), None, Onset(0, 0.0, 0)], 3)
    stream_onset_check(Onset(2, 0.02, 2 ** 31 - 1), 4, ref_peak=0.0)
    assert _ffi.load().vits_stream_onset_check(None, None, 3) == 0


def test_struct_and_names():
    from phoonnx_amd import _ffi
    assert C.sizeof(_ffi.VitsStreamOnset) == 16
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    assert re.search(r"}\s*vits_stream_onset;\s*/\* 16 bytes \*/", header)
    lib = _ffi.load()
    for name in ("vits_stream_onset_check", "vits_stream_onset_start", "vits_run_chunked_enc_trimmed", "vits_run_vocoder_chunked_enc_trimmed",
                 "vits_test_stream_pack_trimmed"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert "vits_enc_chunk_trim_fn" in header


def test_encoded_chunk_keeps_its_constructions():
    from phoonnx_amd.session import EncodedChunk
    c = EncodedChunk(0, np.zeros((1, 4), np.int16), np.array([4], np.int32), np.zeros(1, np.float32), 4)
    assert c.skip is None
    assert EncodedChunk(0, c.data, c.valid, c.peak, 4, np.array([2], np.int32)).skip[0] == 2


def _fallback(piece, encoding, L, keep_lead, ref_peak=None, mode=1, thr=THR):
    from phoonnx_amd import audio_encoding as ae
    chunks = ((f, np.where(np.arange(f, f + n)[None, :] < COUNTS[:, None], X[:, f:f + n], np.nan), S) for f, n in pref.pieces(S, piece))
    return list(ae.stream_shaped(chunks, COUNTS, encoding, ref_peak, VOLUME, SHAPES, limits(L) if L else None, onsets(keep_lead, thr, mode)))


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_host_fallback_equals_the_reference(encoding):
    w = ref.WIDTH[encoding]
    for L, piece, keep_lead in ((0, 256, 2000), (0, 5000, 100), (1, 7, 0), (255, 1000, 2000), (1024, 256, 100)):
        fs, a = ref.starts(X, COUNTS, pref.pieces(S, piece), onsets(keep_lead), L)
        rows = ref.rows_ref(X, COUNTS, a, encoding, None, VOLUME, SHAPES, limits(L))
        got = _fallback(piece, encoding, L, keep_lead)
        ranges = [r for r in ssref.timeline(pref.pieces(S, piece), S, L) if r[1]]
        assert [(c[0], c[1].shape[1]) for c in got] == ranges
        for c, want in zip(got, ref.skips(a, COUNTS, ranges)):
            assert np.array_equal(c[5], want) and np.array_equal(c[2], np.clip(COUNTS - c[0], 0, c[1].shape[1]))
            for b in range(B):
                assert c[1][b, :int(c[5][b])].tobytes() == ref.SILENCE[encoding] * int(c[5][b])
        for b in range(B):
            assert b"".join(c[1][b, int(c[5][b]):int(c[2][b])].tobytes() for c in got) == rows[b], (L, piece, keep_lead, b)
            assert sum(int(c[5][b]) for c in got) == min(a[b], int(COUNTS[b]))
        assert len(rows[0]) == w * (5000 - a[0])


def test_host_fallback_mode_2_is_mode_1_with_the_product():
    peaks = np.array([0.8, 0.5, 0.3, 1.0, 2.0], np.float32)
    two = _fallback(256, "pcm16", 255, 100, ref_peak=peaks, mode=2, thr=0.25)
    from phoonnx_amd import audio_encoding as ae
    per_row = [ref.Onset(1, float(np.float32(0.25) * peaks[b]), 100) for b in range(B)]
    chunks = ((f, np.where(np.arange(f, f + n)[None, :] < COUNTS[:, None], X[:, f:f + n], np.nan), S) for f, n in pref.pieces(S, 256))
    one = list(ae.stream_shaped(chunks, COUNTS, "pcm16", peaks, VOLUME, SHAPES, limits(255), per_row))
    assert len(one) == len(two)
    for p, q in zip(one, two):
        assert p[1].tobytes() == q[1].tobytes() and np.array_equal(p[5], q[5])
    assert any(int(c[5][4]) for c in two) and not any(int(c[5][1]) for c in two)


def test_host_fallback_without_onsets_is_unchanged():
    from phoonnx_amd import audio_encoding as ae
    chunks = [(f, np.nan_to_num(X[:, f:f + n]), S) for f, n in pref.pieces(S, 1000)]
    plain = list(ae.stream_shaped(iter(chunks), COUNTS, "ulaw", None, VOLUME, SHAPES, limits(7)))
    off = list(ae.stream_shaped(iter(chunks), COUNTS, "ulaw", None, VOLUME, SHAPES, limits(7), [ref.Onset(0, 0.0, 0)] * B))
    assert all(len(c) == 5 for c in plain) and all(len(c) == 6 and not c[5].any() for c in off)
    assert [c[1].tobytes() for c in plain] == [c[1].tobytes() for c in off]


# ------------------------------------------------------------------ the voice layer on stand-in sessions (the host fallbacks)

@pytest.mark.parametrize("kind", ["run only", "whole batches", "fp32 chunks"])
def test_voice_trim_silence_on_the_host_fallbacks(kind):
    """at 16 kHz: keep_lead 1 sample within a look-ahead of 16, so every chunking gives synthesize_encoded's leading trim (the
    stand-in waveforms rise from 0 within a few samples: the threshold sits at 0.8 of their peak)"""
    import test_stream_shape_cpu as shaped
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.session import Onset, Trim
    raw = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=False)
    whole = shaped._voice(shaped._Batch())
    kw = dict(fade_in=0.001, fade_out=0.002, limit_ceiling=0.1, limit_lookahead=0.001)
    plain = whole.synthesize_encoded(shaped.TEXT, raw, encoding="pcm16", sentence_silence=0.05, **kw)
    loud = np.abs(whole.synthesize_encoded(shaped.TEXT, raw, encoding="f32", sentence_silence=0.0).data).max() / 0.8
    thr, lead = float(0.8 * loud), 1 / 16000
    want = whole.synthesize_encoded(shaped.TEXT, raw, encoding="pcm16", sentence_silence=0.05, trim_silence=Trim(1, thr, lead, 3600.0), **kw)
    assert 0 < sum(want.sentence_samples) < sum(plain.sentence_samples)
    for chunk_frames in (1, 5, 64):
        voice = shaped._voice(shaped.SESSIONS[kind]())
        got = list(voice.stream_encoded(shaped.TEXT, raw, encoding="pcm16", chunk_frames=chunk_frames, sentence_silence=0.05,
                                        trim_silence=Onset(1, thr, lead), **kw))
        assert b"".join(got) == want.data.tobytes(), (kind, chunk_frames)
    for bad in (0.3, Onset(2, 0.3, 0.0)):
        with pytest.raises(ValueError, match=r"Onset\(1, "):
            voice.stream_encoded(shaped.TEXT, raw, trim_silence=bad)
    with pytest.raises(TypeError):      # a session from before the trim says so when it is asked for one
        list(shaped._voice(shaped._StreamsShaped()).stream_encoded(shaped.TEXT, raw, trim_silence=Onset(1, thr, 0.0)))
