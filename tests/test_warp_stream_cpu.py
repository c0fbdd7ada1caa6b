"""Streamed pitch (include/vitsmi.h, "streamed pitch") without a GPU: the emit rule - vits_warp_emit_end / vits_glide_emit_end -
against a brute-force count over the positions of tests/warp_ref.py and tests/glide_ref.py, n_cap, the refusals that are pure
host code, and TTSVoice.stream_encoded's phoneme_pitch= / pitch_contour= on a recording session."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glide_ref
import warp_ref
from test_glide_cpu import _Recorder, _voice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB, HALF = warp_ref.FB, 38
HOP = 8


def _lib():
    from phoonnx_amd import _ffi
    return _ffi, _ffi.load()


# the rows of the rule: (name, durations in frames, start values, end values)
ROWS = (
    ("dropped token", [5, 0, 7, 3], [3, 5, -7, 12], [3, 5, -7, 12]),
    ("shorter than 38 samples", [2, 2], [4, -4], [4, -4]),
    ("rise -12 -> +12", [40], [-12], [12]),
    ("fall +12 -> -12", [40], [12], [-12]),
    ("mixed glides", [6, 0, 9, 1, 4], [0, 1, -12, 7, 2], [0, 1, 5, 7, -3]),
    ("identity", [7, 3], [0, 0], [0, 0]),
)


def _warp_positions(D, st):
    segs, _, N = warp_ref.plan(D, st, HOP)
    pos = np.concatenate([g.pos0 + np.arange(g.k, dtype=np.int64) * g.step for g in segs] + [np.zeros(0, np.int64)])
    return pos, N


def _glide_positions(D, st0, st1):
    segs, _, N = glide_ref.plan(D, st0, st1, HOP)
    pos = np.concatenate([glide_ref.samples(g)[0] for g in segs if g.k] + [np.zeros(0, np.int64)])
    return pos, N


def _brute(pos, N, n_in, X):
    """the rule, counted: a complete row has all N; else the n whose 38 half-taps lie in front of X"""
    assert len(pos) == N
    return N if X >= n_in else int(np.count_nonzero((pos >> FB) + HALF < X))


def _check(emit, segs, pos, N, n_in, name):
    assert np.all(np.diff(pos) >= 0), name   # (what makes the count a prefix count)
    last = 0
    for X in range(0, n_in + 3):
        got = emit(segs, n_in, N, X)
        assert got == _brute(pos, N, n_in, X), (name, X, got)
        assert got >= last, (name, X)
        last = got
        if X >= n_in:
            assert got == N, (name, X)
    # short of input, nothing is ready whose taps reach X: the last ready sample's staged span ends in front of X
    for X in (1, HALF, HALF + 1, n_in - 1):
        if 0 < X < n_in:
            r = emit(segs, n_in, N, X)
            assert r == 0 or (int(pos[r - 1]) >> FB) + HALF < X, (name, X)
            assert r == N or (int(pos[r]) >> FB) + HALF >= X, (name, X)


def test_the_entries_are_declared_and_exported():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_warp_emit_end", "vits_glide_emit_end", "vits_run_chunked_glided", "vits_run_chunked_enc_glided",
                 "vits_test_warp_pieces", "vits_test_glide_pieces"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert hasattr(lib, "vits_warp_stream_cap") and re.search(r"\bint64_t vits_warp_stream_cap\(", header)
    assert "streamed pitch" in header


@pytest.mark.parametrize("name,D,st0,st1", ROWS, ids=[r[0] for r in ROWS])
def test_glide_emit_end_is_the_brute_force_count(name, D, st0, st1):
    from phoonnx_amd.session import glide_emit_end, glide_plan
    segs, _, N = glide_plan(D, st0, st1, HOP)
    pos, N_ref = _glide_positions(D, st0, st1)
    assert N == N_ref
    _check(glide_emit_end, segs, pos, N, sum(D) * HOP, name)


@pytest.mark.parametrize("name,D,st0,st1", [r for r in ROWS if r[2] == r[3]], ids=[r[0] for r in ROWS if r[2] == r[3]])
def test_warp_emit_end_is_the_brute_force_count(name, D, st0, st1):
    from phoonnx_amd.session import glide_emit_end, glide_plan, warp_emit_end, warp_plan
    segs, _, N = warp_plan(D, st0, HOP)
    pos, N_ref = _warp_positions(D, st0)
    assert N == N_ref
    n_in = sum(D) * HOP
    _check(warp_emit_end, segs, pos, N, n_in, name)
    # equal ends: the glide's rule is the warp's
    gsegs, _, gN = glide_plan(D, st0, st1, HOP)
    assert gN == N and all(glide_emit_end(gsegs, n_in, N, X) == warp_emit_end(segs, n_in, N, X) for X in range(0, n_in + 3, 7))


def test_a_row_without_a_record_is_the_masked_copy():
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import glide_emit_end, warp_emit_end
    for emit, seg in ((warp_emit_end, _ffi.VitsWarpSeg), (glide_emit_end, _ffi.VitsGlideSeg)):
        none = (seg * 0)()
        for n_in in (0, 1, 37, 38, 39, 100):
            for X in range(0, n_in + 3):
                want = n_in if X >= n_in else max(0, min(n_in, X - HALF))
                assert emit(none, n_in, n_in, X) == want, (n_in, X)


def test_emit_end_refuses_what_is_not_a_row():
    from phoonnx_amd.session import SessionError, warp_emit_end, warp_plan
    segs, _, N = warp_plan([4, 4], [3, -3], HOP)
    with pytest.raises(SessionError, match="n_out"):
        warp_emit_end(segs, 64, N + 1, 10)
    with pytest.raises(SessionError, match="bad emit end arguments"):
        warp_emit_end(segs, 64, N, -1)
    segs[1].pos0 += 1
    with pytest.raises(SessionError, match="does not continue the row"):
        warp_emit_end(segs, 64, N, 10)


def test_n_cap():
    from phoonnx_amd.session import SessionError, warp_stream_cap
    assert warp_stream_cap(256, 10 ** 6) == 2 * (256 + HALF)
    assert warp_stream_cap(256, 100) == 100 and warp_stream_cap(1, 10 ** 6) == 78
    with pytest.raises(SessionError):
        warp_stream_cap(0, 5)
    # what one piece of c inputs can complete at the least step, the rule's 38 on either side: never more than n_cap
    from phoonnx_amd.session import glide_emit_end, glide_plan
    for st0, st1 in ((-12, -12), (-12, 12), (12, -12)):
        D = [30]
        segs, _, N = glide_plan(D, [st0], [st1], HOP)
        n_in = sum(D) * HOP
        for c in (1, 8, 24):
            cap = warp_stream_cap(c, 10 ** 6)
            ends = [glide_emit_end(segs, n_in, N, X) for X in range(0, n_in, c)]   # (every piece but the last)
            assert max(np.diff(ends), default=0) <= cap, (st0, st1, c)


# ------------------------------------------------------------------ refusals that need no device

def test_host_only_handle_refusals():
    from conftest import GOLDEN
    _ffi, lib = _lib()
    h = C.c_void_p()
    path = os.path.join(GOLDEN, "tiny_rb1.onnx").encode()
    assert lib.vits_open_host(path, C.byref(h)) == 0, lib.vits_last_error(None)
    try:
        B, T = 1, 4
        ids = np.array([[3, 4, 5, 6]], np.int64)
        lens = np.array([4], np.int64)
        rows = np.array([[0.667, 1.0, 0.8]], np.float32)
        ctl = _ffi.VitsControls()
        ctl.scales_rows = rows.ctypes.data
        noise = _ffi.VitsNoise()
        st = np.array([[0, 13, 0, 0]], np.float32)
        con = _ffi.VitsContour(st.ctypes.data, None, 0)

        @_ffi.CHUNK_FN
        def never(user, samples, Bc, first, n, total):
            raise AssertionError("not reached")

        def run(c):
            return lib.vits_run_chunked_glided(h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, None, C.byref(noise), C.byref(ctl), C.byref(c), 4,
                                               never, None)

        assert run(con) != 0 and b"token_semitones[0,1]=13" in lib.vits_last_error(h)
        st[0, 1] = 2
        end = np.array([[0, 2, float("nan"), 0]], np.float32)
        assert run(_ffi.VitsContour(st.ctypes.data, end.ctypes.data, 0)) != 0 and b"token_semitones_end[0,2]" in lib.vits_last_error(h)
        dur = np.array([[1, 2, 3, 4]], np.int64)
        ctl.durations = dur.ctypes.data
        assert run(_ffi.VitsContour(st.ctypes.data, None, 1)) != 0 and b"compensate and forced durations" in lib.vits_last_error(h)
        ctl.durations = None
        assert run(con) != 0   # a good call: the handle has no device
        assert b"semitones" not in lib.vits_last_error(h)
    finally:
        lib.vits_close(h)


# ------------------------------------------------------------------ the Python surface

class _Streams(_Recorder):
    """a session whose encoded stream takes the pitch keywords: records them, yields one chunk of zeros per call"""

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None,
                                  token_semitones=None, compensate=True, token_semitones_end=None, **more):
        from phoonnx_amd.session import EncodedChunk
        self.st0, self.st1, self.lens, self.more = token_semitones, token_semitones_end, lens, more
        B = len(lens)
        counts = (3 * lens).astype(np.int32)
        n = int(counts.max())
        yield EncodedChunk(0, np.zeros((B, n), np.int16), counts, np.zeros(B, np.float32), n)


def test_stream_encoded_expands_the_pitch_options():
    from phoonnx_amd.config import SynthesisConfig
    rec = _Streams()
    v = _voice(rec)
    text = "abc. de"
    sizes = [[len(ids) for _, ids in g] for g in v._sentence_groups(text, SynthesisConfig())]
    cfg = SynthesisConfig(normalize_audio=False)
    data = b"".join(v.stream_encoded(text, cfg, pitch_contour=[(0, 0), (1, 4)], phoneme_pitch=-2))
    assert len(data) == 2 * 3 * int(rec.lens.sum())
    for b, s in enumerate(sizes):
        st0, st1 = glide_ref.contour_ids(s, lambda x: 4.0 * x)
        n = sum(s)
        assert np.allclose(rec.st0[b, :n], np.add(st0, -2.0), rtol=0, atol=1e-12)
        assert np.allclose(rec.st1[b, :n], np.add(st1, -2.0), rtol=0, atol=1e-12)
        assert not rec.st0[b, n:].any() and not rec.st1[b, n:].any()
    # phoneme_pitch alone: constant tokens, no end values are passed
    b"".join(v.stream_encoded(text, cfg, phoneme_pitch=3.0))
    assert rec.st1 is None and np.all(rec.st0[0, :sum(sizes[0])] == 3.0)
    # neither: the keywords are not passed at all
    b"".join(v.stream_encoded(text, cfg))
    assert rec.st0 is None and rec.st1 is None


def test_stream_encoded_refusals_are_raised_by_the_call():
    from phoonnx_amd.config import SynthesisConfig
    cfg = SynthesisConfig(normalize_audio=False)
    # a session without the keywords (here: without an encoded stream at all) keeps the refusal, word for word
    v = _voice(_Recorder())
    with pytest.raises(ValueError, match=r"phoneme_pitch is not covered by stream_encoded: the chunked entries have no warped form "
                                         r"\(synthesize_encoded takes it\)"):
        v.stream_encoded("ab", cfg, phoneme_pitch=1.0)
    with pytest.raises(ValueError, match=r"pitch_contour is not covered by stream_encoded: the chunked entries have no warped form "
                                         r"\(synthesize_encoded takes it\)"):
        v.stream_encoded("ab", cfg, pitch_contour=[(0, 1)])

    class Warps(_Recorder):
        """it streams and warps, but does not glide"""
        def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None,
                                      token_semitones=None, compensate=True):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="pitch_contour.*no warped form"):
        _voice(Warps()).stream_encoded("ab", cfg, pitch_contour=[(0, 1)])

    class Rated(_Streams):
        def set_output_rate(self, rate, input_rate=None):
            self.rate = rate

    rated = _voice(Rated(), output_sample_rate=8000)
    with pytest.raises(ValueError, match="phoneme_pitch is not covered with an output rate set"):
        rated.stream_encoded("ab", cfg, phoneme_pitch=1.0)
    with pytest.raises(ValueError, match="pitch_contour is not covered with an output rate set"):
        rated.stream_encoded("ab", cfg, pitch_contour=[(0, 1)])
