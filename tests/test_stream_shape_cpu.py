"""Shaped streaming (include/vitsmi.h, "shaped streaming") without a GPU: the NumPy reference against the limited delivery's,
the timeline, every refusal (Python's checks, the engine's own through the C ABI, no callback made), the exported symbols, the
workspace walk, the plan's host code and the sizes of a streamed run along its schedule in a stand-alone driver (plain and under
the sanitizers), the NumPy fallback, and the voice layer on stand-in sessions.

Reference: tests/stream_shape_ref.py over limit_ref / shape_ref / delivery_ref.  Everything is compared exactly."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import limit_ref as lref
import resample_ref as rref
import shape_ref as sref
import stream_pack_ref as pref
import stream_shape_ref as ref
from conftest import GOLDEN, ROOT
from test_stream_pack_cpu import HOP, TEXT, _Batch, _Ort, _Streams, _voice

from phoonnx_amd import MiSession, SessionError, _ffi
from phoonnx_amd import audio_encoding as ae
from phoonnx_amd import session as ses
from phoonnx_amd.config import SynthesisConfig
from phoonnx_amd.session import EncodedChunk, Limit, RawShapes, RawStreamLimit, Shape

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
F = np.float32


# ------------------------------------------------------------------ the reference and the timeline

def _rows(S=700):
    """four rows under a swell, louder than full scale; NaN behind every row's end"""
    rng = np.random.default_rng(11)
    counts = np.array([S, 333, 1, 0], np.int64)
    t = np.arange(S)
    x = (np.tanh(0.5 * rng.standard_normal((4, S))) * np.sin(2 * np.pi * t / 37.0) * (1.0 + 2.0 * (0.5 - 0.5 * np.cos(2 * np.pi * t / 300.0)))).astype(F)
    for b in range(4):
        x[b, int(counts[b]):] = np.nan
    return x, counts


VOLUME = np.array([1.0, 0.5, 3.0, 1.0], F)
SHAPES = [sref.Shape(50, 80, 1, ((20, 1.0), (300, 0.25), (301, 2.0))), sref.Shape(0, 40, 0, ((0, 2.0), (400, 0.5))), sref.Shape(4, 4, 0, ()), sref.NONE]


def _limits(L):
    return [lref.Limit(0.7, L), None, lref.Limit(0.7, L), lref.Limit(0.5, L)]


def _ses_shapes(shapes):
    return [Shape(s.fade_in, s.fade_out, ("linear", "smooth")[s.curve], list(s.points)) for s in shapes]


def _ses_limits(L):
    return [None if l is None else Limit(l.ceiling, l.lookahead) for l in _limits(L)]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_reference_is_the_limited_delivery_of_whole_rows(encoding):
    x, counts = _rows()
    own = np.array([np.max(np.abs(x[b, :int(counts[b])])) if counts[b] else 0 for b in range(4)], F)
    for ref_peak, norm in ((None, 0), (own, 1)):
        rows, vals = ref.rows_ref(x, counts, encoding, ref_peak, VOLUME, SHAPES, _limits(16))
        segs = [lref.Seg(b, b, 0, norm, float(VOLUME[b])) for b in range(4)]
        want, _, _ = lref.deliver_ref(np.nan_to_num(x), counts, segs, None, None, SHAPES, _limits(16), 4, encoding)
        assert rows == want, norm
    assert 0.05 < lref.over_fraction(ref.unlimited(x[0], 700, None, 1.0, SHAPES[0]), 0.7) < 0.5
    assert max(np.abs(v).max() for v in vals[:1]) <= F(0.7)


@pytest.mark.parametrize("L", [0, 1, 7, 255, 1024])
def test_emit_range_is_the_timeline(L):
    """the library's function, the fallback's and the reference's against a statement of their own: after a piece that renders
    through R, everything below R - L has been delivered - after the last one, everything"""
    pieces = sorted({1, 7, max(L - 1, 1), max(L, 1), L + 1, 2 * L + 1, 5000})      # shorter than, equal to and longer than L
    for total in (1, 999, 5000):
        for piece in pieces:
            done, got = 0, []
            for f, n in pref.pieces(total, piece):
                last = f + n >= total
                upto = total if last else max(f + n - L, 0)
                want = (max(f - L, 0), upto - done)
                assert want[1] == 0 or want[0] == done, (L, piece, f)      # what is delivered begins where the last delivery ended
                assert ses.stream_emit_range(f, n, last, total, L) == want == ref.emit_range(f, n, last, total, L) == ae.emit_range(f, n, last, total, L)
                got.append(want)
                done = upto
            # the delivered ranges tile [0, total) exactly
            pos = 0
            for ef, en in got:
                assert en == 0 or ef == pos
                pos += en
            assert pos == total
            if L and piece <= L and total > piece:
                assert got[0][1] == 0, "a piece inside the look-ahead delivers nothing"
    for bad in ((-1, 4, 0, 10, 0), (0, 4, 0, 3, 0), (0, 4, 0, 10, -1), (0, 4, 0, 10, 1025)):
        with pytest.raises(SessionError, match="bad emit range"):
            ses.stream_emit_range(*bad)


# ------------------------------------------------------------------ refusals

NAN, INF = float("nan"), float("inf")
# words of the message -> stream_shaping_check's arguments
REFUSALS = [
    ("row 1: fade_in -1", dict(shapes=RawShapes([(0, 0, 0, 0, 0), (-1, 0, 0, 0, 0)], []), B=2)),
    ("row 0: fade_out -3", dict(shapes=RawShapes([(0, -3, 0, 0, 0)], []), B=1)),
    ("row 1: curve 2", dict(shapes=RawShapes([(0, 0, 0, 0, 0), (0, 0, 2, 0, 0)], []), B=2)),
    ("row 0: n_points -1", dict(shapes=RawShapes([(0, 0, 0, -1, 0)], []), B=1)),
    ("row 1: points [1, +2)", dict(shapes=RawShapes([(0, 0, 0, 0, 0), (0, 0, 0, 2, 1)], [(0, 1.0), (5, 1.0)]), B=2)),
    ("row 0: point 1: pos 3 does not ascend", dict(shapes=RawShapes([(0, 0, 0, 2, 0)], [(3, 1.0), (3, 0.5)]), B=1)),
    ("row 0: point 0: gain 65", dict(shapes=RawShapes([(0, 0, 0, 1, 0)], [(3, 65.0)]), B=1)),
    ("row 0: point 0: gain nan", dict(shapes=RawShapes([(0, 0, 0, 1, 0)], [(3, NAN)]), B=1)),
    ("row 0: point 0: pos -1", dict(shapes=RawShapes([(0, 0, 0, 1, 0)], [(-1, 1.0)]), B=1)),
    ("lookahead -1 outside [0, 1024]", dict(limit=RawStreamLimit(-1, None), B=2)),
    ("lookahead 1025 outside [0, 1024]", dict(limit=RawStreamLimit(1025, [0.5, 0.5]), B=2)),
    ("row 1: limit ceiling 1.5", dict(limit=RawStreamLimit(16, [0.5, 1.5]), B=2)),
    ("row 0: limit ceiling -0.25", dict(limit=RawStreamLimit(16, [-0.25, 0.5]), B=2)),
    ("row 1: limit ceiling nan", dict(limit=RawStreamLimit(16, [0.5, NAN]), B=2)),
    ("row 2: limit ceiling inf", dict(limit=RawStreamLimit(16, [0.0, 0.5, INF]), B=3)),
    ("row 1: volume 1500", dict(limit=RawStreamLimit(16, [0.0, 0.5]), B=2, volume=[1500.0, 1500.0])),
    ("row 0: volume -1024.5", dict(limit=Limit(0.5, 16), B=1, volume=[-1024.5])),
]


@pytest.mark.parametrize("word,kw", REFUSALS)
def test_every_refusal_names_the_row_and_the_value(word, kw):
    with pytest.raises(SessionError) as ei:
        ses.stream_shaping_check(**kw)
    assert word in str(ei.value), str(ei.value)


def test_what_is_not_refused():
    ses.stream_shaping_check()                                                        # no shaping at all
    ses.stream_shaping_check(shapes=Shape(3, 3, "smooth", [(0, 0.0), (9, 64.0)]), limit=Limit(1.0, 1024), B=3, volume=1024.0)
    ses.stream_shaping_check(limit=RawStreamLimit(0, [0.0, 0.5]), B=2, volume=[5000.0, 5000.0])   # no look-ahead: no limited row
    ses.stream_shaping_check(limit=[Limit(0.5, 16), None], B=2, volume=[1.0, 5000.0])             # the loud row is not limited
    with pytest.raises(SessionError, match="one lookahead"):
        ses.stream_shaping_check(limit=[Limit(0.5, 16), Limit(0.5, 17)], B=2)


@pytest.fixture(scope="module")
def host_session():
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    yield s
    s.close()


IDS = np.ones((2, 6), np.int64)
LENS = np.array([6, 4], np.int64)
SC = np.array([0.667, 1.0, 0.8], F)


def test_bad_shapings_are_named_before_the_handle_is_touched(host_session):
    z = np.zeros((2, host_session.hparam("inter"), 5), F)
    for word, kw in (("row 0: limit ceiling 2", dict(limit=Limit(2.0, 16))), ("lookahead 4000", dict(limit=Limit(0.5, 4000))),
                     ("row 1: fade_out -2", dict(shapes=[Shape(), Shape(0, -2)])), ("one lookahead", dict(limit=[Limit(0.5, 1), Limit(0.5, 2)])),
                     ("row 1: volume 2000", dict(limit=Limit(0.5, 16), volume=[1.0, 2000.0]))):
        for call in (lambda: host_session.synthesize_stream_encoded(IDS, LENS, SC, **kw), lambda: host_session.vocoder_stream_encoded(z, **kw)):
            with pytest.raises(SessionError) as ei:
                call()          # (raised by the call itself, not by the first next(): nothing was started)
            assert word in str(ei.value) and "host-only" not in str(ei.value), str(ei.value)
    with pytest.raises(SessionError, match="explicit points"):
        host_session.synthesize_stream_encoded(IDS, LENS, SC, shapes=Shape(0, 0, "linear", [(1, 0.5)]), token_gain_db=np.zeros((2, 6)))
    with pytest.raises(SessionError, match=r"token_gain_db\[1\]\[2\]"):
        host_session.synthesize_stream_encoded(IDS, LENS, SC, token_gain_db=np.where(np.arange(12).reshape(2, 6) == 8, 99.0, 0.0))
    # a valid shaping reaches the handle, and only then does a host-only handle refuse to run
    for kw in (dict(shapes=Shape(3, 3)), dict(limit=Limit(0.5, 110)), dict(token_gain_db=np.zeros((2, 6)), limit=[Limit(0.5, 7), None])):
        with pytest.raises(SessionError, match="host-only"):
            list(host_session.synthesize_stream_encoded(IDS, LENS, SC, **kw))


def test_the_engine_refuses_the_same_without_a_callback(host_session):
    lib, h = host_session._lib, host_session._h
    calls = []

    @_ffi.ENC_CHUNK_FN
    def cb(*args):
        calls.append(args)
        return 0

    @_ffi.STREAM_PLAN_FN
    def plan(*args):
        calls.append(args)
        return 0

    rows = np.tile(SC, (2, 1))
    ctl = _ffi.VitsControls()
    ctl.scales_rows = rows.ctypes.data
    noise = _ffi.VitsNoise()
    z = np.zeros((2, host_session.hparam("inter"), 5), F)
    fmt = _ffi.VitsStreamFormat()
    vol = np.array([1.0, 3000.0], F)
    fmt.volume = vol.ctypes.data

    def both(shp):
        p = None if shp is None else C.byref(shp)
        yield lib.vits_run_chunked_enc_shaped(h, _ffi.ptr(IDS), _ffi.ptr(LENS), 2, 6, None, C.byref(noise), C.byref(ctl), C.byref(fmt), p, 4, cb, None)
        yield lib.vits_run_vocoder_chunked_enc_shaped(h, _ffi.ptr(z), 2, 5, None, C.byref(fmt), p, 4, cb, None)

    for word, limit in (("lookahead 1025", RawStreamLimit(1025, None)), ("row 0: limit ceiling 1.25", RawStreamLimit(8, [1.25, 0.5])),
                        ("row 1: volume 3000", RawStreamLimit(8, [0.0, 0.5]))):
        shp = ses._stream_shaping(None, limit, 2)
        shp.plan = plan
        for rc in both(shp):
            assert rc == -3 and word in host_session._err(), (word, rc, host_session._err())
    shp = ses._stream_shaping(RawShapes([(0, 0, 0, 0, 0), (0, 0, 7, 0, 0)], []), None, 2)
    for rc in both(shp):
        assert rc == -3 and "row 1: curve 7" in host_session._err()
    # the format is looked at first; a shaping that passes - or none - reaches the device check
    assert lib.vits_run_chunked_enc_shaped(h, _ffi.ptr(IDS), _ffi.ptr(LENS), 2, 6, None, C.byref(noise), C.byref(ctl), None, C.byref(shp), 4, cb,
                                           None) == -3 and "null stream format" in host_session._err()
    good = ses._stream_shaping([Shape(3, 3), Shape()], RawStreamLimit(8, [0.5, 0.0]), 2)
    for shp in (good, None):
        for rc in both(shp):
            assert rc != 0 and "host-only" in host_session._err()
    assert calls == []


def test_symbols_and_struct_sizes():
    lib = _ffi.load()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_stream_shaping_check", "vits_stream_emit_range", "vits_run_chunked_enc_shaped", "vits_run_vocoder_chunked_enc_shaped",
                 "vits_test_stream_pack_shaped"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsStreamShaping) == 56 and _ffi.VitsStreamShaping.lookahead.offset == 32 and _ffi.VitsStreamShaping.plan.offset == 40
    assert "/* 56 bytes */" in header and "vits_stream_plan_fn" in header
    # the sections that used to leave the stream out point to it now
    assert "a fade-out cannot know where the stream ends" not in header and "adds latency: a later change" not in header


def test_the_test_hook_checks_its_sizes_on_the_host():
    lib = _ffi.load()
    x, counts = _rows(96)
    counts = np.minimum(counts, 96)
    fmt = _ffi.VitsStreamFormat()
    out = np.zeros(4 * 16 * 96, np.uint8)
    pitches, firsts, ns = np.zeros(96, np.int64), np.zeros(96, np.int64), np.zeros(96, np.int64)
    valid, peaks = np.zeros((96, 4), np.int32), np.zeros((96, 4), F)

    def hook(shp=None, piece=16, cap=out.nbytes, max_pieces=96, S=96, firsts=firsts):
        return lib.vits_test_stream_pack_shaped(0, _ffi.ptr(x), _ffi.ptr(counts), 4, S, piece, C.byref(fmt), None if shp is None else C.byref(shp),
                                                _ffi.ptr(out), cap, _ffi.ptr(pitches), _ffi.ptr(valid), _ffi.ptr(peaks), _ffi.ptr(firsts),
                                                _ffi.ptr(ns), max_pieces)

    for word, kw in (("bad stream pack test arguments", dict(piece=0)), ("bad stream pack test arguments", dict(firsts=None)),
                     ("lookahead 2000", dict(shp=ses._stream_shaping(None, RawStreamLimit(2000, None), 4))),
                     ("6 pieces", dict(max_pieces=5)), ("room for", dict(cap=4 * 32 * 6 - 1, shp=ses._stream_shaping(None, Limit(0.5, 8), 4)))):
        assert hook(**kw) == -3 and word in _ffi.last_error(None), (word, _ffi.last_error(None))
    assert not out.any()


# ------------------------------------------------------------------ the workspace walk and the plan's host code

def _build(exe, *flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", *flags, "-I" + csrc, os.path.join(ROOT, "tests", "stream_shape_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_shape") / "stream_shape_driver")
    _build(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_the_shaped_stream_workspace_is_the_size_its_walk_carves(driver):
    walks = [ln.split() for ln in driver if ln.startswith("walk ")]
    assert len(walks) == 4 * 5 * 4
    size = {}
    for _, b, n, L, knots, verdict, *rest in walks:
        assert verdict == "A", (b, n, L, rest)
        size[int(b), int(n), int(L)] = (int(knots),) + tuple(int(v) for v in rest)
    for (b, n, L), (knots, alone, behind) in size.items():
        # the chunk of n + L samples as F32 at a 16-byte row pitch, the peaks in whole cells, two floats per row; then a 32-byte
        # record per row, a 16-byte knot each, two carries of 2 L floats per row - each at the next 256-byte boundary
        pack = b * (-(-4 * (n + L) // 16) * 16) + -(-4 * b // 16) * 16 + 8 * b
        need = pack + 32 * b + 16 * knots + 2 * (8 * L * b)
        assert need <= alone <= need + 5 * 256, (b, n, L, alone, need)
        assert behind >= alone + 10 * b * (n + L + 5)
        assert alone >= size[b, n, 0][1] and (L == 1024 or alone <= size[b, n, 1024][1])
    tables = [ln for ln in driver if ln.startswith("table ")]
    assert tables == ["table 3 7 0 1 2 ok", "table 2 2 0 1 ok"]        # knots: a row's points and one more


def test_the_driver_states_the_timeline(driver):
    emits = [ln.split() for ln in driver if ln.startswith("emit ")]
    assert len(emits) == 5 * 7 * 3
    for _, L, piece, total, *vals in emits:
        L, piece, total = int(L), int(piece), int(total)
        got = list(zip(map(int, vals[0::2]), map(int, vals[1::2])))
        assert got == ref.timeline(pref.pieces(total, piece), total, L), (L, piece, total)


def _completed(P, fi, fo, total):
    """output samples whose K inputs all lie in front of input position P, by the definition: sample j reads the inputs up to
    floor(j * M / L) + K / 2"""
    L, M, K = rref.plan(fi, fo)[:3]
    last_input = np.arange(total, dtype=np.int64) * M // L + K // 2
    return int(np.searchsorted(last_input, P - 1, side="right"))


def test_the_sizes_of_a_streamed_run_hold_along_its_schedule(driver):
    """stream_n_max / stream_ring_bytes (workspace.hpp) against the schedule restated here: chunks of frames are pieces of input
    samples, an output rate completes what the definition says, a look-ahead delivers the timeline of what was completed.
    Every delivered range is what this says, none exceeds n_max, and a chunk of n_max samples fits a ring slot."""
    B, FI = 3, 22050
    scheds = [ln.split() for ln in driver if ln.startswith("sched ")]
    assert len(scheds) == 3 * 4 * 4 * 5 * 4 and all("bad" not in s for s in scheds)
    seen, empty_completions = set(), 0
    for _, hop, chunk, F, fo, L, total, n_max, ring_f, ring1, ring2, ring4, *vals in scheds:
        hop, chunk, F, fo, L, total, n_max = (int(v) for v in (hop, chunk, F, fo, L, total, n_max))
        seen.add((hop, chunk, F, fo, L))
        got = list(zip(map(int, vals[0::2]), map(int, vals[1::2])))
        rendered = pref.pieces(F * hop, chunk * hop)
        assert len(got) == len(rendered) == -(-F // chunk)
        if fo:
            assert total == int(rref.count(F * hop, FI, fo))
            done, completed = 0, []
            for f, n in rendered:
                upto = total if f + n == F * hop else _completed(f + n, FI, fo, total)
                completed.append((done, upto - done))
                done = upto
            empty_completions += sum(1 for _, n in completed if n == 0)
        else:
            assert total == F * hop
            completed = rendered
        live = [p for p in completed if p[1]]
        want = iter(ref.timeline(live, total, L))
        assert got == [next(want) if n else (f, 0) for f, n in completed], (hop, chunk, F, fo, L)
        # what is delivered tiles [0, total), piece by piece
        pos = 0
        for first, n in got:
            assert n == 0 or first == pos, (hop, chunk, F, fo, L)
            assert 0 <= n <= n_max, (hop, chunk, F, fo, L, n, n_max)
            pos += n
        assert pos == total and n_max <= total
        # a slot of the ring holds the largest chunk with the rows' peaks behind it; a float sink's (no look-ahead) its rows
        for w, ring in ((1, ring1), (2, ring2), (4, ring4)):
            assert B * (-(-w * n_max // 16) * 16) + 4 * B <= int(ring), (hop, chunk, F, fo, L, w)
        if L == 0:
            assert B * 4 * max(n for _, n in got) <= int(ring_f)
    assert len(seen) == len(scheds)
    # (hop 1 and hop 64 in chunks of one frame are shorter than every filter's half length: the grid holds such chunks)
    assert empty_completions > 0


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, driver):
    """The stand-alone program itself, built with -fsanitize=address,undefined (nothing loaded into Python is sanitised)."""
    exe = str(tmp_path / "stream_shape_driver_san")
    _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.splitlines() == driver


# ------------------------------------------------------------------ the NumPy fallback

@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_fallback_gives_the_reference_chunks(encoding):
    x, counts = _rows()
    S = x.shape[1]
    own = np.array([np.max(np.abs(x[b, :int(counts[b])])) if counts[b] else 0 for b in range(4)], F)
    w = ref.WIDTH[encoding]
    for L, piece, ref_peak in ((0, 40, None), (1, 7, None), (16, 7, own), (16, 40, None), (255, 100, own), (255, S, None), (1024, 256, None)):
        limits = _limits(L) if L else None
        want, ranges = ref.stream_ref(x, counts, pref.pieces(S, piece), encoding, ref_peak, VOLUME, SHAPES, limits, L)
        fp32 = [(f, x[:, f:f + n], S) for f, n in pref.pieces(S, piece)]
        got = list(ae.stream_shaped(fp32, lambda: counts, encoding, ref_peak, VOLUME, _ses_shapes(SHAPES), _ses_limits(L) if L else None))
        assert [(g[0], g[1].shape[1]) for g in got] == [r for r in ranges if r[1]], (L, piece)
        for g, c in zip(got, want):
            assert np.array_equal(g[2], c.valid) and g[4] == S and g[1].dtype == np.dtype(ref.DTYPE[encoding])
            assert [g[1][b].tobytes() for b in range(4)] == [c.data[b][:w * c.n] for b in range(4)], (L, piece, c.first)
            assert np.array_equal(g[3].view(np.uint32), c.peak.view(np.uint32))
        rows, _ = ref.rows_ref(x, counts, encoding, ref_peak, VOLUME, SHAPES, limits)
        assert [b"".join(g[1][b, :int(g[2][b])].tobytes() for g in got) for b in range(4)] == rows
    with pytest.raises(ValueError, match="one lookahead"):
        list(ae.stream_shaped([(0, x, S)], counts, encoding, limits=[Limit(0.5, 3), Limit(0.5, 4), None, None]))


# ------------------------------------------------------------------ the voice layer on stand-in sessions

class _StreamsShaped(_Streams):
    """a session that streams encoded chunks and knows the shaping keywords: the reference applied to the same waveforms"""

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None,
                                  shapes=None, limit=None):
        r = self.synthesize_batch(ids, lens, scales, sid)
        B = ids.shape[0]
        counts = r["y_lengths"] * self.HOP
        total = int(counts.max())
        self.asked = getattr(self, "asked", []) + [(shapes, limit)]
        vol = None if volume is None else np.broadcast_to(F(volume), (B,))
        sh = None if shapes is None else [sref.Shape(shapes.fade_in, shapes.fade_out, ("linear", "smooth").index(shapes.curve), ())] * B
        lim = None if limit is None else [lref.Limit(limit.ceiling, limit.lookahead)] * B
        chunks, _ = ref.stream_ref(r["output"][:, 0, 0, :total], counts, pref.pieces(total, chunk_frames * self.HOP), encoding, ref_peak, vol, sh,
                                   lim, 0 if limit is None else limit.lookahead)
        for c in chunks:
            w = ref.WIDTH[encoding]
            yield EncodedChunk(c.first, np.stack([np.frombuffer(row[:w * c.n], ref.DTYPE[encoding]) for row in c.data]), c.valid, c.peak, total)


class _StreamsEncodedOld(_Streams):
    """... and one from before the shaped stream: it does not know the keywords"""

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None):
        yield from _StreamsShaped.synthesize_stream_encoded(self, ids, lens, scales, sid, chunk_frames, encoding, ref_peak, volume)


SESSIONS = {"run only": _Ort, "whole batches": _Batch, "fp32 chunks": _Streams, "shaped chunks": _StreamsShaped}
KEYWORDS = [dict(fade_in=0.001, fade_out=0.002, limit_ceiling=0.1, limit_lookahead=0.0005), dict(fade_out=0.001, fade_curve="smooth"),
            dict(limit_ceiling=0.15, limit_lookahead=0.001)]


@pytest.mark.parametrize("kind", sorted(SESSIONS))
@pytest.mark.parametrize("encoding", ["pcm16", "alaw"])
def test_stream_encoded_joined_is_synthesize_encoded(encoding, kind):
    """at 16 kHz: fades of 16 and 32 samples, a look-ahead of 8 or 16 samples, chunks of 3, 15 and 192 samples"""
    raw = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=False)
    whole = _voice(_Batch())
    plain = whole.synthesize_encoded(TEXT, raw, encoding=encoding, sentence_silence=0.05).data.tobytes()
    for kw in KEYWORDS:
        want = whole.synthesize_encoded(TEXT, raw, encoding=encoding, sentence_silence=0.05, **kw).data.tobytes()
        assert want != plain, kw
        for chunk_frames in (1, 5, 64):
            voice = _voice(SESSIONS[kind]())
            got = list(voice.stream_encoded(TEXT, raw, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=0.05, **kw))
            assert all(isinstance(p, bytes) and p for p in got) and b"".join(got) == want, (kind, kw, chunk_frames)
        if kind == "shaped chunks":     # the device path was asked for exactly what the keywords say
            shapes, limit = voice.session.asked[-1]
            assert (shapes is None) == ("fade_in" not in kw and "fade_out" not in kw) and (limit is None) == ("limit_ceiling" not in kw)
            if limit is not None:
                assert limit.lookahead == int(round(kw["limit_lookahead"] * 16000)) and limit.ceiling == kw["limit_ceiling"]


def test_keywords_are_passed_down_only_when_asked_for():
    raw = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=False)
    voice = _voice(_StreamsEncodedOld())
    want = _voice(_Batch()).synthesize_encoded(TEXT, raw).data.tobytes()
    assert b"".join(voice.stream_encoded(TEXT, raw, chunk_frames=5)) == want        # an older session keeps working
    with pytest.raises(TypeError):
        list(voice.stream_encoded(TEXT, raw, fade_in=0.001))                          # ... and says so when it is asked for more
    for kw, word in ((dict(limit_ceiling=1.5), "limit_ceiling"), (dict(limit_ceiling=0.5, limit_lookahead=1.0), "limit_lookahead"),
                     (dict(fade_in=-1.0), "fade_in"), (dict(fade_curve="cubic"), "fade_curve")):
        with pytest.raises(ValueError, match=word):
            voice.stream_encoded(TEXT, raw, **kw)                                     # (raised by the call itself)
    with pytest.raises(ValueError, match="durations"):
        _voice(_Ort()).stream_encoded(TEXT, raw, phoneme_gain_db=lambda k, toks: [0.0] * len(toks))
