"""Shaped streaming on the GPU (include/vitsmi.h, "shaped streaming"): the two kernels and the carry by value through
vits_test_stream_pack_shaped, then the feature through MiSession and TTSVoice.

Reference: tests/stream_shape_ref.py - whole rows through limit_ref / shape_ref / delivery_ref, cut by the timeline.  Every
comparison is on bytes or float bits; no tolerance anywhere."""
import os
import threading

import numpy as np
import pytest

import limit_ref as lref
import shape_ref as sref
import stream_pack_ref as pref
import stream_shape_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
LOOKAHEADS = (1, 7, 255, 1024)
PIECES = (7, 40, 256, 1000, 5000)
B, S, CEILING = 5, 5000, 0.7
COUNTS = np.array([5000, 4097, 1, 0, 2500], np.int64)
VOLUME = np.array([1.0, 0.5, 3.0, 1.0, 0.5], np.float32)
CEILINGS = (CEILING, CEILING, CEILING, CEILING, 0.0)           # row 4 is not limited
TILE = 2048                                                     # delivered elements of a workgroup of the limited kernel
# fades and breakpoints under the limiter: a row with both, one with points only, the row of one sample with fades that overlap
SHAPES = [sref.Shape(300, 500, 1, ((100, 1.0), (900, 0.25), (901, 2.0), (4000, 1.0))), sref.Shape(0, 0, 0, ((0, 2.0), (4096, 0.5))),
          sref.Shape(4, 4, 0, ()), sref.NONE, sref.Shape(64, 64, 0, ())]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _signal():
    """limit_ref.batch's signal - tanh(0.5 * noise) * sin under a swell to three times the level - at 5000 samples a row, NaN
    behind every row's end"""
    x = lref.batch()[:, :S].copy()
    for b in range(B):
        x[b, int(COUNTS[b]):] = np.nan
    return x


X = _signal()


def _pieces(L):
    return [p for p in PIECES if p != 7 or L <= 7]


def _limits(L, ceilings=CEILINGS):
    return [lref.Limit(c, L) if c else None for c in ceilings]


def _session_shapes(shapes):
    from phoonnx_amd.session import Shape
    return [Shape(s.fade_in, s.fade_out, ("linear", "smooth")[s.curve], list(s.points)) for s in shapes]


def _session_limit(L, ceilings=CEILINGS):
    from phoonnx_amd.session import Limit
    return [Limit(c, L) if c else None for c in ceilings]


_ROWS = {}


def _rows(encoding, L, ref_peak=None, shapes=SHAPES, ceilings=CEILINGS, volume=VOLUME):
    """the reference rows of a configuration, computed once"""
    key = (encoding, L, None if ref_peak is None else tuple(ref_peak), id(shapes), ceilings, tuple(volume))
    if key not in _ROWS:
        _ROWS[key] = ref.rows_ref(X, COUNTS, encoding, ref_peak, volume, shapes, _limits(L, ceilings) if L else None)
    return _ROWS[key]


def _joined(chunks, b, w):
    return b"".join(c.data[b].tobytes()[:w * int(c.valid[b])] for c in chunks)


def _check(got, ranges, piece, encoding, L, rows, what):
    """delivered chunks against the reference rows: ranges, layout, valid, silence behind the rows' ends, the running peaks,
    the joined rows"""
    w = ref.WIDTH[encoding]
    want_ranges = ref.timeline(pref.pieces(S, piece), S, L)
    assert ranges == want_ranges, (what, ranges[:4], want_ranges[:4])
    live = [(f, n, r) for (f, n), r in zip(pref.pieces(S, piece), want_ranges) if r[1]]
    assert len(got) == len(live), what
    pos = 0
    for c, (first, n, (ef, en)) in zip(got, live):
        assert c.first_sample == ef == pos and c.data.shape == (B, ref.pitch_of(en, encoding)), (what, ef)
        assert np.array_equal(c.valid, np.clip(COUNTS - ef, 0, en)), (what, ef)
        for b in range(B):
            pad = c.data[b].tobytes()[w * int(c.valid[b]):]
            assert pad == ref.SILENCE[encoding] * (len(pad) // w), (what, ef, b)
        seen = np.minimum(COUNTS, first + n)
        peak = np.array([np.max(np.abs(X[b, :int(seen[b])])) if seen[b] else 0 for b in range(B)], np.float32)
        assert np.array_equal(_bits(c.peak), _bits(peak)), (what, ef, c.peak, peak)
        pos += en
    assert pos == S
    for b in range(B):
        mine = _joined(got, b, w)
        if mine != rows[b]:
            a, d = np.frombuffer(mine, np.uint8), np.frombuffer(rows[b], np.uint8)
            bad = np.flatnonzero(a != d) if a.size == d.size else None
            raise AssertionError(f"{what} row {b}: {len(mine)} / {len(rows[b])} bytes, "
                                 f"{'sizes differ' if bad is None else f'{bad.size} differ, first at {bad[:8] // w}'}")


def test_the_inputs_exercise_what_can_go_wrong():
    """On the reference alone (no GPU work: it guards the case itself)."""
    for L in LOOKAHEADS:
        u = [ref.unlimited(X[b], int(COUNTS[b]), None, VOLUME[b], SHAPES[b]) for b in range(B)]
        unshaped = [ref.unlimited(X[b], int(COUNTS[b]), None, 1.0, None) for b in range(B)]
        for b in (0, 1):   # the long limited rows
            frac = lref.over_fraction(u[b], CEILING)
            print(f"L={L} row {b}: {100 * frac:.1f} % of the samples exceed the ceiling ({100 * lref.over_fraction(unshaped[b], CEILING):.1f} % unshaped)")
            assert 0.05 <= frac <= 0.50, (b, frac)
        over = np.flatnonzero(np.abs(u[0]) > np.float32(CEILING))
        seen = set()
        for piece in _pieces(L):
            ranges = ref.timeline(pref.pieces(S, piece), S, L)
            assert sum(n for _, n in ranges) == S
            edges = np.arange(piece, S, piece)
            if edges.size and (np.abs(over[None, :] - edges[:, None]) <= L).any():
                seen.add("a piece boundary within L of a sample above the ceiling")
            if any(n == 0 for _, n in ranges):
                seen.add("a piece delivers nothing")
            if piece < 2 * L:
                seen.add("a piece shorter than the carry")
            for ef, en in ranges:
                for c in COUNTS:
                    v = min(max(int(c) - ef, 0), en)
                    if 0 < v < en and (v % TILE) and en > TILE:
                        seen.add("a row ends inside a tile")
                    if 0 < v < en and v % 16:
                        seen.add("a row ends inside a 16-byte cell")
                    if en and c <= ef:
                        seen.add("a row ended before the piece")
        want = {"a piece boundary within L of a sample above the ceiling", "a row ends inside a tile", "a row ends inside a 16-byte cell",
                "a row ended before the piece"}
        if L >= 7:
            want |= {"a piece delivers nothing", "a piece shorter than the carry"}
        assert want <= seen, (L, want - seen)
    assert set(VOLUME.tolist()) == {1.0, 0.5, 3.0} and CEILINGS.count(0.0) == 1


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("L", LOOKAHEADS)
def test_limited_kernel_by_value(L, encoding):
    from phoonnx_amd.session import test_stream_pack_shaped
    rows, vals = _rows(encoding, L)
    first = None
    for piece in _pieces(L):
        got, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, volume=VOLUME, shapes=_session_shapes(SHAPES),
                                              limit=_session_limit(L))
        _check(got, ranges, piece, encoding, L, rows, f"{encoding}/L={L}/{piece}")
        mine = [_joined(got, b, ref.WIDTH[encoding]) for b in range(B)]
        first = first or mine
        assert mine == first, (encoding, L, piece, "the joined rows depend on the piece size")
    if encoding == "f32":   # no delivered sample of a limited row exceeds its ceiling; the unlimited row does clip
        for b in range(4):
            v = np.frombuffer(first[b], "<f4")
            assert not np.isnan(v).any() and (np.abs(v) <= np.float32(CEILING)).all(), b
        assert np.abs(np.frombuffer(first[4], "<f4")).max() > CEILING
        # a faded row starts and ends at exactly 0, under the limiter too
        for b in (0, 2, 4):
            v = np.frombuffer(first[b], "<f4")
            assert v[0] == 0 and v[-1] == 0, b


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_reference_peaks_on_either_side_of_the_threshold(encoding):
    from phoonnx_amd.session import test_stream_pack_shaped
    own = np.array([np.max(np.abs(X[b, :int(COUNTS[b])])) if COUNTS[b] else 0 for b in range(B)], np.float32)
    peaks = np.array([own[0], 1e-9, 2e-8, 1.0, own[4]], np.float32)
    for L, piece in ((7, 40), (255, 1000)):
        rows, _ = _rows(encoding, L, ref_peak=peaks)
        got, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, ref_peak=peaks, volume=VOLUME, shapes=_session_shapes(SHAPES),
                                              limit=_session_limit(L))
        _check(got, ranges, piece, encoding, L, rows, f"{encoding}/L={L}/{piece}/ref_peak")
    assert rows[1] == ref.SILENCE[encoding] * int(COUNTS[1])       # below the threshold: silence
    # the row normalised by its own peak is the limited delivery's normalize 1
    segs = [lref.Seg(b, b, 0, 1, float(VOLUME[b])) for b in range(B)]
    want, _, _ = lref.deliver_ref(np.nan_to_num(X), COUNTS, segs, None, None, SHAPES, _limits(255), B, encoding)
    assert rows[0] == want[0] and rows[4] == want[4]


FADES = [sref.Shape(300, 500, 1, ()), sref.Shape(1, 4096, 0, ()), sref.Shape(4, 4, 0, ()), sref.Shape(10, 10, 1, ()), sref.NONE]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_fades_only(encoding):
    """L = 0: the shaped kernel; the timeline is the unshaped stream's"""
    from phoonnx_amd.session import test_stream_pack_shaped
    rows, _ = _rows(encoding, 0, shapes=FADES)
    w = ref.WIDTH[encoding]
    for piece in (7, 40, 256, 1000, 5000):
        got, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, volume=VOLUME, shapes=_session_shapes(FADES))
        assert ranges == pref.pieces(S, piece)
        _check(got, ranges, piece, encoding, 0, rows, f"{encoding}/fades/{piece}")
    for b in (0, 1, 2):    # the first and last valid samples of a faded row encode exactly 0 (row 2: fades that overlap on one sample)
        ends = np.frombuffer(rows[b][:w] + rows[b][-w:], ref.DTYPE[encoding])
        if encoding == "f32":      # (a negative sample times 0 is -0.0f: a zero all the same)
            assert (ends == 0).all(), b
        else:
            assert ends.tobytes() == 2 * ref.SILENCE[encoding], b
        assert len(rows[b]) == w * COUNTS[b], b
    assert rows[3] == b""


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_no_shaping_is_the_unshaped_stream(encoding):
    from phoonnx_amd.session import test_stream_pack, test_stream_pack_shaped
    for piece in (40, 1000):
        plain = test_stream_pack(X, COUNTS, piece, encoding, volume=VOLUME)
        got, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, volume=VOLUME)
        assert ranges == pref.pieces(S, piece) and len(got) == len(plain)
        for g, p in zip(got, plain):
            assert g.first_sample == p.first_sample and g.data.tobytes() == p.data.tobytes()
            assert np.array_equal(g.valid, p.valid) and np.array_equal(_bits(g.peak), _bits(p.peak))


@pytest.mark.parametrize("encoding", ["pcm16", "f32"])
def test_a_ceiling_nothing_reaches_is_the_shaped_stream_delayed(encoding):
    """|u| <= 0.3 * 3 * 2 < 1 everywhere... the volumes are made small enough for ceiling 1.0: g = 1.0f by the rule, so the
    bytes are the shaped stream's (L = 0), re-cut to the delayed timeline"""
    from phoonnx_amd.session import test_stream_pack_shaped
    quiet = (VOLUME * np.float32(0.05)).astype(np.float32)
    u_max = max(np.abs(ref.unlimited(X[b], int(COUNTS[b]), None, quiet[b], SHAPES[b])).max() for b in (0, 1, 2, 4))
    assert u_max < 1.0
    w = ref.WIDTH[encoding]
    shaped, _ = test_stream_pack_shaped(X, COUNTS, 1000, encoding, volume=quiet, shapes=_session_shapes(SHAPES))
    rows = [_joined(shaped, b, w) for b in range(B)]
    for L, piece in ((7, 40), (1024, 256)):
        got, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, volume=quiet, shapes=_session_shapes(SHAPES),
                                              limit=_session_limit(L, (1.0, 1.0, 1.0, 1.0, 0.0)))
        cut = ref.recut(rows, COUNTS, ranges, encoding)
        assert len(cut) == len(got)
        for g, want in zip(got, cut):
            for b in range(B):
                assert g.data[b].tobytes()[:w * int(g.valid[b])] == want[b], (L, piece, g.first_sample, b)


def test_two_runs_give_the_same_bytes():
    from phoonnx_amd.session import test_stream_pack_shaped
    runs = [test_stream_pack_shaped(X, COUNTS, 256, "ulaw", volume=VOLUME, shapes=_session_shapes(SHAPES), limit=_session_limit(255))
            for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.data.tobytes() == b.data.tobytes() and np.array_equal(_bits(a.peak), _bits(b.peak))


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
LOOK = 110


def _shaping():
    from phoonnx_amd.session import Limit, Shape
    shapes = [Shape(100, 200, "smooth"), Shape(0, 150, "linear", [(0, 1.5), (800, 0.5)]), Shape(50, 50)]
    return shapes, [Limit(0.5, LOOK), None, Limit(0.3, LOOK)]


def _joined_rows(chunks, B=3):
    return [b"".join(c.data[b, :int(c.valid[b])].tobytes() for c in chunks) for b in range(B)]


def _check_timeline(chunks, plain_ranges, counts, encoding, L):
    """the chunks of a shaped stream against the ranges of the unshaped one: the delayed timeline, valid, silence, peaks"""
    total = int(counts.max())
    want = [r for r in ref.timeline(plain_ranges, total, L) if r[1]]
    assert [(c.first_sample, c.data.shape[1]) for c in chunks] == want
    assert sum(n for _, n in want) == total
    for c in chunks:
        n = c.data.shape[1]
        assert c.total_samples == total and np.array_equal(c.valid, np.clip(counts - c.first_sample, 0, n))
        for b in range(len(counts)):
            assert c.data[b, int(c.valid[b]):].tobytes() == ref.SILENCE[encoding] * (n - int(c.valid[b]))
    peaks = np.stack([c.peak for c in chunks])
    assert (np.diff(peaks, axis=0) >= 0).all() and not np.isnan(peaks).any()


@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("chunk_frames", [1, 3, 64])
@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_shaped_stream_of_a_run(preset, chunk_frames, rate):
    s = _session(preset, output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    shapes, limits = _shaping()
    enc = ENCODINGS[(chunk_frames + (rate is not None)) % 4]
    kw = dict(encoding=enc, volume=VOL3, seeds=seeds)
    want = s.synthesize_delivered(ids, lens, scales, sid, normalize=False, shapes=shapes, limits=limits, **kw)
    counts = np.asarray(want["sample_lengths"], np.int64)
    assert len(set(counts.tolist())) == 3      # (at 8000 Hz the shortest row is shorter than the carry of 2 L samples)
    plain = [(c.first_sample, c.data.shape[1]) for c in s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, **kw)]
    chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shapes, limit=limits, **kw))
    _check_timeline(chunks, plain, counts, enc, LOOK)
    assert _joined_rows(chunks) == [a.tobytes() for a in want["streams"]], (preset, chunk_frames, rate, "normalize 0")
    if chunk_frames == 1:
        assert len(chunks) < len(plain), "no piece lies inside the look-ahead"
    assert np.array_equal(s.last_sample_counts(), counts)
    # fades only: the unshaped stream's timeline
    faded = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shapes, **kw))
    assert [(c.first_sample, c.data.shape[1]) for c in faded] == plain
    only = s.synthesize_delivered(ids, lens, scales, sid, normalize=False, shapes=shapes, **kw)
    assert _joined_rows(faded) == [a.tobytes() for a in only["streams"]]
    # normalised by the peaks the first stream reported: the normalised, limited delivery - and there the limiter works
    own = chunks[-1].peak
    assert np.array_equal(_bits(own), _bits(faded[-1].peak))
    norm = s.synthesize_delivered(ids, lens, scales, sid, normalize=True, shapes=shapes, limits=limits, **kw)
    loose = s.synthesize_delivered(ids, lens, scales, sid, normalize=True, shapes=shapes, **kw)
    assert norm["streams"][0].tobytes() != loose["streams"][0].tobytes(), "the limiter has nothing to do"
    chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shapes, limit=limits,
                                              ref_peak=own, **kw))
    _check_timeline(chunks, plain, counts, enc, LOOK)
    assert _joined_rows(chunks) == [a.tobytes() for a in norm["streams"]], (preset, chunk_frames, rate, "normalize 1")
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_token_gains_through_the_plan_callback(rate):
    """free durations: the breakpoints land on the token boundaries of THIS run, inside the engine's plan callback"""
    from phoonnx_amd.session import Limit, Shape
    s = _session("tiny_rb2_ms", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    rng = np.random.default_rng(3)
    db = rng.choice([-np.inf, -6.0, 0.0, 6.0], (3, 40))
    shape = Shape(30, 60, "linear")
    kw = dict(encoding="pcm16", volume=VOL3, seeds=seeds, token_gain_db=db, gain_ramp=0.004)
    want = s.synthesize_delivered(ids, lens, scales, sid, normalize=False, shapes=shape, limits=Limit(0.4, 64), **kw)
    assert any(len(sh.points) > 4 for sh in want["shapes"])
    for chunk_frames in (3, 64):
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shape, limit=Limit(0.4, 64), **kw))
        assert _joined_rows(chunks) == [a.tobytes() for a in want["streams"]], (rate, chunk_frames)
    # forced durations give the same points as the delivery's
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 3, 0).astype(np.int64)
    want = s.synthesize_delivered(ids, lens, scales, sid, normalize=False, shapes=shape, durations=dur, **kw)
    chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=5, shapes=shape, durations=dur, **kw))
    assert _joined_rows(chunks) == [a.tobytes() for a in want["streams"]]
    s.close()


def test_vocoder_stream_shaped():
    from phoonnx_amd.session import Limit, Segment, Shape
    s = _session("tiny_rb1")
    F = 23
    z = np.random.default_rng(5).standard_normal((2, s.hparam("inter"), F)).astype(np.float32)
    vol = np.array([0.5, 2.5], np.float32)
    shapes, limit = [Shape(40, 90, "smooth"), Shape(0, 0, "linear", [(10, 0.5), (500, 2.0)])], [Limit(0.2, 37), None]
    for rate in (None, 8000):
        s.set_output_rate(rate)
        x = s.vocoder(z)[:, 0, 0, :]
        n = x.shape[1]
        want = s.deliver([Segment(b, b, 0, 0, float(vol[b])) for b in range(2)], 2, "f32", shapes=shapes, limits=limit)
        for chunk_frames in (37, 4):
            plain = [(f, a.shape[1]) for f, a, _ in s.vocoder_stream(z, chunk_frames=chunk_frames)]
            chunks = list(s.vocoder_stream_encoded(z, chunk_frames=chunk_frames, encoding="f32", volume=vol, shapes=shapes, limit=limit))
            _check_timeline(chunks, plain, np.array([n, n], np.int64), "f32", 37)
            assert _joined_rows(chunks, 2) == [np.ascontiguousarray(a).tobytes() for a in want], (rate, chunk_frames)
    s.close()


def test_refusals_up_front_and_from_the_plan_callback():
    import ctypes as C
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import Limit, Segment, SessionError, Shape
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    segs = [Segment(b, b, 0, 1, float(VOL3[b])) for b in range(3)]
    before = [np.ascontiguousarray(a).tobytes() for a in s.deliver(segs, 3, "ulaw")]
    # refused by the call itself: nothing was started, the previous run stays deliverable
    for kw, word in ((dict(limit=Limit(2.0, LOOK)), "row 0: limit ceiling 2"), (dict(limit=Limit(0.5, 2000)), "lookahead 2000"),
                     (dict(shapes=Shape(-1, 0)), "row 0: fade_in -1"), (dict(limit=[Limit(0.5, 10), Limit(0.5, 11), None]), "one lookahead"),
                     (dict(limit=Limit(0.5, LOOK), volume=[1.0, 4000.0, 1.0]), "row 1: volume 4000")):
        with pytest.raises(SessionError, match=word):
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
    fmt = _ffi.VitsStreamFormat()

    def run(shp):
        return s._lib.vits_run_chunked_enc_shaped(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 3, 40, _ffi.ptr(sid), C.byref(noise), C.byref(ctl),
                                                  C.byref(fmt), C.byref(shp), 4, cb, None)

    bad = _ffi.VitsStreamShaping()
    bad.lookahead = 1025
    assert run(bad) == -3 and "lookahead 1025" in s._err() and calls == []
    assert [np.ascontiguousarray(a).tobytes() for a in s.deliver(segs, 3, "ulaw")] == before
    # the plan callback: what it sees, what it may refuse - no chunk callback then, and the previous run's results are gone
    seen = []
    ceil = np.array([0.5, 7.0, 0.5], np.float32)

    def planner(rc, write):
        @_ffi.STREAM_PLAN_FN
        def plan(user, B, T, dur, counts, inout):
            seen.append((B, T, np.ctypeslib.as_array(dur, shape=(B * T,)).copy(), np.ctypeslib.as_array(counts, shape=(B,)).copy()))
            if write:
                inout.contents.ceiling = ceil.ctypes.data
            return rc
        return plan

    for rc, write, word in ((1, False, "plan callback refused"), (0, True, "row 1: limit ceiling 7")):
        shp = _ffi.VitsStreamShaping()
        shp.lookahead = 16
        shp.plan = planner(rc, write)
        assert run(shp) == -3 and word in s._err(), s._err()
    assert calls == [] and len(seen) == 2
    B_, T_, dur, counts = seen[0]
    assert (B_, T_) == (3, 40) and np.array_equal(dur.reshape(3, 40), s.last_durations())
    assert np.array_equal(counts, np.asarray(r["y_lengths"], np.int64) * s.hparam("hop"))
    with pytest.raises(SessionError, match="no completed run"):
        s.deliver(segs, 3, "ulaw")
    s.close()


def test_closing_a_shaped_stream_ends_the_run():
    from phoonnx_amd.session import Limit, Shape
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds = _batch(s)
    x = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)["output"][:, 0, 0, :].copy()
    before = threading.active_count()
    gen = s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=1, encoding="ulaw", seeds=seeds, shapes=Shape(10, 10),
                                      limit=Limit(0.5, 16))
    first = next(gen)
    assert first.first_sample == 0 and first.data.shape == (3, s.hparam("hop") - 16)
    gen.close()
    assert threading.active_count() == before
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    assert np.array_equal(r["output"][:, 0, 0, :], x)
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_a_reservation_covers_the_shaped_stream(rate):
    """test_a_reservation_covers_the_stream's recipe with the longest look-ahead and two breakpoints per token"""
    from phoonnx_amd.session import Limit, Shape
    s = _session("tiny_rb1", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 120, 0).astype(np.int64)
    F = 40 * 120
    s.reserve(3, 40, F)
    cap = s.hparam("workspace_bytes")
    db = np.where(np.arange(40)[None, :] % 2 == 0, -6.0, 3.0) * np.ones((3, 1))
    for enc, chunk_frames in (("f32", F), ("pcm16", 1024), ("ulaw", 64)):
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  seeds=seeds, durations=dur, shapes=Shape(100, 100), token_gain_db=db,
                                                  limit=Limit(0.5, 1024)))
        assert s.hparam("workspace_bytes") == cap, (enc, "a shaped stream allocated behind a reservation that covers the request")
        assert sum(c.data.shape[1] for c in chunks) == chunks[0].total_samples
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
def test_voice_stream_encoded_equals_synthesize_encoded(encoding):
    from phoonnx_amd.config import SynthesisConfig
    voice = _voice("tiny_rb2_ms")
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=False)
    kw = dict(fade_in=0.005, fade_out=0.01, limit_ceiling=0.5)
    plain = voice.synthesize_encoded(TEXT, cfg, encoding=encoding)
    for silence, chunk_frames, more in ((0.0, 64, {}), (0.05, 7, {}), (0.0, 3, dict(phoneme_gain_db=lambda k, toks: [-6.0 * (i % 3) for i in range(len(toks))]))):
        want = voice.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=silence, **kw, **more)
        assert want.tobytes() != plain.tobytes()
        got = list(voice.stream_encoded(TEXT, cfg, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=silence, **kw, **more))
        assert b"".join(got) == want.tobytes(), (silence, chunk_frames)
    with pytest.raises(ValueError, match="limit_ceiling"):
        voice.stream_encoded(TEXT, cfg, encoding=encoding, limit_ceiling=1.5)
    with pytest.raises(ValueError, match="fade_curve"):
        voice.stream_encoded(TEXT, cfg, encoding=encoding, fade_curve="cubic")
    voice.session.close()
