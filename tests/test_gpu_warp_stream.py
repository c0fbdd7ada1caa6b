"""Streamed pitch on the GPU (include/vitsmi.h, "streamed pitch"): the stage by value through vits_test_warp_pieces /
vits_test_glide_pieces - the input cut at arbitrary piece ends, the windows joined against the whole launch's bits and the
schedule against the emit rule -, then vits_run_chunked_glided / vits_run_chunked_enc_glided end to end through MiSession
against the whole runs of the same options, and TTSVoice.stream_encoded(pitch_contour=, phoneme_pitch=).

References: the whole-waveform launches (vits_test_warp / vits_test_glide, vits_run_async_glided, synthesize_delivered), bit
for bit; tests/warp_ref.py / tests/glide_ref.py in float64 with their own tolerance, unchanged."""
import ctypes as C

import numpy as np
import pytest

import glide_ref
import warp_ref
from test_gpu_glide import _inputs, _session, _voice
from test_gpu_stream_trim import _threshold

pytestmark = pytest.mark.gpu

S, HOP = 1300, 4
# piece ends: a piece of 1 sample, pieces that complete nothing (X <= 38), an end on row C's token boundary (400) and on
# the fast row's end (1000), the rest in steps of 64; the longest piece (70) sizes n_cap = 2 * (70 + 38) = 216
BOUNDS = [1, 30, 100, 101] + list(range(165, 400, 64)) + [400] + list(range(464, 1000, 64)) + [1000] + list(range(1064, S, 64)) + [S]
N_CAP = 216

IDENTITY = ([200, 100], [0, 0], [0, 0], 1200)
FAST = ([250], [12], [12], 1000)               # the row that consumes its input fastest gates the others until it ends
BOTH = ([125, 0, 125], [-12, 3, 12], [-12, 3, 12], 1000)
GLIDING = ([100, 0, 150, 50], [-12, 0, 5, 0], [12, 0, -7, -12], 1200)
EMPTY = ([2, 3], [3, -2], [3, -2], 0)          # segments and no valid sample
EMPTY_GLIDE = ([2, 3], [3, -2], [1, 4], 0)

# (kind, rows, whether the gating row - FAST - ends while the others have more than n_cap ready)
BATCHES = {
    "glide": ("glide", [IDENTITY, FAST, GLIDING], True),
    "glide, a row without input": ("glide", [EMPTY_GLIDE, BOTH, GLIDING], False),
    "warp": ("warp", [IDENTITY, FAST, BOTH], True),
    "warp, a row without input": ("warp", [BOTH, EMPTY, FAST], True),
}


def _family(kind):
    from phoonnx_amd import session as ses
    if kind == "warp":
        return (lambda D, a, b: ses.warp_plan(D, a, HOP)), ses.test_warp, ses.test_warp_pieces, ses.warp_emit_end
    return (lambda D, a, b: ses.glide_plan(D, a, b, HOP)), ses.test_glide, ses.test_glide_pieces, ses.glide_emit_end


def _schedule(emit, plans, n_in, S_w):
    """the windows the rule gives for BOUNDS: e(X) per piece, cut at N_CAP"""
    out, emitted = [], 0
    for i, X in enumerate(BOUNDS):
        live = [b for b in range(len(plans)) if X < n_in[b]]
        e = S_w if i == len(BOUNDS) - 1 or not live else min(emit(plans[b][0], n_in[b], plans[b][2], X) for b in live)
        pieces = 0
        while emitted < e:
            n = min(N_CAP, e - emitted)
            out.append((emitted, n, i))
            emitted += n
            pieces += 1
    return out


@pytest.mark.parametrize("name", list(BATCHES))
def test_pieces_joined_are_the_whole_launch(name):
    from phoonnx_amd.session import warp_stream_cap
    kind, rows, releases = BATCHES[name]
    plan, whole, pieces, emit = _family(kind)
    B = len(rows)
    assert B == 3
    counts = np.array([r[3] for r in rows], np.int64)
    rng = np.random.default_rng(61)
    x = rng.uniform(-1, 1, (B, S)).astype(np.float32)
    for b in range(B):
        x[b, counts[b]:] = 1000.0                                      # what lies behind a row's valid samples must not show
    plans = [plan(D, a, b) for D, a, b, _ in rows]
    S_w = max(1, max(p[2] for p in plans))
    assert S_w > 512 and warp_stream_cap(max(np.diff([0] + BOUNDS)), S_w) == N_CAP
    want = whole(x, counts, [p[0] for p in plans])
    got, ranges = pieces(x, counts, [p[0] for p in plans], BOUNDS)
    assert got.shape == want.shape == (B, S_w)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name        # bit for bit, zeros behind N_b included
    # the schedule: contiguous, at most n_cap, and exactly what the rule says
    sched = _schedule(emit, plans, counts, S_w)
    assert [tuple(r) for r in ranges.tolist()] == [(f, n) for f, n, _ in sched]
    assert ranges[0, 0] == 0 and np.array_equal(ranges[1:, 0], (ranges[:, 0] + ranges[:, 1])[:-1]) and ranges[-1].sum() == S_w
    assert ranges[:, 1].max() <= N_CAP and ranges[:, 1].min() >= 1
    by_piece = [sum(1 for _, _, i in sched if i == p) for p in range(len(BOUNDS))]
    assert by_piece[0] == 0 and by_piece[1] == 0, "pieces in front of the first 38 samples complete nothing"
    assert max(by_piece) >= 2 or not releases, "no piece releases more than n_cap"
    assert any(f % 256 and (f + n) % 256 and f // 256 == (f + n - 1) // 256 for f, n, _ in sched), "no window inside one tile"
    assert any((f + n - 1) // 256 > f // 256 for f, n, _ in sched), "no window over more than one block"
    # ... and the float64 definition, within its own tolerance
    for b, (D, a, e, n_b) in enumerate(rows):
        if kind == "warp":
            segs, _, N = warp_ref.plan(D, a, HOP)
            ref64, tol = warp_ref.warp64(x[b, :n_b], segs, N), warp_ref.tolerance(segs, 1.0)
        else:
            segs, _, N = glide_ref.plan(D, a, e, HOP)
            ref64, tol = glide_ref.glide64(x[b, :n_b], segs, N), glide_ref.tolerance(segs, 1.0)
        err = float(np.abs(got[b, :N] - ref64).max()) if N else 0.0
        print(f"{name} row {b}: n_b = {n_b}, N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert N == plans[b][2] and err <= tol and not got[b, N:].any(), (name, b, err, tol)


def test_the_hook_refuses_bad_pieces():
    from phoonnx_amd import session as ses
    plan, _, pieces, _ = _family("warp")
    x = np.zeros((1, 64), np.float32)
    segs = plan([16], [3], None)[0]
    for bounds, what in (([10, 10, 64], "does not ascend"), ([10, 60], "not at S"), ([10, 70], "does not ascend")):
        with pytest.raises(ses.SessionError, match=what):
            pieces(x, [64], [segs], bounds)


# ------------------------------------------------------------------ through the ABI

_WHOLE = {}


def _whole(preset, compensate, glide):
    """the whole run of the fixture batch, once per combination: options, output, counts, spans, F"""
    key = (preset, compensate, glide)
    if key not in _WHOLE:
        s = _session(preset)
        ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
        kw = dict(seeds=seeds, token_semitones=st0, compensate=bool(compensate))
        if glide:
            kw["token_semitones_end"] = st1
        r = s.synthesize_batch(ids, lens, scales, sid, return_durations=True, **kw)
        out = r["output"][:, 0, 0].copy()
        out.setflags(write=False)
        _WHOLE[key] = dict(args=(ids, lens, scales, sid), kw=kw, out=out, counts=np.asarray(r["sample_lengths"], np.int64),
                           spans=r["token_spans"], F=int(r["y_lengths"].max()), hop=s.hparam("hop"))
        s.close()
    return _WHOLE[key]


def _chunk_frames(w, which):
    return w["F"] + 5 if which == "F+5" else which


def _join(chunks, B, total):
    y = np.full((B, total), np.nan, np.float32)
    at = 0
    for first, data, tot in chunks:
        assert first == at and tot == total and data.shape[1] >= 1
        y[:, first:first + data.shape[1]] = data
        at += data.shape[1]
    assert at == total
    return y


@pytest.mark.parametrize("compensate", [0, 1])
@pytest.mark.parametrize("chunk", [1, 3, 7, "F+5"])
def test_fp32_pieces_are_the_whole_glided_run(chunk, compensate):
    from phoonnx_amd.session import warp_stream_cap
    w = _whole("tiny_rb2_ms", compensate, True)
    s = _session("tiny_rb2_ms")
    cf = _chunk_frames(w, chunk)
    seen = {}

    def watched():
        for item in s.synthesize_stream(*w["args"], chunk_frames=cf, **w["kw"]):
            if not seen:      # from the first chunk on
                seen.update(counts=s.last_sample_counts(), spans=s.last_token_spans())
            yield item

    chunks = list(watched())
    total = int(w["counts"].max())
    y = _join(chunks, 3, total)
    assert np.array_equal(y.view(np.uint32), w["out"].view(np.uint32)), (chunk, compensate)
    assert np.array_equal(seen["counts"], w["counts"]) and np.array_equal(seen["spans"], w["spans"])
    assert np.array_equal(s.last_sample_counts(), w["counts"]) and np.array_equal(s.last_token_spans(), w["spans"])
    assert max(d.shape[1] for _, d, _ in chunks) <= warp_stream_cap(min(cf, w["F"]) * w["hop"], total)
    s.close()


@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms"])
def test_equal_ends_stream_the_warp(preset):
    w = _whole(preset, 1, False)
    s = _session(preset)
    y = _join(list(s.synthesize_stream(*w["args"], chunk_frames=3, **w["kw"])), 3, int(w["counts"].max()))
    assert np.array_equal(y.view(np.uint32), w["out"].view(np.uint32))
    launches = s.stats()["total_launches"]
    # equal ends given as a glide: the warp's kernel, the same launches, the same bits
    y2 = _join(list(s.synthesize_stream(*w["args"], chunk_frames=3, token_semitones_end=w["kw"]["token_semitones"], **w["kw"])), 3,
               int(w["counts"].max()))
    assert s.stats()["total_launches"] == launches and np.array_equal(y2.view(np.uint32), y.view(np.uint32))
    s.close()


def _kept_rows(chunks, B=3):
    return [b"".join(c.data[b, int(c.skip[b]):int(c.valid[b])].tobytes() for c in chunks) for b in range(B)]


VOL3 = np.array([1.0, 0.5, 2.5], np.float32)
LOOK = 110


@pytest.mark.parametrize("compensate", [0, 1])
@pytest.mark.parametrize("chunk", [1, 3, 7, "F+5"])
def test_encoded_pieces_are_the_delivery_of_the_glided_run(chunk, compensate):
    from phoonnx_amd.session import Limit, Onset, Shape, Trim
    w = _whole("tiny_rb2_ms", compensate, True)
    cf = _chunk_frames(w, chunk)
    s = _session("tiny_rb2_ms")
    args, counts = w["args"], w["counts"]
    total = int(counts.max())

    def check(chunks, want, what):
        at = 0
        for c in chunks:
            n = c.data.shape[1]
            assert c.first_sample == at and c.total_samples == total and n >= 1, what
            assert np.array_equal(c.valid, np.clip(counts - c.first_sample, 0, n)), what
            at += n
        assert at == total, what
        assert _kept_rows(chunks) == [np.ascontiguousarray(r).tobytes() for r in want["streams"]], what

    # plain, in both encodings
    for enc in ("pcm16", "ulaw"):
        kw = dict(encoding=enc, volume=VOL3, **w["kw"])
        want = s.synthesize_delivered(*args, normalize=False, **kw)
        assert np.array_equal(np.asarray(want["sample_lengths"], np.int64), counts)
        chunks = list(s.synthesize_stream_encoded(*args, chunk_frames=cf, **kw))
        assert not any(c.skip.any() for c in chunks)
        check(chunks, want, (chunk, compensate, enc, "plain"))
    # fades, a per-token volume and a limiter with look-ahead: the breakpoints lie on the warp's token spans
    enc = "ulaw" if compensate else "pcm16"
    db = np.random.default_rng(3).choice([-np.inf, -6.0, 0.0, 6.0], (3, 40))
    shape, limit = Shape(100, 200, "smooth"), Limit(0.4, LOOK)
    kw = dict(encoding=enc, volume=VOL3, token_gain_db=db, gain_ramp=0.004, **w["kw"])
    want = s.synthesize_delivered(*args, normalize=False, shapes=shape, limits=limit, **kw)
    assert any(len(sh.points) > 4 for sh in want["shapes"])
    check(list(s.synthesize_stream_encoded(*args, chunk_frames=cf, shapes=shape, limit=limit, **kw)), want, (chunk, compensate, "shaped"))
    # a leading onset trim whose keep_lead <= the look-ahead
    x = w["out"]
    thr = _threshold(x, counts)      # (above the first eighth of the longest row: its onset lies behind sample 0)
    kw = dict(encoding=enc, volume=VOL3, **w["kw"])
    for keep_lead in (0, LOOK):
        trims = [Trim(1, thr, keep_lead, int(counts[b]), 0) for b in range(3)]
        want = s.synthesize_delivered(*args, normalize=False, shapes=shape, limits=limit, trim=trims, **kw)
        chunks = list(s.synthesize_stream_encoded(*args, chunk_frames=cf, shapes=shape, limit=limit, onsets=Onset(1, thr, keep_lead), **kw))
        assert any(c.skip.any() for c in chunks), "nothing was trimmed"
        check(chunks, want, (chunk, compensate, "trimmed", keep_lead))
    s.close()


def test_all_zero_semitones_are_the_unwarped_stream():
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, _, _ = _inputs(s)
    ones = np.ones((3, 40), np.float32)
    zero = np.zeros((3, 40), np.float32)
    zero[1, 30] = 5.0                                                  # behind lens[1]: ignored
    base = list(s.synthesize_stream(ids, lens, scales, sid, chunk_frames=7, seeds=seeds, token_rate=ones))   # vits_run_chunked_ctl
    launches = s.stats()["total_launches"]
    for kw in ({"token_semitones": zero}, {"token_semitones": zero, "token_semitones_end": zero.copy()}, {"token_semitones_end": zero}):
        got = list(s.synthesize_stream(ids, lens, scales, sid, chunk_frames=7, seeds=seeds, token_rate=ones, **kw))
        assert s.stats()["total_launches"] == launches
        assert [(f, d.shape, t) for f, d, t in got] == [(f, d.shape, t) for f, d, t in base]
        assert all(np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) for a, b in zip(got, base))
        with pytest.raises(Exception, match="not warped"):
            s.last_token_spans()
    enc = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=7, seeds=seeds, encoding="ulaw"))
    launches = s.stats()["total_launches"]
    got = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=7, seeds=seeds, encoding="ulaw", token_semitones=zero))
    assert s.stats()["total_launches"] == launches
    assert [(c.first_sample, c.data.tobytes(), c.valid.tolist()) for c in got] == [(c.first_sample, c.data.tobytes(), c.valid.tolist()) for c in enc]
    assert not any(c.skip.any() for c in got)
    s.close()


def test_refusals_leave_the_previous_run_readable():
    from phoonnx_amd import _ffi
    from phoonnx_amd import session as ses
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    kw = dict(seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    r = s.synthesize_batch(ids, lens, scales, sid, return_durations=True, **kw)

    def readable():
        again = np.empty_like(r["output"])
        s._fetch(again, 0, 3)
        assert np.array_equal(again, r["output"]) and np.array_equal(s.last_sample_counts(), r["sample_lengths"])
        assert np.array_equal(s.last_token_spans(), r["token_spans"])

    # by the call, not by the first next()
    bad = st1.copy()
    bad[2, 3] = -13.0
    for call in (s.synthesize_stream, s.synthesize_stream_encoded):
        s.set_output_rate(8000)
        with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
            call(ids, lens, scales, sid, **kw)
        s.set_output_rate(None)
        s.set_output_rates([8000, 0, 16000])
        with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
            call(ids, lens, scales, sid, **kw)
        s.set_output_rates(None)
        with pytest.raises(ses.SessionError, match=r"token_semitones_end\[2,3\]"):
            call(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=bad)
        with pytest.raises(ses.SessionError, match="forced durations are the rendered ones"):
            call(ids, lens, scales, sid, durations=r["durations"], **kw)
        readable()
    # ... and the engine's own refusals, straight at the entry
    lib = s._lib
    rows = np.ascontiguousarray(scales, np.float32)
    seeds64 = np.ascontiguousarray(seeds, np.uint64)
    ctl = _ffi.VitsControls(rows.ctypes.data, seeds64.ctypes.data, None, None)
    noise = _ffi.VitsNoise()

    @_ffi.CHUNK_FN
    def never(user, samples, B, first, n, total):
        raise AssertionError("not reached")

    def run(st_a, st_b, compensate=0):
        con = _ffi.VitsContour(st_a.ctypes.data, st_b.ctypes.data, compensate)
        return lib.vits_run_chunked_glided(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 3, 40, _ffi.ptr(sid), C.byref(noise), C.byref(ctl),
                                           C.byref(con), 4, never, None)

    s.set_output_rate(8000)
    assert run(st0, st1) != 0 and "vits_run_chunked_glided is not covered with an output rate set" in s._err()
    s.set_output_rate(None)
    assert run(st0, bad) != 0 and "token_semitones_end[2,3]" in s._err()
    dur = np.ascontiguousarray(r["durations"], np.int64)
    ctl.durations = dur.ctypes.data
    assert run(st0, st1, 1) != 0 and "forced durations are the rendered ones" in s._err()
    readable()
    s.close()


def test_stream_encoded_with_a_contour_is_synthesize_encoded():
    from phoonnx_amd.config import SynthesisConfig
    text = "hello there. go"
    cfg = SynthesisConfig(normalize_audio=False)
    kw = dict(pitch_contour=[(0, 0), (1, 4)], phoneme_pitch=-2, sentence_silence=0.01)
    s = _session("tiny_rb2_ms")
    want = np.ascontiguousarray(_voice(s).synthesize_encoded(text, cfg, **kw).data).tobytes()
    s.close()
    for chunk_frames in (3, 64):
        s = _session("tiny_rb2_ms")            # (a fresh session: the same point of its noise stream)
        got = b"".join(_voice(s).stream_encoded(text, cfg, chunk_frames=chunk_frames, **kw))
        assert got == want, chunk_frames
        s.close()
