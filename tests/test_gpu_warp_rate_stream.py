"""Streamed pitch at an output rate on the GPU (include/vitsmi.h, "pitch at an output rate"): the wide streamed stage by value
through vits_test_warp_rate_pieces / vits_test_glide_rate_pieces - pieces joined against the whole launch's bits, the windows
against the emit rule - and synthesize_stream / synthesize_stream_encoded with pitch at 8 kHz against the whole run and its
delivery, bit for bit."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_stream_trim import _threshold

pytestmark = pytest.mark.gpu

S, HOP, FI, FO = 1300, 4, 22050, 8000
# piece ends: a piece of one sample, pieces that complete nothing, the fast row's end (1000), steps of 64 otherwise
BOUNDS = [1, 30, 100, 101] + list(range(165, 1000, 64)) + [1000] + list(range(1064, S, 64)) + [S]

IDENTITY = ([200, 100], [0, 0], [0, 0], 1200)
FAST = ([250], [12], [12], 1000)               # step 5.51, Kh = 104: the plan's largest Kh, and the row that gates the others
SLOW = ([125, 0, 125], [-12, 3, 12], [-12, 3, 12], 1000)
GLIDING = ([100, 0, 150, 50], [-12, 0, 5, 0], [12, 0, -7, -12], 1200)
EMPTY = ([2, 3], [3, -2], [3, -2], 0)          # segments and no valid sample

BATCHES = {"warp": [IDENTITY, FAST, SLOW, EMPTY], "glide": [IDENTITY, FAST, GLIDING, EMPTY]}


@pytest.mark.parametrize("kind", list(BATCHES))
def test_pieces_joined_are_the_whole_launch(kind):
    from phoonnx_amd import session as ses
    import warp_rate_ref as ref
    rows = BATCHES[kind]
    B = len(rows)
    L, M = ref.ratio(FI, FO)
    counts = np.array([r[3] for r in rows], np.int64)
    rng = np.random.default_rng(67)
    x = rng.uniform(-1, 1, (B, S)).astype(np.float32)
    for b in range(B):
        x[b, counts[b]:] = 1000.0                                      # what lies behind a row's valid samples must not show
    if kind == "warp":
        plans = [([], None, 0) if not any(a) else ses.warp_plan_rate(D, a, HOP, L, M) for D, a, _, _ in rows]
        whole, pieces = ses.test_warp_rate, ses.test_warp_rate_pieces
    else:
        plans = [([], None, 0) if not (any(a) or any(e)) else ses.glide_plan_rate(D, a, e, HOP, L, M) for D, a, e, _ in rows]
        whole, pieces = ses.test_glide_rate, ses.test_glide_rate_pieces
    want, N = whole(x, counts, [p[0] for p in plans], FI, [FO] * B)
    S_w = int(max(1, N.max()))
    assert N[0] == -(-1200 * L // M) and want.shape == (B, S_w) and S_w > 256
    got, ranges = pieces(x, counts, [p[0] for p in plans], FI, FO, BOUNDS)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kind       # bit for bit, zeros behind N_b included
    # the schedule: contiguous, at most n_cap, and exactly what the rules say
    half, min_step = 104, min(M * ref.ONE // L, ref.token(-12, L, M)[0])
    K = 2 * int(np.ceil(16 / (0.85 * L / M)))
    n_cap = ses.warp_stream_cap_rate(int(np.diff([0] + BOUNDS).max()), S_w, min_step, half)
    sched, emitted = [], 0
    for i, X in enumerate(BOUNDS):
        ready = [ses.identity_emit_end_rate(L, M, K, counts[b], X) if not len(plans[b][0]) else
                 ses.warp_emit_end_rate(plans[b][0], counts[b], plans[b][2], X, half) for b in range(B) if X < counts[b]]
        e = S_w if i == len(BOUNDS) - 1 or not ready else min(ready)
        while emitted < e:
            n = min(n_cap, e - emitted)
            sched.append((emitted, n))
            emitted += n
    assert [tuple(r) for r in ranges.tolist()] == sched
    assert ranges[0, 0] == 0 and ranges[-1].sum() == S_w and ranges[:, 1].max() <= n_cap and ranges[:, 1].min() >= 1
    assert len(sched) > 8 and any(f % 256 and (f + n) % 256 for f, n in sched)


# ------------------------------------------------------------------ the whole path

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), pitch_at_rate=True, **kw)


def _inputs(s, seed=12):
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    st0, st1 = np.zeros((3, 40), np.float32), np.zeros((3, 40), np.float32)
    p0 = np.array([0, 3, -4, 7, -12, 12, 0.5, 2], np.float32)
    p1 = np.array([3, -4, -4, -12, 12, 0, 0.5, -1], np.float32)
    for b in (0, 2):                                                   # row 1 stays unpitched: an identity row of the stream
        st0[b, :lens[b]] = np.resize(np.roll(p0, b), lens[b])
        st1[b, :lens[b]] = np.resize(np.roll(p1, b), lens[b])
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64), st0, st1


_WHOLE = {}


def _whole(glide):
    """the whole pitched run of the fixture batch at 8 kHz, once per family"""
    if glide not in _WHOLE:
        s = _session("tiny_rb2_ms", output_rate=FO)
        ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
        kw = dict(seeds=seeds, token_semitones=st0)
        if glide:
            kw["token_semitones_end"] = st1
        r = s.synthesize_batch(ids, lens, scales, sid, return_durations=True, **kw)
        out = r["output"][:, 0, 0].copy()
        out.setflags(write=False)
        _WHOLE[glide] = dict(args=(ids, lens, scales, sid), kw=kw, out=out, counts=np.asarray(r["sample_lengths"], np.int64),
                             spans=r["token_spans"], F=int(r["y_lengths"].max()))
        s.close()
    return _WHOLE[glide]


def _cf(w, which):
    """chunk_frames: a small one, one that does not divide F, one past F"""
    if which == "F+5":
        return w["F"] + 5
    if which == "odd":
        return next(c for c in (7, 6, 5) if w["F"] % c)
    return which


@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("chunk", [2, "odd", "F+5"])
def test_fp32_pieces_are_the_whole_pitched_run_at_8_khz(chunk, glide):
    w = _whole(glide)
    assert w["F"] > 14
    s = _session("tiny_rb2_ms", output_rate=FO)
    total = int(w["counts"].max())
    y = np.full((3, total), np.nan, np.float32)
    at = 0
    for first, data, tot in s.synthesize_stream(*w["args"], chunk_frames=_cf(w, chunk), **w["kw"]):
        assert first == at and tot == total and data.shape[1] >= 1
        y[:, first:first + data.shape[1]] = data
        at += data.shape[1]
    assert at == total
    assert np.array_equal(y.view(np.uint32), w["out"].view(np.uint32)), (chunk, glide)
    assert np.array_equal(s.last_sample_counts(), w["counts"]) and np.array_equal(s.last_token_spans(), w["spans"])
    s.close()


VOL3 = np.array([1.0, 0.5, 2.5], np.float32)
LOOK = 40


@pytest.mark.parametrize("chunk", [2, "odd", "F+5"])
def test_encoded_pieces_are_the_delivery_of_the_pitched_run_at_8_khz(chunk):
    from phoonnx_amd.session import Limit, Onset, Shape, Trim
    w = _whole(True)
    cf = _cf(w, chunk)
    s = _session("tiny_rb2_ms", output_rate=FO)
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
        rows = [b"".join(c.data[b, int(c.skip[b]):int(c.valid[b])].tobytes() for c in chunks) for b in range(3)]
        assert rows == [np.ascontiguousarray(r).tobytes() for r in want["streams"]], what

    for enc in ("pcm16", "ulaw"):
        kw = dict(encoding=enc, volume=VOL3, **w["kw"])
        want = s.synthesize_delivered(*args, normalize=False, **kw)
        assert np.array_equal(np.asarray(want["sample_lengths"], np.int64), counts)
        check(list(s.synthesize_stream_encoded(*args, chunk_frames=cf, **kw)), want, (chunk, enc, "plain"))
    # fades, a per-token volume and a limiter with look-ahead: the breakpoints lie on the folded plan's token spans
    db = np.random.default_rng(3).choice([-np.inf, -6.0, 0.0, 6.0], (3, 40))
    shape, limit = Shape(40, 80, "smooth"), Limit(0.4, LOOK)
    kw = dict(encoding="ulaw", volume=VOL3, token_gain_db=db, gain_ramp=0.004, **w["kw"])
    want = s.synthesize_delivered(*args, normalize=False, shapes=shape, limits=limit, **kw)
    assert any(len(sh.points) > 4 for sh in want["shapes"])
    check(list(s.synthesize_stream_encoded(*args, chunk_frames=cf, shapes=shape, limit=limit, **kw)), want, (chunk, "shaped"))
    # a leading onset trim
    thr = _threshold(w["out"], counts)
    kw = dict(encoding="pcm16", volume=VOL3, **w["kw"])
    trims = [Trim(1, thr, LOOK, int(counts[b]), 0) for b in range(3)]
    want = s.synthesize_delivered(*args, normalize=False, shapes=shape, limits=limit, trim=trims, **kw)
    chunks = list(s.synthesize_stream_encoded(*args, chunk_frames=cf, shapes=shape, limit=limit, onsets=Onset(1, thr, LOOK), **kw))
    assert any(c.skip.any() for c in chunks), "nothing was trimmed"
    check(chunks, want, (chunk, "trimmed"))
    s.close()


def test_a_stream_with_per_row_rates_stays_refused():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    s.set_output_rates([8000, 0, 16000])
    for call in (s.synthesize_stream, s.synthesize_stream_encoded):
        with pytest.raises(ses.SessionError, match="not covered with an output rate set per row"):
            call(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    s.close()
