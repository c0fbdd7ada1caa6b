"""Limited delivery on the GPU (include/vitsmi.h, "limited delivery"): the gain launch and the limited pack by value through
vits_test_deliver_limited, then the feature through MiSession and TTSVoice.

Reference: tests/limit_ref.py (NumPy: int64 up to the division, float32 behind it) applied to the same float waveform.  Bytes
are exact (a levelled segment's: given the gain the device reports, as in test_gpu_loudness.py)."""
import os

import numpy as np
import pytest

import limit_ref as ref
import loudness_ref as lref
import shape_ref as sref
import trim_ref as tref
from conftest import GOLDEN
from delivery_ref import WIDTH, Seg
from limit_ref import B, CEILING, COUNTS, RATE, Limit
from shape_ref import Shape
from trim_ref import Trim

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
LOOKAHEADS = (1, 7, 255, 1024)
CURVE = {0: "linear", 1: "smooth"}
F = np.float32
X = ref.batch()                      # computed once, never written to


def _segments(segs):
    from phoonnx_amd.session import Segment
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _trims(trims):
    from phoonnx_amd import session as ses
    return None if trims is None else [ses.Trim(*t) for t in trims]


def _levels(levels):
    from phoonnx_amd import session as ses
    return None if levels is None else [ses.Level(*l) for l in levels]


def _shapes(shapes):
    from phoonnx_amd import session as ses
    return None if shapes is None else [ses.Shape(s.fade_in, s.fade_out, CURVE[s.curve], tuple(s.points)) for s in shapes]


def _limits(limits):
    from phoonnx_amd import session as ses
    return None if limits is None else [None if l is None else ses.Limit(float(l.ceiling), int(l.lookahead)) for l in limits]


def _bytes(streams):
    return [np.ascontiguousarray(a).tobytes() for a in streams]


def _same(have, want, what):
    assert [len(g) for g in have] == [len(w) for w in want], what
    for j, (h, w) in enumerate(zip(have, want)):
        if h != w:
            a, b = np.frombuffer(h, np.uint8), np.frombuffer(w, np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what} stream {j}: {bad.size} of {a.size} bytes differ, first at {bad[:8]}")


def _deliver(x, counts, segs, limits, shapes=None, trims=None, levels=None, J=None, encoding="pcm16"):
    from phoonnx_amd.session import test_deliver_limited
    return test_deliver_limited(x, counts, _segments(segs), _limits(limits), _shapes(shapes), _trims(trims), _levels(levels), RATE,
                                J, encoding)


def _check(x, counts, segs, limits, shapes, trims, levels, J, encoding, what):
    """one call against the reference: bytes and kept ranges -> (the call's result, the reference's limited values)"""
    got = _deliver(x, counts, segs, limits, shapes, trims, levels, J, encoding)
    want, kept, vals = ref.deliver_ref(x, counts, segs, trims, levels, shapes, limits, J, encoding, level_gains=got["gain"])
    assert got["kept_first"].tolist() == [a for a, _ in kept] and got["kept_count"].tolist() == [c for _, c in kept], what
    _same(_bytes(got["streams"]), want, what)
    return got, vals


# the common plan: rows 1 and 0 back to back in stream 0 (4097 + 9000 samples: both boundaries lie inside a pack tile and a
# 16-byte cell in every encoding, and inside a tile of the gain kernel - the first one a single sample into it), the rows of one
# and of no sample and the 5000 behind a lead in stream 1
PLAN = [Seg(1, 0, 0, 0, 1.0), Seg(0, 0, 0, 0, 1.0), Seg(2, 1, 0, 0, 1.0), Seg(3, 1, 0, 0, 1.0), Seg(4, 1, 3, 0, 1.0)]


def test_the_batch_covers_what_it_claims():
    """What the reference says of the by-value batch (no GPU work: it guards the cases themselves)."""
    u, kept = ref.unlimited(X, COUNTS, PLAN, None, None, None, 2)
    assert [c for _, c in kept] == [4097, 9000, 1, 0, 5000] and COUNTS.tolist() == [9000, 4097, 1, 0, 5000]
    for g, v in enumerate(u):
        if len(v) >= 300:
            assert 0.05 <= ref.over_fraction(v, CEILING) <= 0.5, (g, ref.over_fraction(v, CEILING))
    assert sum(len(v) >= 300 for v in u) == 3 and max(np.abs(v).max() for v in u if len(v)) > 2.0
    for w in (1, 2, 4):              # bytes per element: a segment boundary inside a tile of 256 cells and inside a 16-byte cell
        for edge in (4097, 4097 + 9000, 4097 + 9000 + 1):
            assert edge % (4096 // w) and edge % (16 // w)
    assert 4097 % 2048 == 1 and (4097 + 9000) % 2048     # ... and inside a tile of the gain kernel
    for L in LOOKAHEADS:             # the limiter works, differently for every L, and holds the ceiling
        g = ref.gains(u[1], Limit(CEILING, L))
        assert (g < 1).mean() > 0.3 and np.abs(ref.apply(u[1], Limit(CEILING, L))).max() <= F(CEILING)


@pytest.mark.parametrize("L", LOOKAHEADS)
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_limited_delivery_by_value(encoding, L):
    from phoonnx_amd.session import test_deliver_shaped
    limits = [Limit(CEILING, L)] * B
    got, vals = _check(X, COUNTS, PLAN, limits, None, None, None, 2, encoding, f"{encoding} L={L}")
    # the layout never depends on the limits; the bytes do
    base = test_deliver_shaped(X, COUNTS, _segments(PLAN), None, None, None, RATE, 2, encoding)
    for key in ("stream_samples", "stream_offsets", "kept_first", "kept_count"):
        assert np.array_equal(base[key], got[key]), key
    assert _bytes(base["streams"]) != _bytes(got["streams"])
    if encoding == "pcm16":          # decoded, no sample of a limited segment exceeds trunc(ceiling * 32767)
        top = int(F(CEILING) * F(32767.0))
        assert all(np.abs(s.astype(np.int32)).max() <= top for s in got["streams"])
        assert max(np.abs(s.astype(np.int32)).max() for s in got["streams"]) >= top - 1 and np.abs(base["streams"][0]).max() == 32767
    # two calls give identical bytes
    again = _deliver(X, COUNTS, PLAN, limits, J=2, encoding=encoding)
    assert _bytes(again["streams"]) == _bytes(got["streams"])


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_edges_of_a_segment(encoding):
    """The loud sample first and last in its segment, a segment shorter than L, and two segments back to back of which the
    first ends loud: the second one's first sample has g == 1."""
    quiet = F(0.25)
    x = np.full((5, 700), quiet, F)
    x[:, 1::2] = -quiet
    counts = np.array([700, 600, 50, 333, 421], np.int64)
    x[0, 0] = 0.95                                     # loud first
    x[1, 599] = -0.95                                  # loud last
    x[2, :50] = (np.random.default_rng(8).standard_normal(50) * 0.9).astype(F)    # c = 50 < L = 255
    x[3, 332] = 1.9                                    # ends loud ...
    segs = [Seg(0, 0, 2, 0, 1.0), Seg(1, 1, 0, 0, 1.0), Seg(2, 2, 0, 0, 1.0), Seg(3, 3, 0, 0, 1.0), Seg(4, 3, 0, 0, 1.0)]    # ... 4 right behind 3
    limits = [Limit(0.7, 110), Limit(0.7, 110), Limit(0.5, 255), Limit(0.7, 64), Limit(0.7, 64)]
    got, vals = _check(x, counts, segs, limits, None, None, None, 4, encoding, encoding)
    u, _ = ref.unlimited(x, counts, segs, None, None, None, 4)
    g = [ref.gains(v, l) for v, l in zip(u, limits)]
    assert g[0][0] == g[0].min() < 1 and (g[0][111:] == 1).all() and g[1][-1] == g[1].min() < 1 and (g[1][:-111] == 1).all()
    assert (g[2] < 1).all() and g[3][-1] < 0.4 and (g[3][:-65] == 1).all()
    assert (g[4] == 1).all()                            # a segment never sees its neighbour
    if encoding == "f32":
        s3 = got["streams"][3]
        assert s3[333] == x[4, 0] and abs(s3[332]) <= F(0.7) and np.array_equal(s3[333:], x[4, :421])
        assert got["streams"][0][2] == vals[0][0] and abs(vals[0][0]) <= F(0.7)


def _mixed():
    """Limited and unlimited segments mixed over four streams with leads and tails: a relative trim, a stream-scope level,
    normalize 2 in another stream, fades and an envelope.  Rows 0 and 4 get a quiet front and back for the trims to cut."""
    x = X.copy()
    x[:2] *= F(0.25)                 # (quiet enough for the level to RAISE them: the gain pushes the peaks past full scale)
    x[0, :300] *= F(0.001)
    x[0, 8500:] *= F(0.001)
    x[4, :150] = 0
    x[4, 4800:5000] = 0
    segs = [Seg(0, 0, 4, 0, 0.9), Seg(1, 0, 0, 0, 0.9),            # stream 0: levelled together (mode 2), row 0 trimmed (relative)
            Seg(4, 1, 7, 2, 1.5), Seg(2, 1, 0, 2, 1.5),            # stream 1: normalize 2, volume 1.5: above the ceiling
            Seg(3, 2, 2, 0, 1.0)]                                  # stream 2: the row without samples, limited
    trims = [Trim(2, 0.05, 16, 32, 5), Trim(0, 0.0, 0, 0, 3), Trim(1, 0.01, 0, 0, 0), tref.OFF, Trim(0, 0.0, 0, 0, 9)]
    lv = lref.Level(2, -3.0, 40.0, 0.0)
    levels = [lv, lv, lref.OFF, lref.OFF, lref.OFF]
    shapes = [Shape(200, 400, 1, ((1000, 1.0), (1500, 1.6), (4000, 0.5))), sref.NONE, Shape(64, 64, 0, ((100, 0.5), (2000, 1.25))), Shape(1, 1, 0, ()),
              sref.NONE]
    limits = [Limit(0.6, 110), None, Limit(0.8, 255), Limit(0.8, 7), Limit(0.5, 1024)]
    return x, segs, trims, levels, shapes, limits


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_limits_with_trims_levels_normalisation_and_shapes(encoding):
    from phoonnx_amd.session import test_deliver_shaped
    x, segs, trims, levels, shapes, limits = _mixed()
    got, vals = _check(x, COUNTS, segs, limits, shapes, trims, levels, 3, encoding, encoding)
    u, kept = ref.unlimited(x, COUNTS, segs, trims, levels, shapes, 3, got["gain"])
    assert kept[0][0] > 0 and kept[0][1] < 9000 and kept[2][0] > 0 and kept[2][1] < 5000                 # the trims cut
    assert 0.05 <= ref.over_fraction(u[0], 0.6) <= 0.5 and 0.05 <= ref.over_fraction(u[2], 0.8) <= 0.5      # the limiter works
    assert np.abs(u[1]).max() > 1 and vals[0][0] == 0 and vals[0][-1] == 0                                  # a faded segment still starts and ends at 0
    # peaks, kept ranges, loudness and gain are those of the unlimited audio; the layout does not depend on the limits
    base = test_deliver_shaped(x, COUNTS, _segments(segs), _shapes(shapes), _trims(trims), _levels(levels), RATE, 3, encoding)
    for key in ("stream_samples", "stream_offsets", "kept_first", "kept_count"):
        assert np.array_equal(base[key], got[key]), key
    assert np.array_equal(base["gain"].view(np.uint32), got["gain"].view(np.uint32)) and base["loudness"][0] == got["loudness"][0]
    assert got["gain"][0] == got["gain"][1] > 1
    # the unlimited segment between limited ones: its bytes are the shaped delivery's
    w = WIDTH[encoding]
    lo = (4 + kept[0][1] + 5) * w
    s0, b0 = _bytes(got["streams"])[0], _bytes(base["streams"])[0]
    assert s0[lo:] == b0[lo:] and s0[:lo] != b0[:lo]
    if encoding == "pcm16":
        a = np.frombuffer(s0[:lo], "<i2")
        assert np.abs(a.astype(np.int32)).max() <= int(F(0.6) * F(32767.0))
        assert np.abs(got["streams"][1].astype(np.int32)).max() <= int(F(0.8) * F(32767.0))
    # everything of x outside the kept ranges set to NaN: the halo does not read there, and the bytes stay
    a2, c2 = kept[2]
    poisoned = np.full_like(x, np.nan)
    for s, (a, c) in zip(segs, kept):
        poisoned[s.row, a:a + c] = x[s.row, a:a + c]
    poisoned[0, :COUNTS[0]] = np.where(np.isnan(poisoned[0, :COUNTS[0]]), x[0, :COUNTS[0]], poisoned[0, :COUNTS[0]])  # (the relative trim's
    # peak and scan read the whole row: row 0 stays whole up to its count)
    assert np.isnan(poisoned[4, :a2]).all() and np.isnan(poisoned[4, a2 + c2:]).all() and np.isnan(poisoned[1, 4097:]).all()
    again = _deliver(poisoned, COUNTS, segs, limits, shapes, trims, levels, 3, encoding)
    assert _bytes(again["streams"]) == _bytes(got["streams"])
    assert np.array_equal(again["kept_first"], got["kept_first"]) and np.array_equal(again["kept_count"], got["kept_count"])


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_a_ceiling_nothing_reaches_and_no_limits(encoding):
    from phoonnx_amd import session as ses
    x, segs, trims, levels, shapes, _ = _mixed()
    segs = [s._replace(volume=0.2, normalize=0) for s in segs]           # |u| <= 0.2 * 1.6 * 2.8 < 1 without levels
    base = ses.test_deliver_shaped(x, COUNTS, _segments(segs), _shapes(shapes), _trims(trims), None, RATE, 3, encoding)
    u, _ = ref.unlimited(x, COUNTS, segs, trims, None, shapes, 3)
    top = max(np.abs(v).max() for v in u if len(v))
    assert 0.5 < top < 1.0
    for limits in ([Limit(1.0, 110)] * 5, [Limit(float(top), 1024)] * 5, None, [None] * 5):
        got = _deliver(x, COUNTS, segs, limits, shapes, trims, None, 3, encoding)
        assert _bytes(got["streams"]) == _bytes(base["streams"])
        for key in ("stream_samples", "stream_offsets", "kept_first", "kept_count"):
            assert np.array_equal(base[key], got[key]), key


def _canary():
    return np.full(4096, 0xA5, np.uint8)


@pytest.mark.parametrize("name", sorted(ref.LIMIT_REFUSALS) + ["a shape", "a trim"])
def test_refusals_write_nothing(name):
    from phoonnx_amd import session as ses
    import delivery_ref as dref
    segs, trims, shapes, limits = list(dref.GOOD), None, None, ses.Limit(0.5, 8)
    if name in ref.LIMIT_REFUSALS:
        raw, vol, index, words = ref.LIMIT_REFUSALS[name]
        limits = ses.RawLimits(raw)
        if vol is not None:
            segs[1] = segs[1]._replace(volume=vol)
    elif name == "a shape":            # everything vits_deliver_shaped refuses
        shapes, index, words = [ses.Shape(), ses.Shape(-4), ses.Shape()], 1, ("fade_in -4",)
    else:
        trims, index, words = [tref.OFF, Trim(3, 0.1, 0, 0, 0), tref.OFF], 1, ("mode 3",)
    x = np.ones((6, 16), F)
    dst = _canary()
    with pytest.raises(ses.SessionError, match=r"\[-3\]") as exc:
        ses.test_deliver_limited(x, dref.COUNTS, _segments(segs), limits, shapes, _trims(trims), None, 22050, 2, "pcm16", dst=dst)
    assert all(w in str(exc.value) for w in words) and f"segment {index}:" in str(exc.value)
    assert (dst == 0xA5).all()


# ------------------------------------------------------------------ through the engine

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _batch(s, seed=12, per_token=60):
    """three rows with forced durations, long enough for several 400 ms blocks each"""
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], per_token, 0).astype(np.int64)
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64), dur


def test_a_run_delivered_with_levels_and_limits_equals_the_host_fallback():
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd import session as ses
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, dur = _batch(s)
    s.reserve(3, 40, 40 * 60)
    cap = s.hparam("workspace_bytes")
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=dur)
    x = r["output"][:, 0, 0, :].copy()
    counts = np.asarray(r["y_lengths"] * s.hparam("hop"), np.int64)
    # row 0 levelled far up, row 1 normalised to full scale, row 2 as rendered times 4: each then meets a ceiling of half its
    # peak or less
    segs = [ses.Segment(0, 0, 5, 0, 1.0), ses.Segment(1, 1, 3, 1, 1.0), ses.Segment(2, 1, 0, 0, 4.0)]
    levels = [ses.Level(1, -3.0, 60.0, 0.0), ses.Level(), ses.Level()]
    trims = [ses.Trim(2, 0.05, 3, 5, 4), ses.Trim(0, 0.0, 0, 0, 7), ses.Trim(2, 0.1, 0, 0, 0)]
    shapes = [ses.Shape(40, 80, "smooth"), ses.Shape(), ses.Shape(0, 0, "linear", ((100, 1.0), (400, 0.5)))]
    peak2 = float(np.abs(x[2, :counts[2]]).max()) * 4.0
    limits = [ses.Limit(0.5, 110), ses.Limit(0.5, 16), ses.Limit(min(1.0, 0.5 * peak2), 255)]
    rate = s.delivered_rate
    for enc in ENCODINGS:
        d = s.synthesize_delivered(ids, lens, scales, sid, segments=segs, n_streams=2, encoding=enc, seeds=seeds, durations=dur,
                                   trim=trims, levels=levels, shapes=shapes, limits=limits)
        assert np.array_equal(d["sample_lengths"], counts) and counts.min() >= 0.8 * rate
        assert s.hparam("workspace_bytes") == cap, "a limited delivery allocated behind a reservation that covers the request"
        # the host fallback over the fetched waveform, segment by segment (the levelled one: by the gain the device reports)
        pieces = [[], []]
        for g, (sg, tr, sh, lm) in enumerate(zip(segs, trims, shapes, limits)):
            row = x[sg.row, :counts[sg.row]]
            if levels[g].mode:
                a, c = ae.trim_range(row, len(row), tr)
                v = ae.leveled(row[a:a + c], d["gain"][g], sg.volume, ae.shape_multiplier(a, c, sh), lm)
                data = np.concatenate([ae.silence(sg.lead_samples, enc), ae.encode(v, enc), ae.silence(tr.tail_samples, enc)])
            else:
                data, ((a, c),) = ae.join_trimmed([row], enc, sg.lead_samples, tr.tail_samples, tr, sg.normalize, sg.volume, shapes=[sh],
                                                  limits=[lm])
            assert (d["kept_first"][g], d["kept_count"][g]) == (a, c)
            pieces[sg.stream].append(data)
        _same(_bytes(d["streams"]), [np.concatenate(p).tobytes() for p in pieces], enc + " (fallback)")
        # the layout is the unlimited call's, the bytes are not: every limiter worked
        plain = s.deliver(segs, 2, enc, trims=trims, levels=levels, shapes=shapes)
        assert [len(p) for p in plain] == [len(q) for q in d["streams"]] and _bytes(plain) != _bytes(d["streams"])
        if enc == "f32":
            assert d["gain"][0] > 1 and np.isfinite(d["loudness"][0])
            n0 = 5 + int(d["kept_count"][0])
            assert np.abs(d["streams"][0][:n0]).max() <= F(0.5) < np.abs(plain[0][:n0]).max()
            assert np.abs(d["streams"][1]).max() <= max(F(0.5), F(limits[2].ceiling))
    # refusals leave the run deliverable
    with pytest.raises(ses.SessionError, match="segment 1: lookahead 2000"):
        s.deliver(segs, 2, "pcm16", limits=[None, ses.Limit(0.5, 2000), None])
    rows = np.empty_like(r["output"])
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])
    s.close()


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


class _NoDelivery:
    """the same session with the surface of one that cannot deliver: the voice takes the NumPy fallback"""

    def __init__(self, session):
        self._s = session
        for name in ("get_inputs", "hparam", "synthesize_batch", "last_durations"):
            setattr(self, name, getattr(session, name))


def _voice(session):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    n_vocab, n_spk = session.hparam("n_vocab"), session.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


def test_synthesize_encoded_stays_under_the_ceiling_and_keeps_the_layout():
    from phoonnx_amd.config import SynthesisConfig
    s = _session("tiny_rb2_ms")
    dev, host = _voice(s), _voice(_NoDelivery(s))
    # (a slow voice: the synthetic one renders a few frames per phoneme, and a sentence needs 400 ms to have a loudness)
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, length_scale=20.0, normalize_audio=False)
    text = "the quick brown fox jumps over the fence and runs away. a lazy dog sleeps in the warm sun all day long"
    for enc in ("pcm16", "ulaw"):
        kw = dict(encoding=enc, sentence_silence=0.01, trim_silence=0.01, trailing_silence=0.05, loudness=-10, max_gain_db=60.0)
        plain = dev.synthesize_encoded(text, cfg, **kw)
        d = dev.synthesize_encoded(text, cfg, **kw, limit_ceiling=0.5)
        assert d.sentence_starts == plain.sentence_starts and d.sentence_samples == plain.sentence_samples and len(d.data) == len(plain.data)
        assert d.gain == plain.gain and d.loudness == plain.loudness         # measured on the unlimited audio
        assert d.tobytes() != plain.tobytes()
        if enc == "pcm16":
            assert np.abs(d.data.astype(np.int32)).max() <= int(F(0.5) * F(32767.0)) < np.abs(plain.data.astype(np.int32)).max()
        # the host fallback over the same run limits as the device does: the layout is the same (its float64 loudness gives a
        # gain that agrees to meter accuracy, not bit for bit - so the bytes are compared where nothing is levelled)
        h = host.synthesize_encoded(text, cfg, **kw, limit_ceiling=0.5)
        assert h.sentence_starts == d.sentence_starts and h.sentence_samples == d.sentence_samples
        kw2 = dict(encoding=enc, sentence_silence=0.01, trim_silence=0.01, trailing_silence=0.05)
        loud = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, length_scale=4.0, normalize_audio=True, volume=1.0)
        d2, h2 = dev.synthesize_encoded(text, loud, **kw2, limit_ceiling=0.5, limit_lookahead=0.002), host.synthesize_encoded(
            text, loud, **kw2, limit_ceiling=0.5, limit_lookahead=0.002)
        assert d2.tobytes() == h2.tobytes() != dev.synthesize_encoded(text, loud, **kw2).tobytes()
    s.close()
