"""Shaped delivery on the GPU (include/vitsmi.h, "shaped delivery"): the shaped pack launch by value through
vits_test_deliver_shaped, on one batch with a row for each way it can go wrong; then the feature through MiSession and TTSVoice.

Reference: tests/shape_ref.py (NumPy float32) applied to the float waveform of the same run.  Bytes are exact (a levelled
segment's: given the gain the device reports, as in test_gpu_loudness.py)."""
import os

import numpy as np
import pytest

import delivery_ref as dref
import loudness_ref as lref
import shape_ref as ref
import trim_ref as tref
from conftest import GOLDEN
from delivery_ref import Seg
from shape_ref import RATE, Shape
from trim_ref import Trim

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
CURVE = {0: "linear", 1: "smooth"}


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


def _bytes(streams):
    return [np.ascontiguousarray(a).tobytes() for a in streams]


def _same(have, want, what):
    assert [len(g) for g in have] == [len(w) for w in want], what
    for j, (h, w) in enumerate(zip(have, want)):
        if h != w:
            a, b = np.frombuffer(h, np.uint8), np.frombuffer(w, np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what} stream {j}: {bad.size} of {a.size} bytes differ, first at {bad[:8]}")


# ------------------------------------------------------------------ by value

BATCH = ref.batch()
_KEPT = {}


def _kept():
    if not _KEPT:
        x, counts, segs, trims, *_ = BATCH
        _KEPT["kept"] = [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segs, trims)]
    return _KEPT["kept"]


def test_the_batch_covers_what_it_claims():
    """What the reference says of the by-value batch (no GPU work: it guards the case itself)."""
    x, counts, segs, trims, levels, shapes, J = BATCH
    kept = _kept()
    mul = [ref.multiplier(a, c, s) for (a, c), s in zip(kept, shapes)]
    valid = np.concatenate([x[b, :int(counts[b])] for b in range(len(counts))])
    assert np.all((valid == 0) | (np.abs(valid) >= 2.0 ** -20)) and np.isnan(x[0, int(counts[0]):]).all()
    # 1: no shape between shaped neighbours, and the boundaries fall inside a 16-byte cell in every encoding
    assert shapes[1] == ref.NONE and (mul[1] == 1).all() and shapes[0] != ref.NONE and shapes[2] != ref.NONE
    assert [segs[g].stream for g in (0, 1, 2)] == [0, 0, 0] and all(segs[g].lead_samples == 0 for g in (1, 2))
    assert kept[0][1] % 16 and (kept[0][1] + kept[1][1]) % 16
    # 2, 3: fades only, c = 3000, 441 and 1000, linear and smooth; 4: overlapping fades
    for g, cv in ((2, 0), (3, 1)):
        assert kept[g] == (0, 3000) and shapes[g] == Shape(441, 1000, cv, ())
        assert mul[g][0] == 0 and mul[g][-1] == 0 and (mul[g][441:2000] == 1).all()
    assert not np.array_equal(mul[2], mul[3])
    assert shapes[4].fade_in + shapes[4].fade_out > kept[4][1] and (mul[4][31:79] < 1).all() and mul[4].max() < 1
    # 5 .. 7: c = 0, 1, 2 with fades of 1 and 5
    assert [kept[g][1] for g in (5, 6, 7)] == [0, 1, 2] and {shapes[g].fade_in for g in (5, 6, 7)} == {1, 5}
    assert mul[6].tolist() == [0.0] and mul[7].tolist() == [0.0, 0.0]
    # 8, 9: points only; more than one tile in every encoding; a single point; two points one sample apart; 600 points 1 to 3
    # apart; points beyond the row's end
    pos = np.array([p for p, _ in shapes[8].points])
    assert kept[8] == (0, 9000) and 9000 > 2 * 4096 and shapes[8].fade_in == shapes[8].fade_out == 0
    d = np.diff(pos)
    assert (d > 0).all() and d[0] == 1 and ((d >= 1) & (d <= 3)).sum() >= 600 and (pos >= 9000).sum() == 2
    run = pos[(pos > 4000) & (pos < 6000)]
    assert run.size == 600 and max((run < lo + 256).sum() - (run < lo).sum() for lo in range(4000, 5000, 64)) > 100     # many points a pass
    assert len(shapes[9].points) == 1 and (mul[9] == 0.5).all()
    # 10: points, fades and a trim with a > 0; points in front of a and behind a + c
    a, c = kept[10]
    p10 = [p for p, _ in shapes[10].points]
    assert a > 0 and c < counts[10] and sum(p < a for p in p10) >= 2 and sum(p >= a + c for p in p10) >= 2 and sum(a < p < a + c for p in p10) >= 3
    assert shapes[10].fade_in and shapes[10].fade_out
    wrong = ref.multiplier(0, c, shapes[10])                # the envelope taken in kept-range coordinates: not the same
    assert not np.array_equal(wrong, mul[10])
    # 11: levelled with a shape; 12 .. 14: normalize 1 and 2 with shapes
    assert levels[11].mode == 1 and shapes[11] != ref.NONE and segs[11].normalize == 0 and kept[11][1] >= 0.4 * RATE
    assert segs[12].normalize == 1 and segs[13].normalize == 2 and segs[14].normalize == 2 and segs[13].stream == segs[14].stream
    assert all(shapes[g] != ref.NONE for g in (12, 13, 14))
    # 15: a gain-0 plateau; 16: a gain of 4 that clips
    assert (mul[15][110:201] == 0).all() and mul[15][105] == 0.5 and (mul[15][:100] == 1).all()
    assert (mul[16] == 4).all() and (np.abs(x[16, :int(counts[16])]) * 4 > 1).all()
    assert len(segs) == 17 and J == 8


def _want(encoding, gains):
    x, counts, segs, trims, levels, shapes, J = BATCH
    return ref.deliver_ref(x, counts, segs, trims, levels, shapes, J, encoding, gains)


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_shaped_delivery_by_value(encoding):
    from phoonnx_amd.session import test_deliver_leveled, test_deliver_shaped
    x, counts, segs, trims, levels, shapes, J = BATCH
    got = test_deliver_shaped(x, counts, _segments(segs), _shapes(shapes), _trims(trims), _levels(levels), RATE, J, encoding)
    want, kept = _want(encoding, got["gain"])
    assert got["kept_first"].tolist() == [a for a, _ in kept] and got["kept_count"].tolist() == [c for _, c in kept]
    _same(_bytes(got["streams"]), want, encoding)
    # peaks, kept ranges, loudness and gain are those of the unshaped audio
    base = test_deliver_leveled(x, counts, _segments(segs), _levels(levels), RATE, _trims(trims), J, encoding)
    assert np.array_equal(base["gain"].view(np.uint32), got["gain"].view(np.uint32)) and base["loudness"][11] == got["loudness"][11]
    loud, gain, _ = lref.measure(x, counts, segs, trims, levels, J, RATE)
    assert abs(got["loudness"][11] - loud[11]) < 0.1 and abs(20 * np.log10(got["gain"][11] / gain[11])) < 0.1
    for key in ("stream_samples", "stream_offsets", "kept_first", "kept_count"):
        assert np.array_equal(base[key], got[key]), key                          # the layout never depends on the shapes
    assert _bytes(base["streams"]) != _bytes(got["streams"])
    # the layout alone (dst = NULL)
    lay = test_deliver_shaped(x, counts, _segments(segs), _shapes(shapes), _trims(trims), _levels(levels), RATE, J, encoding,
                              layout_only=True)
    assert lay["streams"] is None and np.array_equal(lay["stream_offsets"], got["stream_offsets"])


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_without_shapes_it_is_the_levelled_delivery(encoding):
    from phoonnx_amd import session as ses
    x, counts, segs, trims, levels, _, J = BATCH
    base = ses.test_deliver_leveled(x, counts, _segments(segs), _levels(levels), RATE, _trims(trims), J, encoding)
    for shapes in (None, [ses.Shape()] * len(segs), ses.Shape(0, 0, "smooth")):
        got = ses.test_deliver_shaped(x, counts, _segments(segs), shapes, _trims(trims), _levels(levels), RATE, J, encoding)
        assert _bytes(got["streams"]) == _bytes(base["streams"])
        for key in ("stream_samples", "stream_offsets", "kept_first", "kept_count"):
            assert np.array_equal(base[key], got[key]), key
        assert np.array_equal(base["gain"].view(np.uint32), got["gain"].view(np.uint32))
    # ... and without trims and levels too: the delivery
    plain = ses.test_deliver_shaped(np.nan_to_num(x, nan=0.25), counts, _segments(segs), None, None, None, RATE, J, encoding)
    assert _bytes(plain["streams"]) == dref.deliver_ref(np.nan_to_num(x, nan=0.25), counts, segs, J, encoding)


def _canary():
    return np.full(4096, 0xA5, np.uint8)


@pytest.mark.parametrize("name", sorted(ref.SHAPE_REFUSALS) + ["a trim", "a level", "a segment"])
def test_refusals_write_nothing(name):
    from phoonnx_amd import session as ses
    segs, trims, levels, J, shapes = dref.GOOD, None, None, 2, ses.Shape(2, 2)
    if name in ref.SHAPE_REFUSALS:
        records, points, stated, index, words = ref.SHAPE_REFUSALS[name]
        shapes = ses.RawShapes(records, points, stated)
    elif name == "a trim":            # everything vits_deliver_leveled refuses
        trims, index, words = [tref.OFF, Trim(3, 0.1, 0, 0, 0), tref.OFF], 1, ("mode 3",)
    elif name == "a level":
        segs = [s._replace(normalize=0) for s in dref.GOOD]
        levels, index, words = [lref.OFF, lref.OFF, lref.Level(1, 0.5, 30.0, 0.0)], 2, ("target_lufs 0.5",)
    else:
        segs, index, words = dref.GOOD[:1] + [Seg(2, 2, 0, 1, 1.0)], 1, ("stream 2",)
    x = np.ones((6, 16), np.float32)
    dst = _canary()
    with pytest.raises(ses.SessionError, match=r"\[-3\]") as exc:
        ses.test_deliver_shaped(x, dref.COUNTS, _segments(segs), shapes, _trims(trims), _levels(levels), 22050, J, "pcm16", dst=dst)
    assert all(w in str(exc.value) for w in words) and (index is None or f"segment {index}:" in str(exc.value))
    assert (dst == 0xA5).all()


# ------------------------------------------------------------------ through the engine

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _batch(s, seed=12):
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64)


def _token_db(lens, T):
    rng = np.random.default_rng(3)
    db = rng.choice([0.0, 0.0, -6.0, 3.0, -np.inf, -40.0], (len(lens), T))
    db[1, :] = -3.0             # one row at one gain: a single point
    db[2, :] = 0.0              # one row untouched: no points
    return db


@pytest.mark.parametrize("rate", [None, 8000])
def test_token_gains_of_a_run(rate):
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd import session as ses
    s = _session("tiny_rb2_ms", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    x = r["output"][:, 0, 0, :].copy()
    counts = np.asarray(r["sample_lengths"] if rate else r["y_lengths"] * s.hparam("hop"), np.int64)
    db = _token_db(lens, ids.shape[1])
    segs = [Seg(2, 0, 5, 2, 0.5), Seg(0, 0, 5, 2, 0.5), Seg(1, 1, 3, 0, 2.5)]
    trims = [Trim(2, 0.5, 3, 5, 4), Trim(2, 0.5, 3, 5, 4), Trim(0, 0.0, 0, 0, 7)]
    fades = [ses.Shape(40, 80, "smooth"), ses.Shape(), ses.Shape(0, 100, "linear")]
    L, M = ses.resample_plan(int(s.meta("sample_rate") or 22050), rate)[:2] if rate else (1, 1)
    gains = ses.token_gains(db, *db.shape)
    ramp = int(s.delivered_rate * 0.004)
    assert ramp >= 8
    for enc in ("pcm16", "ulaw") if rate else ENCODINGS:
        d = s.synthesize_delivered(ids, lens, scales, sid, segments=_segments(segs), n_streams=2, encoding=enc, seeds=seeds,
                                   trim=_trims(trims), shapes=fades, token_gain_db=db, gain_ramp=0.004, return_durations=True)
        assert np.array_equal(d["durations"], r["durations"]) and np.array_equal(d["sample_lengths"], counts)
        # the points are token_envelope of that run's durations
        for g, sh, fade in zip(segs, d["shapes"], fades):
            e = np.concatenate([[0], np.cumsum(r["durations"][g.row])]) * s.hparam("hop")
            bounds = np.minimum(counts[g.row], -(-e * L // M))
            assert bounds[lens[g.row]] == counts[g.row]
            assert list(sh.points) == ses.token_envelope(bounds, gains[g.row], ramp)
            assert (sh.fade_in, sh.fade_out, sh.curve) == (fade.fade_in, fade.fade_out, fade.curve)
        assert len(d["shapes"][1].points) > 4 and list(d["shapes"][2].points) == [(0, float(np.float32(10 ** (-3.0 / 20))))]
        assert list(d["shapes"][0].points) == []
        # the bytes are the host fallback's over the waveform of the identical run, stream by stream ...
        rows = [x[g.row, :counts[g.row]] for g in segs]
        s0, k0 = ae.join_trimmed(rows[:2], enc, 5, 4, trims[0], 2, 0.5, shapes=d["shapes"][:2])
        s1, k1 = ae.join_trimmed(rows[2:], enc, 3, 7, trims[2], 0, 2.5, shapes=d["shapes"][2:])
        _same(_bytes(d["streams"]), [s0.tobytes(), s1.tobytes()], enc + " (fallback)")
        assert d["kept_first"].tolist() == [a for a, _ in k0 + k1] and d["kept_count"].tolist() == [c for _, c in k0 + k1]
        assert any(a > 0 for a, _ in k0)
        # ... and the reference's
        mine = [Shape(sh.fade_in, sh.fade_out, {"linear": 0, "smooth": 1}[sh.curve], tuple(sh.points)) for sh in d["shapes"]]
        _same(_bytes(d["streams"]), ref.deliver_ref(x, counts, segs, trims, None, mine, 2, enc)[0], enc)
        plain = s.deliver(_segments(segs), 2, enc, trims=_trims(trims))
        assert _bytes(plain) != _bytes(d["streams"]) and [len(p) for p in plain] == [len(q) for q in d["streams"]]
    # refusals leave the run deliverable
    with pytest.raises(ses.SessionError, match="explicit points"):
        s.synthesize_delivered(ids, lens, scales, sid, segments=_segments(segs), n_streams=2, shapes=ses.Shape(points=((0, 0.5),)),
                               token_gain_db=db)
    with pytest.raises(ses.SessionError, match="segment 1: fade_in -4"):
        s.deliver(_segments(segs), 2, "pcm16", shapes=[ses.Shape(), ses.Shape(-4), ses.Shape()])
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


def test_synthesize_encoded_shapes_on_the_device_as_the_fallback_does():
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd.config import SynthesisConfig
    s = _session("tiny_rb2_ms")
    assert s.delivered_rate == 22050
    dev, host = _voice(s), _voice(_NoDelivery(s))
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=True)
    text = "the quick brown fox. jumps over. a lazy dog"
    gain = lambda k, tokens: [(-np.inf if t == "o" else 5.0 if t in "aeiu" else 0.0) - 3.0 * k for t in tokens]
    for enc in ("ulaw", "pcm16"):
        kw = dict(encoding=enc, sentence_silence=0.01, trim_silence=0.01, trailing_silence=0.05, alignments=True)
        plain = dev.synthesize_encoded(text, cfg, **kw)
        more = dict(fade_in=0.005, fade_out=0.02, phoneme_gain_db=gain)
        d, h = dev.synthesize_encoded(text, cfg, **kw, **more), host.synthesize_encoded(text, cfg, **kw, **more)
        assert d.tobytes() == h.tobytes() != plain.tobytes() and len(d.sentence_samples) == 3
        assert d.sentence_starts == h.sentence_starts == plain.sentence_starts and d.sentence_samples == plain.sentence_samples
        zero = ae.encode(np.zeros(1, np.float32), enc)[0]
        for st, n in zip(d.sentence_starts, d.sentence_samples):
            assert n > int(22050 * 0.02) and d.data[st] == zero and d.data[st + n - 1] == zero
        assert any(plain.data[st] != zero or plain.data[st + n - 1] != zero for st, n in zip(plain.sentence_starts, plain.sentence_samples))
        for ad, ah in zip(d.phoneme_alignments, h.phoneme_alignments):
            assert [(p.phoneme, p.start_sample, p.num_samples) for p in ad] == [(p.phoneme, p.start_sample, p.num_samples) for p in ah]
        # the requests entry: the same sentences, each a stream of its own
        rd = dev.synthesize_requests_encoded([(text, cfg)], seeds=[7], **{k: v for k, v in kw.items() if k != "alignments"}, **more)
        rh = host.synthesize_requests_encoded([(text, cfg)], seeds=[7], **{k: v for k, v in kw.items() if k != "alignments"}, **more)
        assert rd[0].tobytes() == rh[0].tobytes() and rd[0].sentence_samples == rh[0].sentence_samples
    s.close()
