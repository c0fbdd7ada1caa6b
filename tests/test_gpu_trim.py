"""Trimmed delivery on the GPU (include/vitsmi.h, "trimmed delivery"): the scan and the delivery over kept ranges by value
through vits_test_deliver_trimmed, on one batch with a row for each way the scan can go wrong; then the feature through
MiSession and TTSVoice.

Reference: tests/trim_ref.py applied to the float waveform of the same run.  Bytes, kept ranges and layout are exact."""
import os

import numpy as np
import pytest

import delivery_ref as dref
import trim_ref as ref
from conftest import GOLDEN
from delivery_ref import Seg
from trim_ref import OFF, Trim

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")


def _segments(segs):
    from phoonnx_amd.session import Segment
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _trims(trims):
    from phoonnx_amd import session as ses
    return None if trims is None else [ses.Trim(*t) for t in trims]


def _bytes(streams):
    return [np.ascontiguousarray(a).tobytes() for a in streams]


# ------------------------------------------------------------------ by value

BATCH = ref.batch()
_WANT = {}


def _want(encoding):
    if encoding not in _WANT:
        _WANT[encoding] = ref.deliver_ref(*BATCH[:4], BATCH[4], encoding)
    return _WANT[encoding]


def test_the_batch_covers_what_it_claims():
    """What the reference says of the by-value batch (no GPU work: it guards the case itself)."""
    x, counts, segs, trims, J = BATCH
    _, first, count = _want("f32")
    kept = {s.row: (int(a), int(c)) for s, a, c in zip(segs, first, count)}
    n = {b: int(counts[b]) for b in range(len(counts))}
    assert kept[0] == (0, 300) and n[0] % 64 and n[0] % 256            # active at index 0 and at n - 1: nothing to cut
    assert kept[1] == (417 - 10, 31)                                   # exactly one active sample, negative, with its margins
    assert kept[2] == (0, 0) and kept[3] == (0, 0) and n[2] > 0 and n[3] > 0       # below the threshold; equal to it
    assert np.all(np.abs(x[3, :n[3]]) == np.float32(0.25)) and trims[6].threshold == 0.25
    assert kept[4] == (0, 0) and n[4] == 0
    assert kept[5] == (98, 305) and (x[5, :n[5]] <= 0.01).all() and x[5, n[5]] == 100.0       # only negative; 100 behind n is not the peak
    assert n[6] > 65536 and kept[6] == (4900, 69000 + 1 + 100 - 4900)
    assert kept[7] == (0, 0) and trims[4].mode == 2 and trims[4].threshold >= 1 and segs[4].normalize == 2
    assert kept[8] == (0, 90) and trims[8].keep_lead > 3 and trims[8].keep_tail > 10          # margins clipped at both ends
    assert kept[9] == (0, 65) and trims[9].mode == 0
    front = sum(1 for r, (a, c) in kept.items() if a > 0)
    back = sum(1 for r, (a, c) in kept.items() if c > 0 and a + c < n[r])
    empty = sum(1 for r, (a, c) in kept.items() if c == 0 and n[r] > 0)
    assert front >= 3 and back >= 3 and empty >= 3
    assert {s.normalize for s in segs} == {0, 1, 2}
    assert any(t.tail_samples and s.lead_samples for s, t in zip(segs, trims)) and any(t.tail_samples and not s.lead_samples for s, t in zip(segs, trims))


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_trimmed_delivery_by_value(encoding):
    from phoonnx_amd.session import test_deliver_trimmed
    x, counts, segs, trims, J = BATCH
    want, first, count = _want(encoding)
    got = test_deliver_trimmed(x, counts, _segments(segs), _trims(trims), J, encoding)
    assert np.array_equal(got["kept_first"], first), (got["kept_first"], first)
    assert np.array_equal(got["kept_count"], count), (got["kept_count"], count)
    kept = np.zeros(len(counts), np.int64)
    for s, c in zip(segs, count):
        kept[s.row] = c
    samples, offsets, total = ref.plan_ref(kept, segs, trims, J, encoding)
    assert np.array_equal(got["stream_samples"], samples) and np.array_equal(got["stream_offsets"], offsets)
    have = _bytes(got["streams"])
    assert [len(g) for g in have] == [len(w) for w in want]
    for j in range(J):
        if have[j] != want[j]:
            a, b = np.frombuffer(have[j], np.uint8), np.frombuffer(want[j], np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{encoding} stream {j}: {bad.size} of {a.size} bytes differ, first at {bad[:8]}")
    # the layout alone (dst = NULL): the scan runs, the same kept ranges and layout
    lay = test_deliver_trimmed(x, counts, _segments(segs), _trims(trims), J, encoding, layout_only=True)
    assert lay["streams"] is None and np.array_equal(lay["kept_first"], first) and np.array_equal(lay["kept_count"], count)
    assert np.array_equal(lay["stream_offsets"], offsets)


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_without_trims_it_is_the_delivery(encoding):
    from phoonnx_amd.session import test_deliver, test_deliver_trimmed
    x, counts, segs, _, J = BATCH
    x = np.nan_to_num(x[:, :1024], nan=0.5)               # (the untrimmed delivery reads whole rows: short ones)
    counts = np.minimum(counts, 1000)
    base = _bytes(test_deliver(x, counts, _segments(segs), J, encoding))
    assert base == dref.deliver_ref(x, counts, segs, J, encoding)
    for trims in (None, [OFF] * len(segs), [Trim(0, 0.9, 50, 50, 0)] * len(segs)):
        got = test_deliver_trimmed(x, counts, _segments(segs), _trims(trims), J, encoding)
        assert _bytes(got["streams"]) == base
        assert np.array_equal(got["stream_samples"], dref.plan_ref(counts, segs, J, encoding)[0])
        assert np.array_equal(got["stream_offsets"], dref.plan_ref(counts, segs, J, encoding)[1])
        assert not got["kept_first"].any() and np.array_equal(got["kept_count"], [counts[s.row] for s in segs])


def _canary():
    return np.full(4096, 0xA5, np.uint8)


@pytest.mark.parametrize("name", sorted(ref.TRIM_REFUSALS) + sorted(dref.REFUSALS))
def test_refusals_write_nothing(name):
    from phoonnx_amd.session import SessionError, test_deliver_trimmed
    if name in ref.TRIM_REFUSALS:
        trims, index, word = ref.TRIM_REFUSALS[name]
        segs, J, enc = dref.GOOD, 2, "pcm16"
    else:
        segs, J, enc, index, word = dref.REFUSALS[name]
        trims = [Trim(2, 0.5, 0, 0, 1)] * len(segs)
    x = np.ones((6, 16), np.float32)
    dst = _canary()
    with pytest.raises(SessionError, match=r"\[-3\]") as exc:
        test_deliver_trimmed(x, dref.COUNTS, _segments(segs), _trims(trims), J, enc, dst=dst)
    assert word in str(exc.value) and (index is None or f"segment {index}:" in str(exc.value))
    assert (dst == 0xA5).all()


def test_a_short_buffer_is_refused_behind_the_scan():
    from phoonnx_amd.session import SessionError, test_deliver_trimmed
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.01, 0.01, (6, 16)).astype(np.float32)
    x[0, 1:4] = 0.5
    x[2, 2:7] = -0.5
    x[3, 1] = 0.5
    trims = [Trim(1, 0.25, 0, 0, 0), Trim(1, 0.25, 1, 1, 0), Trim(1, 0.25, 0, 0, 3)]
    want, first, count = ref.deliver_ref(x, dref.COUNTS, dref.GOOD, trims, 2, "pcm16")
    assert count.tolist() == [3, 6, 1] and first.tolist() == [1, 1, 1]
    need = sum(len(w) for w in want)
    assert need < dref.plan_ref(dref.COUNTS, dref.GOOD, 2, "pcm16")[2]          # (shorter than the untrimmed delivery)
    dst = _canary()
    with pytest.raises(SessionError, match=f"{need} needed"):
        test_deliver_trimmed(x, dref.COUNTS, _segments(dref.GOOD), _trims(trims), 2, "pcm16", dst=dst[:need - 1])
    assert (dst == 0xA5).all()
    got = test_deliver_trimmed(x, dref.COUNTS, _segments(dref.GOOD), _trims(trims), 2, "pcm16", dst=dst[:need])
    assert _bytes(got["streams"]) == want and (dst[need:] == 0xA5).all()


# ------------------------------------------------------------------ through a session

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


# the synthetic voices render no silence: a relative threshold of 0.5 moves both ends of some row (asserted)
PLANS = {"one stream, leads and tails": ([Seg(2, 0, 11, 2, 0.5), Seg(0, 0, 0, 2, 0.5), Seg(1, 0, 3, 0, 2.5)],
                                         [Trim(2, 0.5, 0, 0, 4), Trim(2, 0.5, 3, 5, 0), Trim(2, 0.5, 0, 0, 7)], 1),
         "one row per stream, one off": ([Seg(b, b, 0, 1, 1.0) for b in range(3)], [Trim(2, 0.5, 2, 2, 1), OFF, Trim(1, 0.05, 0, 0, 0)], 3)}


def _check_run(s, x, counts, plans=PLANS, encodings=ENCODINGS):
    moved = 0
    for name, (segs, trims, J) in plans.items():
        segs = [g for g in segs if g.row < x.shape[0]]
        trims = trims[:len(segs)]
        for enc in encodings:
            want, first, count = ref.deliver_ref(x, counts, segs, trims, J, enc)
            got, kf, kc = s.deliver(_segments(segs), J, enc, trims=_trims(trims), return_kept=True)
            assert np.array_equal(kf, first) and np.array_equal(kc, count), (name, enc, kf, first, kc, count)
            assert _bytes(got) == want, (name, enc)
            assert [g.dtype for g in got] == [np.dtype(dref.DTYPE[enc])] * J
        moved += sum(1 for g, a, c in zip(segs, first, count) if a > 0 and 0 < a + c < counts[g.row])
    assert moved >= 1, "the threshold moved both ends of no row"


@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_trimmed_delivery_of_a_run(preset):
    s = _session(preset)
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = r["output"][:, 0, 0, :].copy(), np.asarray(r["y_lengths"] * s.hparam("hop"), np.int64)
    _check_run(s, x, counts)
    # the layout alone, then the real call: they agree
    segs, trims, J = PLANS["one stream, leads and tails"]
    lay = s.deliver_layout(_segments(segs), J, "ulaw", trims=_trims(trims))
    got, kf, kc = s.deliver(_segments(segs), J, "ulaw", trims=_trims(trims), return_kept=True)
    assert np.array_equal(lay["kept_first"], kf) and np.array_equal(lay["kept_count"], kc)
    assert lay["stream_samples"].tolist() == [len(g) for g in got] and lay["stream_offsets"][-1] == sum(g.nbytes for g in got)
    # without trims: the delivery; and the run is still there
    assert _bytes(s.deliver(_segments(segs), J, "alaw", trims=_trims([OFF] * 3))) == _bytes(s.deliver(_segments(segs), J, "alaw"))
    rows = np.empty_like(r["output"])
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])
    # run and trimmed delivery in one call
    d = s.synthesize_delivered(ids, lens, scales, sid, segments=_segments(segs), n_streams=J, encoding="pcm16", seeds=seeds,
                               trim=_trims(trims))
    want, first, count = ref.deliver_ref(x, counts, segs, trims, J, "pcm16")
    assert _bytes(d["streams"]) == want and np.array_equal(d["kept_first"], first) and np.array_equal(d["kept_count"], count)
    # a refused trim leaves the run deliverable
    from phoonnx_amd.session import SessionError
    with pytest.raises(SessionError, match="segment 1: trim mode 3"):
        s.deliver(_segments(segs), J, "pcm16", trims=_trims([OFF, Trim(3, 0.1, 0, 0, 0), OFF]))
    assert _bytes(s.deliver(_segments(segs), J, "pcm16", trims=_trims(trims))) == want
    s.close()


@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_trimmed_delivery_at_an_output_rate(preset):
    s = _session(preset, output_rate=8000)
    ids, lens, scales, sid, seeds = _batch(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    x, counts = r["output"][:, 0, 0, :].copy(), np.asarray(r["sample_lengths"], np.int64)
    _check_run(s, x, counts, encodings=("ulaw", "alaw"))
    rows = np.empty_like(r["output"])
    s._fetch(rows, 0, 3)
    assert np.array_equal(rows, r["output"])        # delivering did not move what it delivered
    s.close()


@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_trimmed_delivery_after_the_vocoder(preset):
    s = _session(preset)
    hop, F = s.hparam("hop"), 23
    z = np.random.default_rng(5).standard_normal((2, s.hparam("inter"), F)).astype(np.float32)
    sid = np.array([1, 0], np.int64) if s.hparam("n_speakers") > 1 else None
    for rate in (None, 8000):
        s.set_output_rate(rate)
        x = s.vocoder(z, sid)[:, 0, 0, :]
        n = x.shape[1]
        plans = {"two rows": ([Seg(1, 0, 2, 1, 1.0), Seg(0, 0, 0, 0, 0.5)], [Trim(2, 0.5, 1, 1, 3), Trim(2, 0.5, 0, 0, 0)], 1)}
        _check_run(s, x, np.array([n, n], np.int64), plans, ("pcm16", "ulaw"))
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_a_reservation_covers_the_trimmed_delivery(rate):
    s = _session("tiny_rb1", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 120, 0).astype(np.int64)
    F = 40 * 120
    s.reserve(3, 40, F)
    cap = s.hparam("workspace_bytes")
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=dur)
    assert int(r["y_lengths"].max()) == F and s.hparam("workspace_bytes") == cap
    x = r["output"][:, 0, 0, :].copy()
    counts = np.asarray(r["sample_lengths"] if rate else r["y_lengths"] * s.hparam("hop"), np.int64)
    segs, trims, J = PLANS["one stream, leads and tails"]
    for enc in ENCODINGS:
        want = ref.deliver_ref(x, counts, segs, trims, J, enc)[0]
        assert _bytes(s.deliver(_segments(segs), J, enc, trims=_trims(trims))) == want, enc
        assert s.hparam("workspace_bytes") == cap, (enc, "a trimmed delivery allocated behind a reservation that covers the request")
    s.close()


# ------------------------------------------------------------------ the voice layer

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


def test_synthesize_encoded_trims_on_the_device_as_the_fallback_does():
    from phoonnx_amd.config import SynthesisConfig
    s = _session("tiny_rb2_ms")
    dev, host = _voice(s), _voice(_NoDelivery(s))
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=True)
    text = "the quick brown fox. jumps over. a lazy dog"
    plain = dev.synthesize_encoded(text, cfg, encoding="ulaw", sentence_silence=0.01)
    for scope in ("sentence", "text"):
        kw = dict(encoding="ulaw", sentence_silence=0.01, normalize_scope=scope, alignments=True, trim_silence=0.5, trailing_silence=0.1)
        d, h = dev.synthesize_encoded(text, cfg, **kw), host.synthesize_encoded(text, cfg, **kw)
        assert d.tobytes() == h.tobytes() and len(d.sentence_samples) == 3
        assert d.sentence_starts == h.sentence_starts and d.sentence_samples == h.sentence_samples
        assert any(c < n for c, n in zip(d.sentence_samples, plain.sentence_samples))
        tail = int(22050 * 0.1 * 2) // 2
        assert len(d.data) == sum(d.sentence_samples) + 3 * (220 + tail)
        for ad, ah, st, n in zip(d.phoneme_alignments, h.phoneme_alignments, d.sentence_starts, d.sentence_samples):
            assert [(p.phoneme, p.start_sample, p.num_samples) for p in ad] == [(p.phoneme, p.start_sample, p.num_samples) for p in ah]
            assert ad[0].start_sample == st and sum(p.num_samples for p in ad) == n
    s.close()
