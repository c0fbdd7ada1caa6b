"""Levelled delivery on the GPU (include/vitsmi.h, "levelled delivery"): the sub-block energies of the loudness kernels by value
through vits_test_loudness_blocks, the levelled delivery through vits_test_deliver_leveled, then the feature through MiSession
and TTSVoice.

Reference: tests/loudness_ref.py (float64).  Energies and loudness are held to the meter tolerance of EBU Tech 3341, 0.1 LU;
bytes are exact given the gains the device reports; repeatability and independence are bit for bit."""
import math
import os

import numpy as np
import pytest

import delivery_ref as dref
import loudness_ref as ref
import trim_ref as tref
from conftest import GOLDEN
from delivery_ref import Seg
from loudness_ref import Level
from trim_ref import Trim

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
LC = 1024          # the compiled chunk (asserted against what the library reports)


def _segments(segs):
    from phoonnx_amd.session import Segment
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _trims(trims):
    from phoonnx_amd import session as ses
    return None if trims is None else [ses.Trim(*t) for t in trims]


def _levels(levels):
    from phoonnx_amd import session as ses
    return None if levels is None else [ses.Level(*l) for l in levels]


def _bytes(streams):
    return [np.ascontiguousarray(a).tobytes() for a in streams]


# ------------------------------------------------------------------ sub-block energies, by value

def _energy_batch(fs):
    """One launch at rate fs: every length at which the kernels take another path, a row that starts at an odd sample, and
    the gating signal of both rates; NaN behind every row's end (and in front of the odd start).
    -> (x, counts, firsts)"""
    hop = ref.hop(fs)
    lengths = [0, 1, hop - 1, hop, 4 * hop - 1, 4 * hop, 4 * hop + 1, LC - 1, LC, LC + 1, 3 * LC + 17]
    signals = [ref.gating_signal(22050), ref.gating_signal(8000)]
    rng = np.random.default_rng(fs)
    rows = [(rng.uniform(-0.5, 0.5, n) + 0.3 * np.sin(0.05 * np.arange(n))).astype(np.float32) for n in lengths]
    rows.append((0.4 * np.sin(0.11 * np.arange(5 * hop + 77))).astype(np.float32))        # the odd start
    rows += signals
    firsts = np.zeros(len(rows), np.int64)
    firsts[len(lengths)] = 1023
    S = max(len(r) + int(f) for r, f in zip(rows, firsts)) + 5
    x = np.full((len(rows), S), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, firsts[b]:firsts[b] + len(r)] = r
    return x, np.array([len(r) for r in rows], np.int64), firsts


_ENERGY = {}


def _energy_case(fs):
    """the batch of a rate and its float64 reference, computed once"""
    if fs not in _ENERGY:
        x, counts, firsts = _energy_batch(fs)
        want = [ref.sub_blocks(x[b, firsts[b]:firsts[b] + counts[b]], fs) for b in range(len(counts))]
        _ENERGY[fs] = (x, counts, firsts, want)
    return _ENERGY[fs]


@pytest.mark.parametrize("fs", [22050, 8000])
def test_sub_block_energies_against_the_float64_reference(fs):
    """The tolerance is the standard's own, per sub-block: 0.1 LU where the sub-block's mean square reaches the absolute
    gate's z0, the same as an absolute bound (10^0.01 - 1) hop z0 below it."""
    from phoonnx_amd.session import test_loudness_blocks
    x, counts, firsts, want = _energy_case(fs)
    hop = ref.hop(fs)
    got, chunk = test_loudness_blocks(x, counts, fs, firsts)
    assert chunk == LC
    z0 = 10.0 ** ((-70.0 + 0.691) / 10.0)
    worst, checked = 0.0, 0
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size == counts[b] // hop, (b, g.size, w.size)
        assert np.isfinite(g).all(), (b, "what lies outside the kept range showed")
        loud = w / hop >= z0
        if loud.any():
            dev = 10.0 * np.abs(np.log10(g[loud].astype(np.float64) / w[loud]))
            worst = max(worst, float(dev.max()))
            assert dev.max() <= 0.1, (fs, b, float(dev.max()))
        if (~loud).any():
            assert np.abs(g[~loud] - w[~loud]).max() <= (10.0 ** 0.01 - 1.0) * hop * z0, (fs, b)
        checked += g.size
    print(f"loudness kernels at {fs} Hz: {checked} sub-blocks, largest deviation {worst:.2e} dB")
    # the lengths did what they are there for
    n_sub = [g.size for g in got]
    assert n_sub[:7] == [0, 0, 0, 1, 3, 4, 4] and n_sub[11] == 5
    assert n_sub[12:] == [len(ref.gating_signal(r)) // hop for r in (22050, 8000)]
    # ... and the gates over the device's energies read what the reference reads
    from phoonnx_amd.session import loudness_gate
    sig = 12 if fs == 22050 else 13
    L, nb, na, nr = loudness_gate([got[sig]], hop)
    assert (nb, na, nr) == (37, 35, 30) and abs(L - ref.gate([want[sig]], fs)[0]) <= 0.1


@pytest.mark.parametrize("fs", [22050, 8000])
def test_energies_are_repeatable_and_depend_on_the_row_alone(fs):
    from phoonnx_amd.session import test_loudness_blocks
    x, counts, firsts, _ = _energy_case(fs)
    first, _ = test_loudness_blocks(x, counts, fs, firsts)
    again, _ = test_loudness_blocks(x, counts, fs, firsts)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    # the 4 s signal and the odd-start row: alone (B = 1), and as row 5 of 7 beside longer and shorter rows, at another
    # place in its buffer
    for src in (12 if fs == 22050 else 13, 11, 10):
        n, f = int(counts[src]), int(firsts[src])
        row = x[src, f:f + n]
        alone, _ = test_loudness_blocks(row[None, :].copy(), [n], fs)
        assert alone[0].tobytes() == first[src].tobytes(), src
        others = [0, 9, 12, 3, 13, None, 7]
        S = int(max(counts.max(), n + 3)) + 9
        y = np.full((7, S), np.nan, np.float32)
        c7, f7 = np.zeros(7, np.int64), np.zeros(7, np.int64)
        for b, o in enumerate(others):
            if o is None:
                y[b, 3:3 + n], c7[b], f7[b] = row, n, 3
            else:
                m, fo = int(counts[o]), int(firsts[o])
                y[b, :m], c7[b] = x[o, fo:fo + m], m
        beside, _ = test_loudness_blocks(y, c7, fs, f7)
        assert beside[5].tobytes() == first[src].tobytes(), src
        assert beside[2].tobytes() == first[12].tobytes()


# ------------------------------------------------------------------ the levelled delivery, by value

FS = 8000


def _delivery_batch():
    """6 rows over 3 streams at 8 kHz: leads, trims on some, modes 0, 1 and 2 mixed, a ceiling that binds, a row under 400 ms.
    -> (x, counts, segments, trims, levels, n_streams)"""
    rng = np.random.default_rng(77)

    def voiced(seconds, amp, quiet_front=0, quiet_back=0):
        n = int(seconds * FS)
        t = np.arange(n) / FS
        v = amp * (0.7 * np.sin(2 * np.pi * 180.0 * t) + 0.3 * rng.standard_normal(n))
        v[:quiet_front] *= 1e-3
        v[n - quiet_back:] *= 1e-3
        return v.astype(np.float32)

    rows = [voiced(1.0, 0.25, 1201, 903), voiced(0.6, 0.5), voiced(0.9, 0.1, 777, 0), voiced(1.3, 0.3), voiced(0.7, 0.2),
            voiced(0.3, 0.2)]
    S = max(map(len, rows)) + 7
    x = np.full((6, S), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    segs = [Seg(0, 0, 3, 0, 1.0), Seg(1, 0, 0, 1, 0.8),                 # stream 0: a levelled row, a peak-normalised one
            Seg(2, 1, 0, 0, 1.0), Seg(3, 1, 5, 0, 0.5),                 # stream 1: levelled as a stream
            Seg(4, 2, 0, 0, 1.0), Seg(5, 2, 2, 0, 1.0)]                 # stream 2: a ceiling that binds; a row under 400 ms
    trims = [Trim(2, 0.1, 10, 10, 4), tref.OFF, Trim(1, 0.01, 0, 5, 0), tref.OFF, Trim(0, 0.0, 0, 0, 6), tref.OFF]
    levels = [Level(1, -19.0, 30.0, 0.0), ref.OFF, Level(2, -16.0, 30.0, 0.0), Level(2, -16.0, 30.0, 0.0),
              Level(1, -3.0, 60.0, 0.5), Level(1, -19.0, 30.0, 0.0)]
    return x, np.array([len(r) for r in rows], np.int64), segs, trims, levels, 3


_DELIVERY = {}


def _delivery_case():
    if not _DELIVERY:
        x, counts, segs, trims, levels, J = _delivery_batch()
        _DELIVERY["batch"] = (x, counts, segs, trims, levels, J)
        _DELIVERY["want"] = ref.measure(x, counts, segs, trims, levels, J, FS)
    return _DELIVERY["batch"], _DELIVERY["want"]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_levelled_delivery_end_to_end(encoding):
    from phoonnx_amd.session import test_deliver_leveled, test_deliver_trimmed
    (x, counts, segs, trims, levels, J), (want_l, want_g, want_kept) = _delivery_case()
    got = test_deliver_leveled(x, counts, _segments(segs), _levels(levels), FS, _trims(trims), J, encoding)
    assert [(int(a), int(c)) for a, c in zip(got["kept_first"], got["kept_count"])] == want_kept
    assert want_kept[0][0] > 0 and sum(want_kept[0]) < counts[0] and want_kept[2][0] > 0        # the trims cut
    loud, gain = got["loudness"], got["gain"]
    # loudness within the meter tolerance; the stream's two segments share one figure; mode 0 reports none
    for g in (0, 2, 3, 4):
        assert abs(loud[g] - want_l[g]) <= 0.1, (g, loud[g], want_l[g])
    assert loud[2] == loud[3] and gain[2] == gain[3] and math.isnan(loud[1]) and gain[1] == 1.0
    # a row under 400 ms: no integrated loudness, gain 1
    assert counts[5] < 0.4 * FS and loud[5] == -math.inf and gain[5] == 1.0 and want_l[5] == -math.inf
    # the bytes: the reference's encoding of the same rows with the gains the device reports
    assert _bytes(got["streams"]) == ref.deliver_ref(x, counts, segs, trims, levels, J, encoding, gain)
    assert got["stream_samples"].tolist() == [len(s) for s in got["streams"]]
    # the gains are the rule applied to what the device measured
    pk = [np.abs(x[s.row, a:a + c]).max() for s, (a, c) in zip(segs, want_kept)]
    for g, peak in ((0, pk[0]), (2, max(pk[2], pk[3])), (4, pk[4])):
        assert gain[g] == ref.gain(loud[g], peak, levels[g]), g
    # the layout only: the same figures, nothing packed
    lay = test_deliver_leveled(x, counts, _segments(segs), _levels(levels), FS, _trims(trims), J, encoding, layout_only=True)
    assert lay["streams"] is None and lay["gain"].tobytes() == gain.tobytes() and np.array_equal(lay["stream_offsets"], got["stream_offsets"])
    # without levels, and with every level off: the trimmed delivery's bytes exactly
    norm = [s._replace(normalize=1 + g % 2) for g, s in enumerate(segs)]
    base = test_deliver_trimmed(x, counts, _segments(norm), _trims(trims), J, encoding)
    for lv in (None, [ref.OFF] * 6, [Level(0, -5.0, 1.0, 0.9)] * 6):
        same = test_deliver_leveled(x, counts, _segments(norm), _levels(lv), FS, _trims(trims), J, encoding)
        assert _bytes(same["streams"]) == _bytes(base["streams"])
        assert np.array_equal(same["stream_offsets"], base["stream_offsets"]) and (same["gain"] == 1.0).all()


def test_a_levelled_row_reads_its_target_and_a_binding_ceiling_holds():
    from phoonnx_amd.session import test_deliver_leveled
    (x, counts, segs, trims, levels, J), (want_l, want_g, want_kept) = _delivery_case()
    got = test_deliver_leveled(x, counts, _segments(segs), _levels(levels), FS, _trims(trims), J, "f32")
    # segment 0: mode 1, neither cap binds, volume 1, nothing clips - what was delivered reads the target
    a, c = want_kept[0]
    out0 = got["streams"][0][3:3 + c]
    assert got["gain"][0] < 10.0 ** (30.0 / 20.0) and np.abs(out0).max() < 1.0
    assert abs(ref.loudness(out0, FS) - -19.0) <= 0.1
    # segment 4: the ceiling binds - the delivered sample peak is the ceiling, within the roundings of the gain (2^-24
    # relative) and of the one product (2^-24 relative)
    peak_in = np.abs(x[4, :counts[4]]).max()
    assert got["gain"][4] == np.float32(float(np.float32(0.5)) / float(peak_in)) and want_g[4] == got["gain"][4]
    out4 = got["streams"][2][:counts[4]]
    assert abs(float(np.abs(out4).max()) - 0.5) <= 0.5 * 2.0 ** -23


def test_refusals_on_the_device_path_leave_the_buffers_alone():
    from phoonnx_amd.session import SessionError, test_deliver_leveled
    (x, counts, segs, trims, levels, J), _ = _delivery_case()
    bad = list(levels)
    bad[3] = Level(2, -14.0, 30.0, 0.0)
    with pytest.raises(SessionError, match="segment 3: stream level"):
        test_deliver_leveled(x, counts, _segments(segs), _levels(bad), FS, _trims(trims), J, "pcm16")
    with pytest.raises(SessionError, match="sample_rate 7000"):
        test_deliver_leveled(x, counts, _segments(segs), _levels(levels), 7000, _trims(trims), J, "pcm16")


# ------------------------------------------------------------------ through a session

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


SEGS = [Seg(2, 0, 11, 0, 0.5), Seg(0, 0, 0, 0, 0.5), Seg(1, 1, 3, 1, 0.9)]
TRIMS = [Trim(2, 0.05, 0, 0, 4), Trim(2, 0.05, 3, 5, 0), tref.OFF]
LEVELS = [Level(2, -20.0, 40.0, 0.9), Level(2, -20.0, 40.0, 0.9), ref.OFF]


@pytest.mark.parametrize("rate", [None, 8000])
def test_levelled_delivery_of_a_run_and_its_reservation(rate):
    from phoonnx_amd.session import SessionError
    s = _session("tiny_rb1", output_rate=rate)
    fs = rate or s.delivered_rate
    ids, lens, scales, sid, seeds, dur = _batch(s)
    s.reserve(3, 40, 40 * 60)
    cap = s.hparam("workspace_bytes")
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=dur)
    x = r["output"][:, 0, 0, :].copy()
    counts = np.asarray(r["sample_lengths"] if rate else r["y_lengths"] * s.hparam("hop"), np.int64)
    assert counts.min() >= 0.8 * fs, "the rows are too short to have blocks"
    want_l, want_g, want_kept = ref.measure(x, counts, SEGS, TRIMS, LEVELS, 2, fs)
    assert np.isfinite(want_l[0])
    for enc in ("ulaw", "f32"):
        got, kf, kc, loud, gain = s.deliver(_segments(SEGS), 2, enc, trims=_trims(TRIMS), levels=_levels(LEVELS), return_kept=True,
                                            return_levels=True)
        assert [(int(a), int(c)) for a, c in zip(kf, kc)] == want_kept
        assert abs(loud[0] - want_l[0]) <= 0.1 and loud[0] == loud[1] and math.isnan(loud[2])
        assert _bytes(got) == ref.deliver_ref(x, counts, SEGS, TRIMS, LEVELS, 2, enc, gain), enc
        assert s.hparam("workspace_bytes") == cap, "a levelled delivery allocated behind a reservation that covers the request"
    # without levels: the trimmed delivery; a rate that is not the delivered one is refused where one is set, and the run stays
    assert _bytes(s.deliver(_segments(SEGS), 2, "alaw", trims=_trims(TRIMS), levels=_levels([ref.OFF] * 3))) == _bytes(
        s.deliver(_segments(SEGS), 2, "alaw", trims=_trims(TRIMS)))
    if rate:
        with pytest.raises(SessionError, match="sample_rate 22050 differs from the output rate 8000"):
            s.deliver(_segments(SEGS), 2, "ulaw", levels=_levels(LEVELS), sample_rate=22050)
    with pytest.raises(SessionError, match="segment 0: normalize 1"):
        s.deliver(_segments([SEGS[0]._replace(normalize=1)] + SEGS[1:]), 2, "ulaw", levels=_levels(LEVELS))
    # run and levelled delivery in one call
    d = s.synthesize_delivered(ids, lens, scales, sid, segments=_segments(SEGS), n_streams=2, encoding="pcm16", seeds=seeds,
                               durations=dur, trim=_trims(TRIMS), levels=_levels(LEVELS))
    assert _bytes(d["streams"]) == ref.deliver_ref(x, counts, SEGS, TRIMS, LEVELS, 2, "pcm16", d["gain"])
    assert abs(d["loudness"][0] - want_l[0]) <= 0.1 and s.hparam("workspace_bytes") == cap
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


def test_synthesize_encoded_levels_on_the_device_as_the_fallback_does():
    from phoonnx_amd.config import SynthesisConfig
    s = _session("tiny_rb2_ms")
    dev, host = _voice(s), _voice(_NoDelivery(s))
    # (a slow voice: the synthetic one renders a few frames per phoneme, and a sentence needs 400 ms to have a loudness)
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, length_scale=20.0, volume=1.0, normalize_audio=False)
    text = "the quick brown fox jumps over the fence and runs away. a lazy dog sleeps in the warm sun all day long"
    for scope in ("sentence", "text"):
        kw = dict(encoding="f32", sentence_silence=0.01, loudness=-19.0, loudness_scope=scope, max_gain_db=60.0)
        d, h = dev.synthesize_encoded(text, cfg, **kw), host.synthesize_encoded(text, cfg, **kw)
        assert d.sentence_starts == h.sentence_starts and d.sentence_samples == h.sentence_samples and len(d.data) == len(h.data)
        assert len(d.loudness) == 2 and all(np.isfinite(d.loudness)), (d.loudness, d.sentence_samples)
        assert np.abs(np.array(d.loudness) - np.array(h.loudness)).max() <= 0.1
        for st, n in zip(d.sentence_starts, d.sentence_samples):          # what was delivered reads the target
            if scope == "sentence" and np.abs(d.data[st:st + n]).max() < 1.0:
                assert abs(ref.loudness(d.data[st:st + n], 22050) - -19.0) <= 0.1
    with pytest.raises(ValueError, match="normalize_audio"):
        dev.synthesize_encoded(text, SynthesisConfig(normalize_audio=True), loudness=-19.0)
    s.close()
