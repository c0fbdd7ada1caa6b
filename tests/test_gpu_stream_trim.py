"""Trimmed streaming on the GPU (include/vitsmi.h, "trimmed streaming"): the scan and the pack kernels by value through
vits_test_stream_pack_trimmed, then the feature through MiSession and TTSVoice.

Reference: tests/stream_trim_ref.py - f_b and a_b from the rule over the piece list, the rows' bytes composed from shape_ref /
limit_ref / delivery_ref under the equivalent trim.  Every comparison is on bytes, integers or float bits; no tolerance
anywhere."""
import os

import numpy as np
import pytest

import limit_ref as lref
import shape_ref as sref
import stream_pack_ref as pref
import stream_shape_ref as ssref
import stream_trim_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
B, S, THR, COUNTS = ref.B, ref.S, ref.THR, ref.COUNTS
VOLUME = np.array([1.0, 0.5, 3.0, 1.0, 0.5], np.float32)
CEILINGS = (0.7, 0.7, 0.7, 0.7, 0.0)                              # row 4 is not limited
SHAPES = [sref.Shape(300, 500, 1, ((100, 1.0), (900, 0.25), (901, 2.0), (4000, 1.0))), sref.Shape(0, 0, 0, ((0, 2.0), (4096, 0.5))),
          sref.Shape(4, 4, 0, ()), sref.NONE, sref.Shape(64, 64, 0, ())]
X = ref.batch()
# (piece, L, keep_lead) per encoding: the product pieces x L x keep_lead thinned to a latin-square walk - every piece size, every
# L and every keep_lead in every encoding, the pairs rotating with the encoding - and in front, in every encoding, the clamped
# case (keep_lead 2000, L 0, piece 256, f = 1300).  The three edge rows (2: never found, 3: empty, 4: the tile edge) are in X.
PIECES, LOOKAHEADS, LEADS = (7, 256, 1000, 5000), (0, 1, 255, 1024), (0, 100, 2000)


def _cases(e):
    out = [(256, 0, 2000)]
    for i, piece in enumerate(PIECES):
        for j in range(2):
            L = LOOKAHEADS[(i + 2 * j + e) % 4]
            if piece == 7 and L > 7:       # (pieces of 7 under a long look-ahead: thousands of launches that show nothing new)
                L = LOOKAHEADS[(e + j) % 2]
            out.append((piece, L, LEADS[(i + j + e) % 3]))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _session_shapes(shapes):
    from phoonnx_amd.session import Shape
    return [Shape(s.fade_in, s.fade_out, ("linear", "smooth")[s.curve], list(s.points)) for s in shapes]


def _limits(L):
    return [lref.Limit(c, L) if c else None for c in CEILINGS] if L else None


def _session_limit(L):
    from phoonnx_amd.session import Limit
    return [Limit(c, L) if c else None for c in CEILINGS] if L else None


def _onsets(keep_lead, thr=THR, mode=1):
    from phoonnx_amd.session import Onset
    return [Onset(mode, thr, keep_lead)] * B


def _check(got, ranges, start, piece, encoding, L, keep_lead, what, ref_peak=None, onsets=None):
    """chunks, skips and starts of one configuration against the reference"""
    w = ref.WIDTH[encoding]
    pieces = pref.pieces(S, piece)
    want_ranges = ssref.timeline(pieces, S, L)
    assert ranges == want_ranges, (what, ranges[:4], want_ranges[:4])
    fs, a = ref.starts(X, COUNTS, pieces, onsets or [ref.Onset(1, THR, keep_lead)] * B, L, ref_peak)
    assert start.tolist() == a, (what, start, a)
    rows = ref.rows_ref(X, COUNTS, a, encoding, ref_peak, VOLUME, SHAPES, _limits(L))
    live = [(f, n, r) for (f, n), r in zip(pieces, want_ranges) if r[1]]
    assert len(got) == len(live), what
    for c, (first, n, (ef, en)), skip in zip(got, live, ref.skips(a, COUNTS, [r for _, _, r in live])):
        assert c.first_sample == ef and c.data.shape == (B, ssref.pitch_of(en, encoding)), (what, ef)
        assert np.array_equal(c.valid, np.clip(COUNTS - ef, 0, en)), (what, ef)
        assert np.array_equal(c.skip, skip), (what, ef, c.skip, skip)
        for b in range(B):
            raw = c.data[b].tobytes()
            assert raw[:w * int(skip[b])] == ref.SILENCE[encoding] * int(skip[b]), (what, ef, b, "in front of the skip")
            pad = raw[w * int(c.valid[b]):]
            assert pad == ref.SILENCE[encoding] * (len(pad) // w), (what, ef, b)
        seen = np.minimum(COUNTS, first + n)      # the running peak: ALL valid rendered samples, dropped ones included
        peak = np.array([np.max(np.abs(X[b, :int(seen[b])])) if seen[b] else 0 for b in range(B)], np.float32)
        assert np.array_equal(_bits(c.peak), _bits(peak)), (what, ef, c.peak, peak)
    for b in range(B):
        mine = b"".join(c.data[b].tobytes()[w * int(c.skip[b]):w * int(c.valid[b])] for c in got)
        assert sum(int(c.skip[b]) for c in got) == min(a[b], int(COUNTS[b])), (what, b)
        if mine != rows[b]:
            p, q = np.frombuffer(mine, np.uint8), np.frombuffer(rows[b], np.uint8)
            bad = np.flatnonzero(p != q) if p.size == q.size else None
            raise AssertionError(f"{what} row {b}: {len(mine)} / {len(rows[b])} bytes, "
                                 f"{'sizes differ' if bad is None else f'{bad.size} differ, first at {bad[:8] // w}'}")
    return a


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_trimmed_kernels_by_value(encoding):
    from phoonnx_amd.session import test_stream_pack_trimmed
    seen = set()
    for piece, L, keep_lead in _cases(ENCODINGS.index(encoding)):
        got, ranges, start = test_stream_pack_trimmed(X, COUNTS, piece, encoding, volume=VOLUME, shapes=_session_shapes(SHAPES),
                                                      limit=_session_limit(L), onsets=_onsets(keep_lead))
        a = _check(got, ranges, start, piece, encoding, L, keep_lead, f"{encoding}/{piece}/L={L}/lead={keep_lead}")
        seen.add("clamped" if a[0] > max(0, 1300 - keep_lead) else "the delivery's start")
        if any(n == 0 for _, n in ranges):
            seen.add("a piece delivers nothing")
    assert {"clamped", "the delivery's start"} <= seen


def test_the_cases_cover_the_lists():
    """On the case table alone (no GPU work: it guards the thinning)."""
    every = [c for e in range(4) for c in _cases(e)]
    assert {c[0] for c in every} == set(PIECES) and {c[1] for c in every} == set(LOOKAHEADS) and {c[2] for c in every} == set(LEADS)
    for e in range(4):
        assert _cases(e)[0] == (256, 0, 2000)
        assert {c[0] for c in _cases(e)} == set(PIECES) and {c[2] for c in _cases(e)} == set(LEADS)
        assert any(L == 0 for _, L, _ in _cases(e)) and any(L > 0 for _, L, _ in _cases(e))     # both pack kernels


@pytest.mark.parametrize("encoding", ["pcm16", "f32"])
def test_onsets_without_shaping_take_the_shaped_kernel(encoding):
    """neither fades, points nor limiter: the unshaped stream's bytes behind the start, silence in front"""
    from phoonnx_amd.session import test_stream_pack, test_stream_pack_trimmed
    w = ref.WIDTH[encoding]
    plain = test_stream_pack(X, COUNTS, 1000, encoding, volume=VOLUME)
    got, ranges, start = test_stream_pack_trimmed(X, COUNTS, 1000, encoding, volume=VOLUME, onsets=_onsets(100))
    assert ranges == pref.pieces(S, 1000) and start.tolist() == [1200, 0, ref.INT_MAX, ref.INT_MAX, 2000]
    for g, p in zip(got, plain):
        assert np.array_equal(_bits(g.peak), _bits(p.peak)) and np.array_equal(g.valid, p.valid)
        for b in range(B):
            lo, hi = w * int(g.skip[b]), w * int(g.valid[b])
            assert g.data[b].tobytes()[lo:hi] == p.data[b].tobytes()[lo:hi]
            assert g.data[b].tobytes()[:lo] == ref.SILENCE[encoding] * int(g.skip[b])


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_mode_2_is_mode_1_with_the_product(encoding):
    from phoonnx_amd.session import Onset, test_stream_pack_trimmed
    peaks = np.array([0.8, 0.5, 0.3, 1.0, 2.0], np.float32)
    kw = dict(ref_peak=peaks, volume=VOLUME, shapes=_session_shapes(SHAPES), limit=_session_limit(255))
    two, ranges, start2 = test_stream_pack_trimmed(X, COUNTS, 256, encoding, onsets=_onsets(100, 0.25, 2), **kw)
    per_row = [Onset(1, float(np.float32(0.25) * peaks[b]), 100) for b in range(B)]
    one, _, start1 = test_stream_pack_trimmed(X, COUNTS, 256, encoding, onsets=per_row, **kw)
    assert np.array_equal(start1, start2) and 0 < start2[4] < ref.INT_MAX and start2[1] == 0
    for p, q in zip(one, two):
        assert p.data.tobytes() == q.data.tobytes() and np.array_equal(p.skip, q.skip)
    _check(two, ranges, start2, 256, encoding, 255, 100, f"{encoding}/mode 2", ref_peak=peaks, onsets=[ref.Onset(2, 0.25, 100)] * B)


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_onsets_all_off_are_the_shaped_stream(encoding):
    from phoonnx_amd.session import Onset, test_stream_pack_shaped, test_stream_pack_trimmed
    for L, piece in ((0, 1000), (255, 256)):
        kw = dict(volume=VOLUME, shapes=_session_shapes(SHAPES), limit=_session_limit(L))
        shaped, ranges = test_stream_pack_shaped(X, COUNTS, piece, encoding, **kw)
        for onsets in (None, Onset(0, 0.5, 7)):
            got, mine, start = test_stream_pack_trimmed(X, COUNTS, piece, encoding, onsets=onsets, **kw)
            assert mine == ranges and not start.any() and len(got) == len(shaped)
            for g, p in zip(got, shaped):
                assert g.data.tobytes() == p.data.tobytes() and not g.skip.any()
                assert np.array_equal(g.valid, p.valid) and np.array_equal(_bits(g.peak), _bits(p.peak))


def test_two_runs_give_the_same_bytes():
    from phoonnx_amd.session import test_stream_pack_trimmed
    runs = [test_stream_pack_trimmed(X, COUNTS, 256, "ulaw", volume=VOLUME, shapes=_session_shapes(SHAPES), limit=_session_limit(255),
                                     onsets=_onsets(2000)) for _ in range(2)]
    assert runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])
    for p, q in zip(runs[0][0], runs[1][0]):
        assert p.data.tobytes() == q.data.tobytes() and np.array_equal(_bits(p.peak), _bits(q.peak)) and np.array_equal(p.skip, q.skip)


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


VOL3 = np.array([1.0, 0.5, 2.5], np.float32)
LOOK = 110


def _shaping():
    from phoonnx_amd.session import Limit, Shape
    shapes = [Shape(100, 200, "smooth"), Shape(0, 150, "linear", [(0, 1.5), (800, 0.5)]), Shape(50, 50)]
    return shapes, [Limit(0.5, LOOK), None, Limit(0.3, LOOK)]


def _kept_rows(chunks, n_rows=3):
    return [b"".join(c.data[b, int(c.skip[b]):int(c.valid[b])].tobytes() for c in chunks) for b in range(n_rows)]


def _threshold(x, counts):
    """a threshold from the run's own waveform: above everything in the first eighth of the longest row, so that its onset
    lies behind sample 0 - and below its peak, so that it has one"""
    b = int(np.argmax(counts))
    lead = np.abs(x[b, :int(counts[b]) // 8]).max()
    assert lead < np.abs(x[b, :int(counts[b])]).max()
    return float(lead)


def _starts(chunks, counts):
    """(f is not reported) a_b of every row from the skips: their sum, where the row has an onset"""
    return [sum(int(c.skip[b]) for c in chunks) for b in range(len(counts))]


@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("chunk_frames", [1, 64])
@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_trimmed_stream_of_a_run(preset, chunk_frames, rate):
    from phoonnx_amd.session import Onset, Trim
    s = _session(preset, output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    shapes, limits = _shaping()
    enc = ENCODINGS[(chunk_frames + (rate is not None)) % 4]
    kw = dict(encoding=enc, volume=VOL3, seeds=seeds)
    x = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)["output"][:, 0, 0, :]
    counts = np.asarray(s.last_sample_counts(), np.int64)
    thr = _threshold(x, counts)
    fs = [ref.first_active(x[b], counts[b], thr) for b in range(3)]
    assert any(f is not None and f > 0 for f in fs), fs
    for keep_lead in (0, LOOK):        # (keep_lead <= lookahead: a_b is the delivery's, whatever chunk_frames is)
        plain = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shapes, limit=limits, **kw))
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, shapes=shapes, limit=limits,
                                                  onsets=Onset(1, thr, keep_lead), **kw))
        assert [(c.first_sample, c.data.shape, c.valid.tolist(), _bits(c.peak).tolist()) for c in chunks] == \
               [(c.first_sample, c.data.shape, c.valid.tolist(), _bits(c.peak).tolist()) for c in plain]
        a = [min(max(f - keep_lead, 0), int(n)) if f is not None else int(n) for f, n in zip(fs, counts)]
        assert _starts(chunks, counts) == a, (preset, chunk_frames, rate, keep_lead)
        for c in chunks:
            for b in range(3):
                assert c.data[b, :int(c.skip[b])].tobytes() == ref.SILENCE[enc] * int(c.skip[b])
        trims = [Trim(1, thr, keep_lead, int(counts[b]), 0) for b in range(3)]
        want = s.synthesize_delivered(ids, lens, scales, sid, normalize=False, shapes=shapes, limits=limits, trim=trims, **kw)
        assert _kept_rows(chunks) == [np.ascontiguousarray(r).tobytes() for r in want["streams"]], (preset, chunk_frames, rate, keep_lead)
        assert [int(k) for k, f in zip(want["kept_first"], fs) if f is not None] == [v for v, f in zip(a, fs) if f is not None]
    s.close()


def test_vocoder_stream_trimmed():
    from phoonnx_amd.session import Limit, Onset, Segment, Shape, Trim
    s = _session("tiny_rb1")
    F = 23
    z = np.random.default_rng(5).standard_normal((2, s.hparam("inter"), F)).astype(np.float32)
    vol = np.array([0.5, 2.5], np.float32)
    shapes, limit = [Shape(40, 90, "smooth"), Shape(0, 0, "linear", [(10, 0.5), (500, 2.0)])], [Limit(0.2, 37), None]
    for rate in (None, 8000):
        s.set_output_rate(rate)
        x = s.vocoder(z)[:, 0, 0, :]
        n = x.shape[1]
        thr = _threshold(x, np.array([n, n]))
        fs = [ref.first_active(x[b], n, thr) for b in range(2)]
        assert any(f for f in fs)
        trims = [Trim(1, thr, 30, n, 0)] * 2
        want = s.deliver([Segment(b, b, 0, 0, float(vol[b])) for b in range(2)], 2, "f32", shapes=shapes, limits=limit, trims=trims)
        for chunk_frames in (37, 4):
            chunks = list(s.vocoder_stream_encoded(z, chunk_frames=chunk_frames, encoding="f32", volume=vol, shapes=shapes, limit=limit,
                                                   onsets=Onset(1, thr, 30)))
            assert _kept_rows(chunks, 2) == [np.ascontiguousarray(r).tobytes() for r in want], (rate, chunk_frames)
    s.close()


def test_refusals_up_front_leave_the_previous_run():
    import ctypes as C
    from phoonnx_amd import _ffi
    from phoonnx_amd.session import Onset, RawOnset, Segment, SessionError
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds = _batch(s)
    s.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
    segs = [Segment(b, b, 0, 1, float(VOL3[b])) for b in range(3)]
    before = [np.ascontiguousarray(a).tobytes() for a in s.deliver(segs, 3, "ulaw")]
    for onsets, more, word in ((Onset(3, 0.1, 0), {}, "row 0: onset mode 3"), ([None, Onset(1, -1.0, 0), None], {}, "row 1: onset threshold -1"),
                               (Onset(1, 0.1, -5), {}, "row 0: onset keep_lead -5"), (RawOnset(1, 0.1, 0, 4), {}, "row 0: onset reserved 4"),
                               ([None, None, Onset(2, 0.1, 0)], {}, "row 2: onset mode 2 needs ref_peak")):
        with pytest.raises(SessionError, match=word):
            s.synthesize_stream_encoded(ids, lens, scales, sid, seeds=seeds, onsets=onsets, **more)
    calls = []

    @_ffi.ENC_CHUNK_TRIM_FN
    def cb(*args):
        calls.append(args)
        return 0

    rows = np.ascontiguousarray(scales)
    ctl = _ffi.VitsControls()
    ctl.scales_rows, ctl.seeds = rows.ctypes.data, seeds.ctypes.data
    noise, fmt = _ffi.VitsNoise(), _ffi.VitsStreamFormat()
    bad = (_ffi.VitsStreamOnset * 3)()
    bad[1].mode, bad[1].threshold = 2, 0.5
    rc = s._lib.vits_run_chunked_enc_trimmed(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 3, 40, _ffi.ptr(sid), C.byref(noise), C.byref(ctl),
                                             C.byref(fmt), None, bad, 4, cb, None)
    assert rc == -3 and "row 1: onset mode 2 needs ref_peak" in s._err() and calls == []
    z = np.zeros((3, s.hparam("inter"), 8), np.float32)
    rc = s._lib.vits_run_vocoder_chunked_enc_trimmed(s._h, _ffi.ptr(z), 3, 8, None, C.byref(fmt), None, bad, 4, cb, None)
    assert rc == -3 and "row 1: onset mode 2" in s._err() and calls == []
    assert [np.ascontiguousarray(a).tobytes() for a in s.deliver(segs, 3, "ulaw")] == before
    s.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_a_reservation_covers_the_trimmed_stream(rate):
    from phoonnx_amd.session import Limit, Onset, Shape
    s = _session("tiny_rb1", output_rate=rate)
    ids, lens, scales, sid, seeds = _batch(s)
    dur = np.where(np.arange(40)[None, :] < lens[:, None], 120, 0).astype(np.int64)
    F = 40 * 120
    s.reserve(3, 40, F)
    cap = s.hparam("workspace_bytes")
    for enc, chunk_frames, limit in (("f32", F, Limit(0.5, 1024)), ("pcm16", 1024, None), ("ulaw", 64, Limit(0.5, 1024))):
        chunks = list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=chunk_frames, encoding=enc, volume=VOL3,
                                                  seeds=seeds, durations=dur, shapes=Shape(100, 100), limit=limit, onsets=Onset(1, 0.01, 64)))
        assert s.hparam("workspace_bytes") == cap, (enc, "a trimmed stream allocated behind a reservation that covers the request")
        assert sum(c.data.shape[1] for c in chunks) == chunks[0].total_samples and all(c.skip is not None for c in chunks)
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
def test_voice_stream_encoded_trims_like_synthesize_encoded(encoding):
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.session import Onset, Trim
    voice = _voice("tiny_rb2_ms")
    s = voice.session
    cfg = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=True)
    # ref_peak: the final peaks of an untrimmed stream of the same audio
    from phoonnx_amd.sharding import pad_batch
    ids, lens = pad_batch(voice._sentence_ids(TEXT, cfg))
    sid = np.full((len(lens),), 1, np.int64)
    last = list(s.synthesize_stream_encoded(ids, lens, voice._scales(cfg), sid, chunk_frames=64, encoding=encoding))[-1]
    peaks = last.peak
    kw = dict(fade_in=0.005, fade_out=0.01, limit_ceiling=0.5, limit_lookahead=0.004)
    plain = voice.synthesize_encoded(TEXT, cfg, encoding=encoding, **kw)
    # a float: mode 2 against ref_peak; an Onset: keep_lead in seconds, within the look-ahead
    thr1 = float(np.float32(0.3) * peaks.min())
    trimmed = 0
    for trim, want_trim, silence, chunk_frames in ((0.3, Trim(2, 0.3, 0.0, 3600.0), 0.0, 64), (Onset(2, 0.3, 0.003), Trim(2, 0.3, 0.003, 3600.0), 0.05, 3),
                                                   (Onset(1, thr1, 0.0), Trim(1, thr1, 0.0, 3600.0), 0.0, 1)):
        want = voice.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=silence, trim_silence=want_trim, **kw)
        trimmed += sum(want.sentence_samples) < sum(plain.sentence_samples)
        got = list(voice.stream_encoded(TEXT, cfg, encoding=encoding, chunk_frames=chunk_frames, sentence_silence=silence, ref_peak=peaks,
                                        trim_silence=trim, **kw))
        assert b"".join(got) == want.tobytes(), (trim, chunk_frames)
    assert trimmed, "no case trimmed anything"
    off = SynthesisConfig(speaker_id=1, noise_scale=0.0, noise_w_scale=0.0, volume=0.8, normalize_audio=False)
    for c, more in ((off, {}), (cfg, {})):
        with pytest.raises(ValueError, match=r"Onset\(1, "):
            voice.stream_encoded(TEXT, c, encoding=encoding, trim_silence=0.3, **more)
    s.close()
