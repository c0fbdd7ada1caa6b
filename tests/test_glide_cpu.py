"""Pitch contours (include/vitsmi.h, "pitch contours") without a GPU: the cutoff function against the warp's token, a row's
plan against tests/glide_ref.py through vits_glide_plan, the properties the definition promises - asserted on the engine's
records -, the refusals on a host-only handle, the figures the header quotes re-measured on the reference, and
TTSVoice's pitch_contour= on a recording session."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import glide_ref as ref
import warp_ref
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")
ONE = ref.ONE

# the figures of the header's parenthesis (measured on glide_ref.figures() / measure_gain())
TONE_ERR, GAIN = 2.1e-5, 1.987

ENDS = (-12, -7, -1, 0, 0.5, 3, 12)


def _lib():
    from phoonnx_amd import _ffi
    return _ffi, _ffi.load()


def _plan(D, st0, st1, hop):
    """vits_glide_plan: (segments as glide_ref.Seg, spans, N) - the counts first, as a caller that sizes its buffers does"""
    _ffi, lib = _lib()
    D = np.ascontiguousarray(D, np.int64)
    st0 = None if st0 is None else np.ascontiguousarray(st0, np.float32)
    st1 = None if st1 is None else np.ascontiguousarray(st1, np.float32)
    n = C.c_int64(-1)
    count = lib.vits_glide_plan(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), len(D), hop, None, None, C.byref(n))
    assert count >= 0, lib.vits_last_error(None)
    segs = (_ffi.VitsGlideSeg * max(count, 1))()
    spans = np.full(len(D), -1, np.int64)
    n2 = C.c_int64(-1)
    assert lib.vits_glide_plan(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), len(D), hop, segs, _ffi.ptr(spans), C.byref(n2)) == count
    assert n2.value == n.value and all(g.pad_[0] == 0 and g.pad_[1] == 0 for g in segs[:count])
    return [ref.Seg(g.n0, g.pos0, g.k, g.step0, g.step1) for g in segs[:count]], spans, n.value


def test_the_entries_are_declared_and_exported():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_run_async_glided", "vits_glide_token", "vits_glide_cutoff", "vits_glide_plan", "vits_test_glide"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsGlideSeg) == 40 == C.sizeof(_ffi.VitsWarpSeg)
    assert "vits_glide_seg" in header and "vits_contour" in header


def test_the_cutoff_equals_the_warps_token_for_every_step():
    _, lib = _lib()
    c, Kh = C.c_int64(), C.c_int32()
    # every integer step against warp_ref.token's formula (double, rint) - vectorised; the engine's function at each
    s = np.arange(ONE // 2, 2 * ONE + 1, dtype=np.int64)
    want_c = np.rint(warp_ref.RHO * np.minimum(1.0, ONE / s.astype(np.float64)) * ONE).astype(np.int64)
    want_Kh = -(-warp_ref.Z * ONE // want_c)
    got = np.empty((len(s), 2), np.int64)
    for i, v in enumerate(s.tolist()):
        assert lib.vits_glide_cutoff(v, C.byref(c), C.byref(Kh)) == 0
        got[i] = c.value, Kh.value
    assert np.array_equal(got[:, 0], want_c) and np.array_equal(got[:, 1], want_Kh)
    assert all(ref.cutoff(v) == tuple(got[v - ONE // 2]) for v in (ONE // 2, ONE - 1, ONE, ONE + 1, 70000, 2 * ONE))
    # ... and against vits_warp_token itself over a fine sweep of semitones: every step it can produce is covered above
    step, wc, wKh = C.c_int64(), C.c_int64(), C.c_int32()
    for st in np.linspace(-12, 12, 4801):
        assert lib.vits_warp_token(float(st), C.byref(step), C.byref(wc), C.byref(wKh)) == 0
        assert ONE // 2 <= step.value <= 2 * ONE
        assert tuple(got[step.value - ONE // 2]) == (wc.value, wKh.value), st
    for bad in (ONE // 2 - 1, 2 * ONE + 1, 0, -5):
        assert lib.vits_glide_cutoff(bad, None, None) != 0
    assert lib.vits_glide_cutoff(ONE, None, None) == 0


def _check_properties(segs, spans, N, D, hop):
    """what "pitch contours" promises of a row's records"""
    assert int(spans.sum()) == N
    pos = 0
    for g in segs:
        assert g.pos0 == pos and g.k <= ref.MAX_SPAN
        lo, hi = min(g.step0, g.step1), max(g.step0, g.step1)
        if g.k:
            p, s = ref.samples(g)
            inc = np.diff(np.concatenate([p, [ref.pos_at(g, g.k)]]))
            assert inc.min() >= lo and inc.max() <= hi, g
            assert s.min() >= lo and s.max() <= hi and s[0] == g.step0, g
        pos = ref.pos_at(g, g.k)
    end = int(np.sum(D)) * hop
    if segs:
        assert abs(pos - (end << ref.FB)) < 2 * ONE, (pos / ONE, end)   # the end of the row: within 2 samples of cum * hop


def test_the_plan_equals_the_reference_and_keeps_its_promises():
    rng = np.random.default_rng(11)
    for hop in (1, 2, 4, 8, 256):
        for rep in range(6):
            T = int(rng.integers(1, 24))
            D = rng.integers(0, 6, T)
            st0 = rng.choice(ENDS, T).astype(np.float32)
            st1 = rng.choice(ENDS, T).astype(np.float32)
            segs, spans, N = _plan(D, st0, st1, hop)
            rsegs, rspans, rN = ref.plan(D, st0, st1, hop)
            assert segs == rsegs and np.array_equal(spans, rspans) and N == rN
            assert len(segs) == int((D > 0).sum()) and not spans[D == 0].any()
            _check_properties(segs, spans, N, D, hop)
    assert _plan([], None, None, 8) == ([], pytest.approx([]), 0)
    # st0 NULL: zeros; st1 NULL: the start values
    a = _plan([2, 3], None, [4, -4], 8)
    assert a[0] == ref.plan([2, 3], [0, 0], [4, -4], 8)[0]
    b = _plan([2, 3], [4, -4], None, 8)
    assert all(g.step0 == g.step1 for g in b[0]) and b[0] == ref.plan([2, 3], [4, -4], [4, -4], 8)[0]


def test_the_carry_cases():
    """P <= pos: at hop 1 a token after a fast one is already passed - k == 0, a record all the same, nothing accumulates"""
    seen = 0
    rng = np.random.default_rng(3)
    for rep in range(40):
        T = 12
        D = rng.integers(0, 3, T)
        st0 = rng.choice([12, 12, 7, -12], T).astype(np.float32)
        st1 = rng.choice([12, 3, -12], T).astype(np.float32)
        segs, spans, N = _plan(D, st0, st1, 1)
        assert (segs, N) == ref.plan(D, st0, st1, 1)[::2]
        seen += sum(1 for g in segs if g.k == 0)
        _check_properties(segs, spans, N, D, 1)
    assert seen >= 5


def test_equal_ends_reproduce_the_warps_plan():
    _ffi, lib = _lib()
    rng = np.random.default_rng(7)
    for hop in (1, 4, 256):
        D = rng.integers(0, 6, 19)
        st = rng.uniform(-12, 12, 19).astype(np.float32)
        segs, spans, N = _plan(D, st, st, hop)
        w = (_ffi.VitsWarpSeg * 19)()
        wspans, wn = np.zeros(19, np.int64), C.c_int64()
        count = lib.vits_warp_plan(_ffi.ptr(np.ascontiguousarray(D, np.int64)), _ffi.ptr(st), 19, hop, w, _ffi.ptr(wspans), C.byref(wn))
        assert count == len(segs) and wn.value == N and np.array_equal(spans, wspans)
        c, Kh = C.c_int64(), C.c_int32()
        for g, q in zip(segs, w[:count]):
            assert (g.n0, g.pos0, g.k, g.step0, g.step1) == (q.n0, q.pos0, q.k, q.step, q.step)
            assert lib.vits_glide_cutoff(g.step0, C.byref(c), C.byref(Kh)) == 0 and (c.value, Kh.value) == (q.c, q.half_taps)


def test_a_tokens_numbers_and_its_rate():
    _, lib = _lib()
    a, b, r = C.c_int64(), C.c_int64(), C.c_float()
    for st0, st1 in ((-12, 12), (12, -12), (-3, 4), (0, 7), (0.5, 0.5), (0, 0)):
        assert lib.vits_glide_token(st0, st1, C.byref(a), C.byref(b), C.byref(r)) == 0
        ra, rb, rr = ref.token(st0, st1)
        assert (a.value, b.value) == (ra, rb) and np.float32(r.value) == rr
        if st0 == st1:
            assert np.float32(r.value) == np.float32(2.0 ** (st0 / 12.0))
    assert lib.vits_glide_token(0, 0, None, None, None) == 0
    for bad in (float("nan"), 12.5, -13.0, float("inf")):
        assert lib.vits_glide_token(bad, 0, None, None, None) != 0 and lib.vits_glide_token(0, bad, None, None, None) != 0


def test_a_token_past_the_span_limit_is_refused():
    _ffi, lib = _lib()
    D, st0, st1 = np.array([1 << 16], np.int64), np.array([-12], np.float32), np.array([-11], np.float32)
    n = C.c_int64()
    assert lib.vits_glide_plan(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), 1, 256, None, None, C.byref(n)) < 0
    assert b"token 0" in lib.vits_last_error(None) and b"gliding token" in lib.vits_last_error(None)
    D[0] = 1 << 13                                                          # 2^21 input samples: fine
    assert lib.vits_glide_plan(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), 1, 256, None, None, C.byref(n)) == 1


@pytest.mark.parametrize("bad", [float("nan"), 12.5, -13.0, float("inf")])
def test_bad_values_are_refused_naming_the_array_row_and_token(bad):
    _ffi, lib = _lib()
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    s = MiSession(PATH, host_only=True)
    ids, lens = np.ones((2, 5), np.int64), np.array([5, 3], np.int64)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    st0, st1 = np.zeros((2, 5), np.float32), np.zeros((2, 5), np.float32)
    st1[1, 2] = bad
    with pytest.raises(SessionError, match=r"token_semitones_end\[1,2\]"):
        s.synthesize_batch(ids, lens, scales, token_semitones=st0, token_semitones_end=st1)
    with pytest.raises(SessionError, match=r"token_semitones_end\[1,2\]"):
        s.synthesize_batch(ids, lens, scales, token_semitones_end=st1)
    rows = np.tile(scales, (2, 1))
    ctl = _ffi.VitsControls(rows.ctypes.data, None, None, None)
    noise = _ffi.VitsNoise()

    def run(a, b):
        con = _ffi.VitsContour(None if a is None else a.ctypes.data, None if b is None else b.ctypes.data, 1)
        rc = s._lib.vits_run_async_glided(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 2, 5, None, C.byref(noise), C.byref(ctl), C.byref(con))
        return rc, s._err()

    rc, err = run(st0, st1)
    assert rc != 0 and "token_semitones_end[1,2]" in err
    rc, err = run(st1, st0)
    assert rc != 0 and "token_semitones[1,2]" in err and "_end" not in err
    rc, err = run(None, st1)
    assert rc != 0 and "token_semitones_end[1,2]" in err
    st1[1, 2] = 0
    st1[1, 4] = bad                                                          # behind lens[1]: ignored - the device is asked for
    rc, err = run(st0, st1)
    assert rc != 0 and "host-only" in err
    s.close()


def test_the_refusals_of_a_glided_run_on_a_host_only_handle():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    s = MiSession(PATH, host_only=True)
    ids, lens = np.ones((1, 4), np.int64), np.array([4], np.int64)
    st0, st1 = np.array([[0, 2, 0, 0]], np.float32), np.array([[0, 4, 1, 0]], np.float32)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    forced = np.full((1, 4), 3)
    with pytest.raises(SessionError, match="forced durations are the rendered ones"):
        s.synthesize_batch(ids, lens, scales, durations=forced, token_semitones=st0, token_semitones_end=st1, compensate=True)
    # the pure glide takes forced durations, and a host-only handle gets as far as the device
    with pytest.raises(SessionError, match="host-only"):
        s.synthesize_batch(ids, lens, scales, durations=forced, token_semitones=st0, token_semitones_end=st1, compensate=False)
    with pytest.raises(SessionError, match="host-only"):
        s.synthesize_delivered(ids, lens, scales, token_semitones_end=st1)
    for setter, arg in ((s.set_output_rate, 8000), (s.set_output_rates, [16000])):
        setter(arg)
        with pytest.raises(SessionError, match="not covered with an output rate set"):
            s.synthesize_batch(ids, lens, scales, token_semitones=st0, token_semitones_end=st1)
        with pytest.raises(SessionError, match="not covered with an output rate set"):
            s.synthesize_batch(ids, lens, scales, token_semitones_end=st0)   # equal ends (zeros -> st0): the warp, refused alike
        setter(None)
    with pytest.raises(SessionError, match="token_semitones_end"):
        s.synthesize_batch(ids, lens, scales, token_semitones_end=np.zeros((1, 3)))
    s.close()


def test_the_pipelined_session_names_the_keyword():
    from phoonnx_amd.session import PipelinedSession, SessionError
    p = PipelinedSession.__new__(PipelinedSession)
    with pytest.raises(SessionError, match="token_semitones_end"):
        p.synthesize_batch(np.ones((1, 2), np.int64), np.array([2], np.int64), np.ones(3, np.float32), token_semitones_end=np.zeros((1, 2)))


def test_the_reference_meets_the_headers_figures():
    tone = ref.figures()
    gain = ref.measure_gain()
    print(f"tone error {tone:.3e}, gain {gain:.4f}")
    assert tone <= 1.25 * TONE_ERR and tone >= 0.75 * TONE_ERR
    assert gain <= ref.GAIN and abs(gain - GAIN) <= 0.25 * GAIN and ref.GAIN - gain < 0.01   # rounded UP to two decimals
    assert gain > warp_ref.GAIN                                                # why this module has a bound of its own
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for v in ("2.1e-5", "1.987", "1.99"):
        assert v in header, v


def test_glide64_on_its_own_terms():
    """the reference: an identity plan copies; equal ends are warp64; the tolerance counts the largest Kh visited"""
    x = np.random.default_rng(2).standard_normal(400)
    segs, _, N = ref.plan([5, 5], [0, 0], [0, 0], 10)
    assert N == 100 and np.array_equal(ref.glide64(x, segs, N), x[:100])
    D, st = [4, 0, 3, 5], [3, 0, -7, 12]
    segs, _, N = ref.plan(D, st, st, 8)
    wsegs, _, wN = warp_ref.plan(D, st, 8)
    assert N == wN and np.allclose(ref.glide64(x, segs, N), warp_ref.warp64(x, wsegs, wN), rtol=0, atol=1e-15)
    assert ref.max_half(ref.plan([5], [-12], [12], 8)[0]) == 38 and ref.max_half(ref.plan([5], [-12], [0], 8)[0]) == 19
    assert ref.tolerance(ref.plan([5], [-12], [12], 8)[0], 1.0) == 80 * 2.0 ** -24 * ref.GAIN


# ------------------------------------------------------------------ the Python surface

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(session, **kw):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    cfg = VoiceConfig(num_symbols=40, num_speakers=1, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={"^": [1], "_": [0], "$": [2], **{c: [3 + i, 30] for i, c in enumerate("abcdefgh ")}},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True, **kw)


class _Recorder:
    """a session that delivers and glides: records the call, returns a warped run's shape of result"""

    def get_inputs(self):
        from phoonnx_amd.session import NodeArg
        return [NodeArg("input", "tensor(int64)", [None, None])]

    def hparam(self, key):
        return {"hop": 4, "n_speakers": 1}[key]

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16",
                             return_durations=False, token_semitones=None, compensate=True, token_semitones_end=None, **more):
        self.st0, self.st1, self.lens = token_semitones, token_semitones_end, lens
        B, T = ids.shape
        spans = np.where(np.arange(T)[None, :] < lens[:, None], 3, 0).astype(np.int64)
        counts = spans.sum(axis=1)
        streams = [np.zeros(int(c), np.int16) for c in counts] if n_streams == B else [np.zeros(int(counts.sum()), np.int16)]
        res = {"streams": streams, "sample_lengths": counts, "y_lengths": lens.copy(),
               "kept_first": np.zeros(B, np.int64), "kept_count": counts}
        if return_durations:
            res["durations"], res["token_spans"] = np.where(spans > 0, 1, 0), spans
        return res

    last_durations = synthesize_batch = None


_expected = ref.contour_ids


def test_pitch_contour_gives_start_and_end_values_per_id():
    from phoonnx_amd.config import SynthesisConfig
    rec = _Recorder()
    v = _voice(rec)
    text = "abc. de"
    sizes = [[len(ids) for _, ids in g] for g in v._sentence_groups(text, SynthesisConfig())]
    assert all(len(s) >= 3 for s in sizes) and any(m > 1 for s in sizes for m in s)

    def check(value_of):
        for b, s in enumerate(sizes):
            st0, st1 = _expected(s, value_of)
            n = sum(s)
            assert np.allclose(rec.st0[b, :n], st0, rtol=0, atol=1e-12) and np.allclose(rec.st1[b, :n], st1, rtol=0, atol=1e-12)
            assert not rec.st0[b, n:].any() and not rec.st1[b, n:].any()
            # continuous: every id starts where the one before it ended, the first at value(0), the last ends at value(1)
            assert np.array_equal(rec.st0[b, 1:n], rec.st1[b, :n - 1])
            assert rec.st0[b, 0] == value_of(0.0) and rec.st1[b, n - 1] == value_of(1.0)

    # a rise
    out = v.synthesize_encoded(text, pitch_contour=[(0, 0), (1, 4)], alignments=True)
    check(lambda x: 4.0 * x)
    # alignments come from the token spans: 3 samples an id here, not durations * hop = 4
    al = out.phoneme_alignments
    assert [[a.num_samples for a in s] for s in al] == [[3 * m for m in s] for s in sizes]
    # a rise-fall, as percent-like fractions
    v.synthesize_encoded(text, pitch_contour=[(0.0, -2.0), (0.5, 6.0), (1.0, 0.0)])
    check(lambda x: -2.0 + 16.0 * x if x <= 0.5 else 6.0 - 12.0 * (x - 0.5))
    # a single point: held on both sides - constant, yet through the glide arrays
    v.synthesize_encoded(text, pitch_contour=[(0.3, 2.5)])
    check(lambda x: 2.5)
    # points that fall inside a group: only the values at the group boundaries count (positions are phoneme counts)
    pts = [(0.1, 0.0), (0.15, 8.0), (0.9, -4.0)]
    v.synthesize_encoded(text, pitch_contour=pts)
    check(lambda x: float(np.interp(x, [p for p, _ in pts], [q for _, q in pts])))
    # a callable: (sentence_index, tokens) -> points
    seen = []

    def contour(k, tokens):
        seen.append((k, len(tokens)))
        return [(0, float(k)), (1, float(k) + 3)]

    v.synthesize_encoded(text, pitch_contour=contour)
    assert seen == [(k, len(s)) for k, s in enumerate(sizes)]
    for b, s in enumerate(sizes):
        st0, st1 = _expected(s, lambda x: b + 3.0 * x)
        assert np.allclose(rec.st0[b, :sum(s)], st0, atol=1e-12) and np.allclose(rec.st1[b, :sum(s)], st1, atol=1e-12)
    # without a contour the end values are not passed at all
    v.synthesize_encoded(text, phoneme_pitch=1.0)
    assert rec.st1 is None and np.all(rec.st0[0, :sum(sizes[0])] == 1.0)


def test_phoneme_pitch_is_added_to_both_ends():
    from phoonnx_amd.config import SynthesisConfig
    rec = _Recorder()
    v = _voice(rec)
    sizes = [[len(ids) for _, ids in g] for g in v._sentence_groups("abc", SynthesisConfig())]
    per = lambda k, tokens: [float(i) for i in range(len(tokens))]  # noqa: E731
    v.synthesize_encoded("abc", pitch_contour=[(0, 0), (1, 4)], phoneme_pitch=per)
    st0, st1 = _expected(sizes[0], lambda x: 4.0 * x)
    add = [float(i) for i, m in enumerate(sizes[0]) for _ in range(m)]
    n = sum(sizes[0])
    assert np.allclose(rec.st0[0, :n], np.add(st0, add), atol=1e-12) and np.allclose(rec.st1[0, :n], np.add(st1, add), atol=1e-12)
    with pytest.raises(ValueError, match=r"sentence 0 is not within \[-12, 12\]"):
        v.synthesize_encoded("abc", pitch_contour=[(0, 0), (1, 10)], phoneme_pitch=3.0)
    res = v.synthesize_requests_encoded([("abc", None), ("de", None)], pitch_contour=[(0, -1), (1, 1)], phoneme_pitch=-3.0,
                                        alignments=True)
    live = np.arange(rec.st0.shape[1])[None, :] < rec.lens[:, None]
    assert len(res) == 2 and rec.st0[live].min() == -4.0 and rec.st1[live].max() == -2.0


def test_pitch_contour_refusals():
    v = _voice(_Recorder())
    with pytest.raises(ValueError, match="pitch_contour.*no warped form"):
        v.stream_encoded("ab", pitch_contour=[(0, 1)])
    for bad, what in (([(0, 13.0)], r"within \[-12, 12\]"), ([(0.5, 0), (0.2, 1)], "non-decreasing"), ([(1.5, 0)], r"within \[0, 1\]"),
                      ([], "no point"), ([(0, float("nan"))], r"within \[-12, 12\]"), (3.0, "sequence of")):
        with pytest.raises(ValueError, match=what):
            v.synthesize_encoded("ab", pitch_contour=bad)

    class Old(_Recorder):
        """a session that warps but does not glide: it has no token_semitones_end"""
        def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16",
                                 return_durations=False, token_semitones=None, compensate=True):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="pitch_contour needs a session that glides"):
        _voice(Old()).synthesize_encoded("ab", pitch_contour=[(0, 1)])
    with pytest.raises(ValueError, match="pitch_contour needs a session that glides"):
        _voice(Old()).synthesize_requests_encoded([("ab", None)], pitch_contour=[(0, 1)])

    class NoDelivery:
        get_inputs, hparam = _Recorder.get_inputs, _Recorder.hparam

    with pytest.raises(ValueError, match="pitch_contour needs a session that glides"):
        _voice(NoDelivery()).synthesize_encoded("ab", pitch_contour=[(0, 1)])

    class Rated(_Recorder):
        def set_output_rate(self, rate, input_rate=None):
            self.rate = rate

    with pytest.raises(ValueError, match="pitch_contour is not covered with an output rate set"):
        _voice(Rated(), output_sample_rate=8000).synthesize_encoded("ab", pitch_contour=[(0, 1)])
    with pytest.raises(ValueError, match="pitch_contour is not covered with an output rate set"):
        v.synthesize_requests_encoded([("ab", None)], pitch_contour=[(0, 1)], output_sample_rates=[8000])


def test_synthesis_config_is_unchanged():
    from phoonnx_amd.config import SynthesisConfig
    names = [f.name for f in dataclasses.fields(SynthesisConfig)]
    assert not any("pitch" in n or "semitone" in n or "contour" in n for n in names)
