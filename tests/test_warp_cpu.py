"""The per-token time warp (include/vitsmi.h, "intonation") without a GPU: a token's numbers and a row's plan against
tests/warp_ref.py through vits_warp_token / vits_warp_plan, the plan's arithmetic, the refusals - on a host-only handle
where they need one -, the figures the header quotes re-measured on the reference, and the Python surface."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import warp_ref as ref
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")

# the figures of the header's parenthesis (measured on warp_ref.figures())
TONE_ERR, INTERP_ERR, ALIAS, GAIN = 1.8e-5, 1.6e-6, 2.2e-5, 1.95


def _lib():
    from phoonnx_amd import _ffi
    return _ffi, _ffi.load()


def _plan(D, st, hop):
    """vits_warp_plan: (segments as warp_ref.Seg, spans, N) - the counts first, as a caller that sizes its buffers does"""
    _ffi, lib = _lib()
    D = np.ascontiguousarray(D, np.int64)
    st = None if st is None else np.ascontiguousarray(st, np.float32)
    n = C.c_int64(-1)
    count = lib.vits_warp_plan(_ffi.ptr(D), _ffi.ptr(st), len(D), hop, None, None, C.byref(n))
    assert count >= 0, lib.vits_last_error(None)
    segs = (_ffi.VitsWarpSeg * max(count, 1))()
    spans = np.full(len(D), -1, np.int64)
    n2 = C.c_int64(-1)
    assert lib.vits_warp_plan(_ffi.ptr(D), _ffi.ptr(st), len(D), hop, segs, _ffi.ptr(spans), C.byref(n2)) == count
    assert n2.value == n.value and all(g.pad_ == 0 for g in segs[:count])
    return [ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in segs[:count]], spans, n.value


def test_the_entries_are_declared_and_exported():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_run_async_warped", "vits_last_token_spans", "vits_warp_token", "vits_warp_plan", "vits_test_warp"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsWarpSeg) == 40


@pytest.mark.parametrize("st", [-12, -7, -0.5, 0, 0.5, 7, 12])
def test_a_tokens_numbers_equal_the_reference(st):
    _, lib = _lib()
    step, c, Kh = C.c_int64(), C.c_int64(), C.c_int32()
    assert lib.vits_warp_token(st, C.byref(step), C.byref(c), C.byref(Kh)) == 0
    assert (step.value, c.value, Kh.value) == ref.token(st)
    if st <= 0:
        assert Kh.value == 19
    if st == 12:
        assert Kh.value == 38 and step.value == 2 * ref.ONE
    assert lib.vits_warp_token(st, None, None, None) == 0


def test_the_plan_equals_the_reference():
    D, st, hop = [3, 0, 5, 2, 7], [0, 4, -5, 12, -12], 8
    segs, spans, N = _plan(D, st, hop)
    rsegs, rspans, rN = ref.plan(D, st, hop)
    assert segs == rsegs and np.array_equal(spans, rspans) and N == rN
    assert N == 198 and [g.n0 for g in segs] == [0, 24, 78, 86]
    assert spans[1] == 0 and len(segs) == 4                                  # the dropped token has no segment


def test_plan_arithmetic():
    rng = np.random.default_rng(5)
    for hop in (1, 4, 256):
        D = rng.integers(0, 9, 23)
        # zero semitones: the native row
        for st in (None, np.zeros(23)):
            segs, spans, N = _plan(D, st, hop)
            assert N == int(D.sum()) * hop and all(g.step == ref.ONE for g in segs)
            assert np.array_equal(spans, D * hop)
        st = rng.uniform(-12, 12, 23).astype(np.float32)
        segs, spans, N = _plan(D, st, hop)
        rsegs, rspans, rN = ref.plan(D, st, hop)
        assert segs == rsegs and np.array_equal(spans, rspans) and N == rN
        assert int(spans.sum()) == N
        r = np.array([ref.token(v)[0] / ref.ONE for v in st])
        assert abs(N - float((D * hop / r).sum())) < 1 + int((D > 0).sum())
        # phase is continuous: every segment starts where the one before it ends
        for a, b in zip(segs, segs[1:]):
            assert b.n0 == a.n0 + a.k and b.pos0 == a.pos0 + a.k * a.step
    assert _plan([], None, 8) == ([], pytest.approx([]), 0)


@pytest.mark.parametrize("bad", [float("nan"), 12.5, -13.0, float("inf")])
def test_bad_semitones_are_refused_naming_row_and_token(bad):
    _ffi, lib = _lib()
    assert lib.vits_warp_token(bad, None, None, None) != 0
    D, st = np.array([2, 2, 2], np.int64), np.array([0, 0, bad], np.float32)
    n = C.c_int64()
    assert lib.vits_warp_plan(_ffi.ptr(D), _ffi.ptr(st), 3, 8, None, None, C.byref(n)) < 0
    assert b"token 2" in lib.vits_last_error(None)
    # through the run entry, on a host-only handle: refused before the device is looked at
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    s = MiSession(PATH, host_only=True)
    ids, lens = np.ones((2, 5), np.int64), np.array([5, 3], np.int64)
    sem = np.zeros((2, 5), np.float32)
    sem[1, 2] = bad
    with pytest.raises(SessionError, match=r"token_semitones\[1,2\]"):
        s.synthesize_batch(ids, lens, np.array([0.667, 1.0, 0.8], np.float32), token_semitones=sem)
    rows = np.tile(np.array([0.667, 1.0, 0.8], np.float32), (2, 1))
    ctl = _ffi.VitsControls(rows.ctypes.data, None, None, None)
    into = _ffi.VitsIntonation(sem.ctypes.data, 1)
    noise = _ffi.VitsNoise()
    rc = s._lib.vits_run_async_warped(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 2, 5, None, C.byref(noise), C.byref(ctl), C.byref(into))
    assert rc != 0 and "token_semitones[1,2]" in s._err()
    sem[1, 2] = 0
    sem[1, 4] = bad                                                          # behind lens[1]: ignored - the device is asked for
    rc = s._lib.vits_run_async_warped(s._h, _ffi.ptr(ids), _ffi.ptr(lens), 2, 5, None, C.byref(noise), C.byref(ctl), C.byref(into))
    assert rc != 0 and "host-only" in s._err()
    s.close()


def test_compensate_with_forced_durations_is_refused_on_a_host_only_handle():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    s = MiSession(PATH, host_only=True)
    ids, lens = np.ones((1, 4), np.int64), np.array([4], np.int64)
    sem = np.array([[0, 2, 0, 0]], np.float32)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    with pytest.raises(SessionError, match="forced durations are the rendered ones"):
        s.synthesize_batch(ids, lens, scales, durations=np.full((1, 4), 3), token_semitones=sem, compensate=True)
    # the pure warp takes forced durations, and a host-only handle gets as far as the device
    with pytest.raises(SessionError, match="host-only"):
        s.synthesize_batch(ids, lens, scales, durations=np.full((1, 4), 3), token_semitones=sem, compensate=False)
    # an output rate: not covered
    s.set_output_rate(8000)
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, token_semitones=sem)
    s.set_output_rate(None)
    s.set_output_rates([16000])
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, token_semitones=sem)
    s.close()


def test_the_reference_meets_the_headers_figures():
    tone, interp, alias, gain = ref.figures()
    print(f"tone error {tone:.3e}, interpolation {interp:.3e}, alias {alias:.3e}, gain {gain:.4f}")
    assert tone <= 1.25 * TONE_ERR and interp <= 1.25 * INTERP_ERR and alias <= 1.25 * ALIAS
    assert gain <= 1.25 * GAIN and gain <= ref.GAIN                          # the tolerance's 1.98, not trusted: measured
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for v in ("1.8e-5", "1.6e-6", "2.2e-5", "1.95"):
        assert v in header, v


def test_warp64_on_its_own_terms():
    """the reference: an identity plan copies; a +12 token plays every other sample of a slow tone"""
    x = np.random.default_rng(2).standard_normal(100)
    segs, _, N = ref.plan([5, 5], [0, 0], 10)
    assert N == 100 and np.array_equal(ref.warp64(x, segs, N), x)
    m = np.arange(4000, dtype=np.float64)
    segs, _, N = ref.plan([500], [12], 8)
    assert N == 2000
    y = ref.warp64(np.cos(0.05 * m), segs, N)
    assert np.abs(y - np.cos(0.1 * np.arange(N)))[80:-80].max() < 2e-5


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
    """a session that delivers and takes semitones: records the call, returns a warped run's shape of result"""

    def get_inputs(self):
        from phoonnx_amd.session import NodeArg
        return [NodeArg("input", "tensor(int64)", [None, None])]

    def hparam(self, key):
        return {"hop": 4, "n_speakers": 1}[key]

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16",
                             return_durations=False, token_semitones=None, compensate=True, **more):
        self.semitones, self.lens = token_semitones, lens
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


def test_phoneme_pitch_expands_over_id_groups():
    rec = _Recorder()
    v = _voice(rec)
    from phoonnx_amd.config import SynthesisConfig
    groups = v._sentence_groups("ab. c", SynthesisConfig())
    sizes = [[len(ids) for _, ids in g] for g in groups]
    out = v.synthesize_encoded("ab. c", phoneme_pitch=2.0, alignments=True)
    assert rec.semitones.shape == (2, max(sum(s) for s in sizes))
    for b, s in enumerate(sizes):
        assert np.all(rec.semitones[b, :sum(s)] == 2.0) and not rec.semitones[b, sum(s):].any()
    # one value per phoneme: every id of a group, its blanks included, takes the group's value
    per = lambda k, tokens: [float(i) - 1 for i in range(len(tokens))]  # noqa: E731
    v.synthesize_encoded("ab. c", phoneme_pitch=per)
    for b, s in enumerate(sizes):
        want = [float(i) - 1 for i, n in enumerate(s) for _ in range(n)]
        assert rec.semitones[b, :len(want)].tolist() == want
    v.synthesize_encoded("ab. c", phoneme_pitch=[[float(i) for i in range(len(s))] for s in sizes])
    assert rec.semitones[1, :sum(sizes[1])].tolist() == [float(i) for i, n in enumerate(sizes[1]) for _ in range(n)]
    # alignments come from the token spans: 3 samples an id here, not durations * hop = 4
    al = out.phoneme_alignments
    assert [[a.num_samples for a in s] for s in al] == [[3 * n for n in s] for s in sizes]
    assert al[0][-1].start_sample + al[0][-1].num_samples == out.sentence_samples[0]
    with pytest.raises(ValueError, match="2 values for the"):
        v.synthesize_encoded("ab. c", phoneme_pitch=lambda k, tokens: [0.0, 0.0])
    with pytest.raises(ValueError, match=r"within \[-12, 12\]"):
        v.synthesize_encoded("ab. c", phoneme_pitch=12.5)
    res = v.synthesize_requests_encoded([("ab", None), ("c", None)], phoneme_pitch=-3.0, alignments=True)
    assert np.all(rec.semitones[np.arange(rec.semitones.shape[1])[None, :] < rec.lens[:, None]] == -3.0) and len(res) == 2


def test_phoneme_pitch_refusals():
    v = _voice(_Recorder())
    with pytest.raises(ValueError, match="phoneme_pitch.*no warped form"):
        v.stream_encoded("ab", phoneme_pitch=1.0)

    class Old(_Recorder):
        def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16"):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="phoneme_pitch needs a session that warps"):
        _voice(Old()).synthesize_encoded("ab", phoneme_pitch=1.0)

    class NoDelivery:
        get_inputs, hparam = _Recorder.get_inputs, _Recorder.hparam

    with pytest.raises(ValueError, match="phoneme_pitch needs a session that warps"):
        _voice(NoDelivery()).synthesize_requests_encoded([("ab", None)], phoneme_pitch=1.0)

    class Rated(_Recorder):
        def set_output_rate(self, rate, input_rate=None):
            self.rate = rate

    with pytest.raises(ValueError, match="not covered with an output rate set"):
        _voice(Rated(), output_sample_rate=8000).synthesize_encoded("ab", phoneme_pitch=1.0)
    with pytest.raises(ValueError, match="not covered with an output rate set"):
        v.synthesize_requests_encoded([("ab", None)], phoneme_pitch=1.0, output_sample_rates=[8000])


def test_the_pipelined_session_names_the_keywords():
    from phoonnx_amd.session import PipelinedSession, SessionError
    p = PipelinedSession.__new__(PipelinedSession)
    with pytest.raises(SessionError, match="token_semitones.*compensate"):
        p.synthesize_batch(np.ones((1, 2), np.int64), np.array([2], np.int64), np.ones(3, np.float32), token_semitones=np.zeros((1, 2)))


def test_synthesis_config_is_unchanged():
    from phoonnx_amd.config import SynthesisConfig
    names = [f.name for f in dataclasses.fields(SynthesisConfig)]
    assert not any("pitch" in n or "semitone" in n for n in names)
