"""Fitted durations (include/vitsmi.h, "fitted durations") without a GPU: vits_fit_plan against tests/fit_ref.py - every
comparison exact, the definition is integers and IEEE double -, the identity and the invariants of the definition, the
refusals with their messages - on a host-only handle where they need one -, the ABI surface and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fit_ref as ref
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")
SCALES = np.array([0.667, 1.0, 0.8], np.float32)


def _lib():
    from phoonnx_amd import _ffi
    return _ffi, _ffi.load()


def _plan(w, lens, groups, targets, modes):
    from phoonnx_amd.session import Fit, fit_plan
    return fit_plan(w, lens, Fit(groups, targets, modes))


def _same(got, want):
    """durations, the BITS of s*, frames and status"""
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (got[1], want[1])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (got[2:], want[2:])


def _free(w, lens, rows):
    """the free run's count over `rows`: sum of ceil(cleaned w)"""
    return int(sum(np.ceil(ref.clean(w[b, :lens[b]]).astype(np.float64)).sum() for b in rows))


def _weights(rng, B, T):
    return np.exp(rng.normal(1.0, 1.0, (B, T))).astype(np.float32)


def test_the_entries_are_declared_and_exported():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_fit_plan", "vits_run_async_fitted", "vits_run_chunked_fitted", "vits_run_chunked_enc_fitted", "vits_last_fit",
                 "vits_test_fit_durations"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsFit) == 32
    for name, value in (("VITS_FIT_MET", 0), ("VITS_FIT_FLOOR", 1), ("VITS_FIT_CEIL", 2), ("VITS_FIT_KEPT", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), header) and getattr(_ffi, name) == value
        assert getattr(ref, name[9:]) == value
    assert "fitted durations" in header


@pytest.mark.parametrize("seed", range(6))
def test_random_rows_equal_the_reference(seed):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 400))
    w = _weights(rng, 1, T)
    lens = np.array([T if seed % 2 else int(rng.integers(1, T + 1))], np.int64)
    free = _free(w, lens, [0])
    for F in (free, max(1, int(free * 0.5)), int(free * 1.7), max(1, free - 1), free + 1):
        for mode in (1, 2):
            got = _plan(w, lens, [0], [F], [mode])
            _same(got, ref.fit(w, lens, [0], [F], [mode]))


def test_ties_take_the_extra_frames_in_token_order():
    T, F = 37, 100                                                           # F is no multiple of T
    w = np.full((1, T), 1.3, np.float32)
    got = _plan(w, [T], [0], [F], [1])
    _same(got, ref.fit(w, [T], [0], [F], [1]))
    d = got[0][0]
    assert got[3][0] == ref.MET and d.sum() == F and set(d.tolist()) == {2, 3}
    assert np.array_equal(d, np.sort(d)[::-1]) and (d == 3).sum() == F - 2 * T  # the first R tokens, and only they


def test_cleaned_values_zeros_nan_inf_and_large_weights():
    w = np.array([[0.0, -1.5, np.nan, np.inf, -np.inf, 2.0 ** 25, 2.0 ** 24, 3.7, 1e-30, 0.4]], np.float32)
    assert ref.clean(w)[0].tolist()[:7] == [0, 0, 0, 0, 0, 2.0 ** 24, 2.0 ** 24]
    for F, mode in ((2 ** 22, 1), (2 ** 24, 1), (9, 1), (2 ** 24, 2)):
        got = _plan(w, [10], [0], [F], [mode])
        _same(got, ref.fit(w, [10], [0], [F], [mode]))
        assert not got[0][0, :5].any()                                       # what counts as 0 takes no frame at any s
    z = np.zeros((1, 4), np.float32)                                         # nothing to scale: count is 0 everywhere
    got = _plan(z, [4], [0], [5], [1])
    assert got[3][0] == ref.CEIL and got[1][0] == 16.0 and got[2][0] == 0 and not got[0].any()


def test_groups_of_several_rows_with_their_own_lens():
    rng = np.random.default_rng(11)
    B, T = 5, 70
    w = _weights(rng, B, T)
    lens = np.array([70, 13, 41, 0, 7], np.int64)
    groups = [0, 1, -1, 0, 2]                                                # row 3 has no tokens, row 2 is not fitted
    targets = [int(_free(w, lens, [0, 3]) * 0.8), int(_free(w, lens, [1]) * 1.25), _free(w, lens, [4])]
    got = _plan(w, lens, groups, targets, [1, 1, 2])
    want = ref.fit(w, lens, groups, targets, [1, 1, 2])
    _same(got, want)
    assert (got[0][2] == -1).all()                                           # the canary of a row of no group
    assert not got[0][3].any() and got[0][0].sum() == targets[0]
    assert got[3].tolist() == [ref.MET, ref.MET, ref.KEPT]
    # one group over rows of different lens: one s for all of them
    got = _plan(w, lens, [0] * B, [900], [1])
    _same(got, ref.fit(w, lens, [0] * B, [900], [1]))
    assert got[0].sum() == 900


def test_both_clamps_and_both_branches_of_mode_2():
    rng = np.random.default_rng(3)
    w = _weights(rng, 1, 50)
    free = _free(w, [50], [0])
    lo = int(ref.terms(ref.clean(w[0]), 2.0 ** -4).sum())
    hi = int(ref.terms(ref.clean(w[0]), 16.0).sum())
    for F, mode, status, scale in ((lo - 1, 1, ref.FLOOR, 2.0 ** -4), (hi + 5, 1, ref.CEIL, 16.0), (hi, 1, ref.MET, 16.0),
                                   (lo, 1, ref.MET, None), (free + 10, 2, ref.KEPT, 1.0), (free, 2, ref.KEPT, 1.0),
                                   (free - 10, 2, ref.MET, None), (lo - 1, 2, ref.FLOOR, 2.0 ** -4)):
        got = _plan(w, [50], [0], [F], [mode])
        _same(got, ref.fit(w, [50], [0], [F], [mode]))
        assert got[3][0] == status and (scale is None or got[1][0] == scale), (F, mode, got[1:])
        if status == ref.KEPT:
            assert np.array_equal(got[0][0], np.ceil(w[0].astype(np.float64)).astype(np.int64)) and got[2][0] == free
        if status == ref.FLOOR:
            assert got[2][0] == lo > F
        if status == ref.CEIL:
            assert got[2][0] == hi < F


@pytest.mark.parametrize("seed", range(4))
def test_the_identity_and_the_invariants(seed):
    rng = np.random.default_rng(100 + seed)
    B, T = int(rng.integers(1, 4)), int(rng.integers(1, 300))
    w = _weights(rng, B, T)
    w[rng.random((B, T)) < 0.1] = 0.0
    w[0, : min(T, 6)] = 2.5                                                  # ties
    lens = rng.integers(0, T + 1, B)
    lens[0] = T
    rows = list(range(B))
    free = _free(w, lens, rows)
    # a target equal to the free run's own count reproduces the free run's durations token for token
    d, s, frames, status = _plan(w, lens, [0] * B, [free], [1])
    assert status[0] == ref.MET and s[0] >= 1.0 and frames[0] == free
    for b in rows:
        assert np.array_equal(d[b, :lens[b]], np.ceil(ref.clean(w[b, :lens[b]]).astype(np.float64)).astype(np.int64))
        assert not d[b, lens[b]:].any()
    # every fitted duration is ceil(w s*) or one more; the sum is the target when the status is MET
    for F in (max(1, free // 3), free * 2 + 1):
        d, s, frames, status = _plan(w, lens, [0] * B, [F], [1])
        for b in rows:
            base = ref.terms(ref.clean(w[b, :lens[b]]), s[0])
            assert ((d[b, :lens[b]] == base) | (d[b, :lens[b]] == base + 1)).all()
        if status[0] == ref.MET:
            assert d.sum() == F == frames[0]
        assert 2.0 ** -4 <= s[0] <= 16.0


def _raw_plan(B, T, groups, n_groups, targets, modes, lens=None, w=True, dur=True):
    """vits_fit_plan with whatever the case passes: (rc, message, the outputs - canaries where nothing was written)"""
    _ffi, lib = _lib()
    wa = np.ones((B, T), np.float32)
    la = np.full(B, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    g = None if groups is None else np.asarray(groups, np.int32)
    t = None if targets is None else np.asarray(targets, np.int64)
    m = None if modes is None else np.asarray(modes, np.int32)
    fit = _ffi.VitsFit(_ffi.ptr(g), n_groups, _ffi.ptr(t), _ffi.ptr(m))
    d = np.full((B, T), -7, np.int64)
    sc, fr, st = np.full(4, -7.0), np.full(4, -7, np.int64), np.full(4, -7, np.int32)
    rc = lib.vits_fit_plan(_ffi.ptr(wa) if w else None, _ffi.ptr(la), B, T, C.byref(fit), _ffi.ptr(d) if dur else None, _ffi.ptr(sc),
                           _ffi.ptr(fr), _ffi.ptr(st))
    return rc, _ffi.last_error(None), (d, sc, fr, st)


@pytest.mark.parametrize("case, message", [
    (dict(groups=[0, 0], n_groups=1, targets=[0], modes=[1]), r"fit target_frames\[0\]=0 outside \[1,16777216\]"),
    (dict(groups=[0, 0], n_groups=1, targets=[(1 << 24) + 1], modes=[1]), r"fit target_frames\[0\]=16777217 outside \[1,16777216\]"),
    (dict(groups=[0, 1], n_groups=2, targets=[5, -3], modes=[1, 1]), r"fit target_frames\[1\]=-3 outside"),
    (dict(groups=[0, 0], n_groups=1, targets=[5], modes=[3]), r"fit mode\[0\]=3 is neither 1 \(exact\) nor 2 \(at most\)"),
    (dict(groups=[0, 0], n_groups=1, targets=[5], modes=[0]), r"fit mode\[0\]=0 is neither"),
    (dict(groups=[0, 2], n_groups=2, targets=[5, 5], modes=[1, 1]), r"fit group\[1\]=2 outside \[-1,2\)"),
    (dict(groups=[-2, 0], n_groups=1, targets=[5], modes=[1]), r"fit group\[0\]=-2 outside \[-1,1\)"),
    (dict(groups=[0, 0], n_groups=2, targets=[5, 5], modes=[1, 1]), r"fit group 1 has no rows"),
    (dict(groups=[-1, -1], n_groups=1, targets=[5], modes=[1]), r"fit group 0 has no rows"),
    (dict(groups=[0, 0], n_groups=-1, targets=[5], modes=[1]), r"fit n_groups = -1 is negative"),
    (dict(groups=None, n_groups=1, targets=[5], modes=[1]), r"needs group, target_frames and mode"),
    (dict(groups=[0, 0], n_groups=1, targets=[5], modes=[1], lens=[2, 9]), r"input_lengths\[1\]=9 outside \[0,3\]"),
    (dict(groups=[0, 0], n_groups=1, targets=[5], modes=[1], w=False), r"null pointer"),
    (dict(groups=[0, 0], n_groups=1, targets=[5], modes=[1], dur=False), r"null pointer"),
])
def test_the_plan_refuses_and_writes_nothing(case, message):
    rc, err, outs = _raw_plan(2, 3, **case)
    assert rc < 0 and re.search(message, err), err
    for a in outs:
        assert (a == -7).all()


def test_the_run_entries_refuse_on_a_host_only_handle_before_the_device_is_looked_at():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import Fit, SessionError
    _ffi, _ = _lib()
    s = MiSession(PATH, host_only=True)
    hop = s.hparam("hop")
    ids, lens = np.ones((2, 5), np.int64), np.array([5, 3], np.int64)
    rows = np.tile(SCALES, (2, 1))
    noise = _ffi.VitsNoise()

    def raw(entry, group, G, target, mode, durations=None):
        g, t, m = np.asarray(group, np.int32), np.asarray(target, np.int64), np.asarray(mode, np.int32)
        ctl = _ffi.VitsControls(rows.ctypes.data, None, None if durations is None else durations.ctypes.data, None)
        fit = _ffi.VitsFit(g.ctypes.data, G, t.ctypes.data, m.ctypes.data)
        head = (s._h, _ffi.ptr(ids), _ffi.ptr(lens), 2, 5, None, C.byref(noise), C.byref(ctl))
        if entry == "async":
            rc = s._lib.vits_run_async_fitted(*head, C.byref(fit))
        elif entry == "chunked":
            rc = s._lib.vits_run_chunked_fitted(*head, C.byref(fit), 8, _ffi.CHUNK_FN(lambda *a: 0), None)
        else:
            fmt = _ffi.VitsStreamFormat(0, None, None)
            rc = s._lib.vits_run_chunked_enc_fitted(*head, C.byref(fmt), None, None, C.byref(fit), 8, _ffi.ENC_CHUNK_TRIM_FN(lambda *a: 0), None)
        return rc, s._err()

    limit = min(1 << 24, (2 ** 31 - 1) // hop)
    for entry in ("async", "chunked", "enc"):
        rc, err = raw(entry, [0, 0], 1, [limit + 1], [1])
        assert rc != 0 and f"fit target_frames[0]={limit + 1} outside [1,{limit}]" in err, err
        rc, err = raw(entry, [0, 1], 1, [9], [1])
        assert rc != 0 and "fit group[1]=1 outside [-1,1)" in err, err
        rc, err = raw(entry, [0, 0], 1, [9], [5])
        assert rc != 0 and "fit mode[0]=5" in err, err
        rc, err = raw(entry, [0, -1], 2, [9, 9], [1, 1])
        assert rc != 0 and "fit group 1 has no rows" in err, err
        rc, err = raw(entry, [0, 0], 1, [9], [1], durations=np.full((2, 5), 2, np.int64))
        assert rc != 0 and "durations and a fit are contradictory" in err, err
        rc, err = raw(entry, [0, 0], 1, [9], [1])                               # a good fit: the device is asked for
        assert rc != 0 and "host-only" in err, err
        rc, err = raw(entry, [-1, -1], 0, [9], [1])                             # no row in any group: the entry without a fit
        assert rc != 0 and "host-only" in err, err
    # nothing to report
    assert s._lib.vits_last_fit(s._h, None, None, None, 0) < 0 and "not fitted" in s._err()
    with pytest.raises(SessionError, match="not fitted"):
        s.last_fit()
    # the Python entries raise the same, by the call itself
    fit = Fit([0, 0], [9])
    with pytest.raises(SessionError, match="host-only"):
        s.synthesize_batch(ids, lens, SCALES, fit=fit)
    for call in (lambda **kw: s.synthesize_batch(ids, lens, SCALES, **kw),
                 lambda **kw: s.synthesize_delivered(ids, lens, SCALES, **kw),
                 lambda **kw: s.synthesize_stream(ids, lens, SCALES, **kw),
                 lambda **kw: s.synthesize_stream_encoded(ids, lens, SCALES, **kw)):
        with pytest.raises(ValueError, match="fit= and durations= are contradictory"):
            call(fit=fit, durations=np.full((2, 5), 2))
        with pytest.raises(ValueError, match="fit= together with token_semitones="):
            call(fit=fit, token_semitones=np.zeros((2, 5), np.float32))
        with pytest.raises(ValueError, match="fit= together with token_semitones="):
            call(fit=fit, token_semitones_end=np.zeros((2, 5), np.float32))
        with pytest.raises(SessionError, match=rf"fit target_frames\[0\]={limit + 1} outside \[1,{limit}\]"):
            call(fit=Fit([0, 0], [limit + 1]))
        with pytest.raises(SessionError, match=r"fit target_frames\[0\]=0 outside"):
            call(fit=Fit([0, 0], [0]))
        with pytest.raises(SessionError, match=r"fit group\[1\]=3 outside \[-1,1\)"):
            call(fit=Fit([0, 3], [9]))
        with pytest.raises(SessionError, match=r"fit mode\[0\]='loose' is neither"):
            call(fit=Fit([0, 0], [9], "loose"))
        with pytest.raises(SessionError, match="fit group 1 has no rows"):
            call(fit=Fit([0, 0], [9, 9]))
        with pytest.raises(SessionError, match=r"Invalid shape for 'fit.groups'"):
            call(fit=Fit([0, 0, 0], [9]))
        with pytest.raises(SessionError, match="must be a session.Fit"):
            call(fit=([0, 0], [9]))
    s.close()


def test_fit_modes_by_name():
    from phoonnx_amd.session import Fit
    assert Fit([0], [5]).modes.tolist() == [1] and Fit([0], [5], "at_most").modes.tolist() == [2]
    assert Fit([0, 1], [5, 6], ["exact", 2]).modes.tolist() == [1, 2]
    f = Fit.one_group(3, 40, "at_most")
    assert f.groups.tolist() == [0, 0, 0] and f.target_frames.tolist() == [40] and f.modes.tolist() == [2]


def test_the_pipelined_session_names_the_keyword():
    from phoonnx_amd.session import Fit, PipelinedSession, SessionError
    p = PipelinedSession.__new__(PipelinedSession)
    with pytest.raises(SessionError, match="'fit' is not covered by PipelinedSession"):
        p.synthesize_batch(np.ones((1, 2), np.int64), np.array([2], np.int64), np.ones(3, np.float32), fit=Fit([0], [5]))


# ------------------------------------------------------------------ TTSVoice: the target arithmetic, on stub sessions

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(session, rate=22050, **kw):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    cfg = VoiceConfig(num_symbols=40, num_speakers=1, num_langs=1, sample_rate=rate, lang_code="en",
                      phoneme_id_map={"^": [1], "_": [0], "$": [2], **{c: [3 + i, 30] for i, c in enumerate("abcdefgh ")}},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True, **kw)


class _Fitting:
    """a session whose entries take fit=: records it and answers with the shape of a fitted run"""
    HOP = 256

    def get_inputs(self):
        from phoonnx_amd.session import NodeArg
        return [NodeArg("input", "tensor(int64)", [None, None])]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": 1}[key]

    def set_output_rate(self, rate, input_rate=None):
        self.rate = rate

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16",
                             return_durations=False, fit=None, **more):
        self.fit, self.B = fit, ids.shape[0]
        counts = np.full(self.B, 10, np.int64)
        lead = sum(int(g.lead_samples) for g in segments)
        return {"streams": [np.zeros(int(counts.sum()) + lead, np.int16)], "sample_lengths": counts, "y_lengths": lens.copy(),
                "kept_first": np.zeros(self.B, np.int64), "kept_count": counts, "fit_scale": np.array([1.25]),
                "fit_frames": np.array([77], np.int64), "fit_status": np.array([0], np.int32)}

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None,
                                  fit=None, **more):
        self.fit, self.B = fit, ids.shape[0]
        return iter(())

    last_durations = synthesize_batch = None


def test_the_voice_turns_seconds_into_one_group_of_frames():
    from phoonnx_amd.config import SynthesisConfig
    rec = _Fitting()
    v = _voice(rec)
    cfg = SynthesisConfig(normalize_audio=False)
    out = v.synthesize_encoded("ab. c. de", cfg, duration=2.0)
    assert rec.B == 3 and rec.fit.groups.tolist() == [0, 0, 0] and rec.fit.modes.tolist() == [1]
    assert rec.fit.target_frames.tolist() == [int(np.floor(2.0 * 22050 / 256 + 0.5))] == [172]
    assert out.fit_scale == 1.25 and out.fit_status == 0
    # the pauses the call itself adds come off the slot: a lead and a tail per sentence
    v.synthesize_encoded("ab. c. de", cfg, duration=2.0, duration_mode="at_most", sentence_silence=0.1, trailing_silence=0.05)
    pauses = 3 * (2205 + 1102)
    assert rec.fit.target_frames.tolist() == [int(np.floor((44100 - pauses) / 256 + 0.5))] and rec.fit.modes.tolist() == [2]
    # at an output rate the slot is counted at the delivered rate and the frames at the voice's own
    v8 = _voice(_Fitting(), output_sample_rate=8000)
    v8.synthesize_encoded("ab. c", cfg, duration=1.5, sentence_silence=0.25)
    want = int(np.floor((1.5 * 8000 - 2 * 2000) * 22050 / (8000 * 256) + 0.5))
    assert v8.session.fit.target_frames.tolist() == [want] == [86]
    # without duration nothing is passed down, and the result's fields stay None
    out = v.synthesize_encoded("ab", cfg)
    assert rec.fit is None and out.fit_scale is None and out.fit_status is None
    # the stream: leads only
    list(v.stream_encoded("ab. c", cfg, duration=1.0, sentence_silence=0.1))
    assert rec.B == 2 and rec.fit.target_frames.tolist() == [int(np.floor((22050 - 2 * 2205) / 256 + 0.5))]


def test_the_voices_refusals():
    from phoonnx_amd.config import SynthesisConfig
    cfg = SynthesisConfig(normalize_audio=False)
    v = _voice(_Fitting())
    with pytest.raises(ValueError, match="below 1 frame"):
        v.synthesize_encoded("ab", cfg, duration=0.005)
    with pytest.raises(ValueError, match="below 1 frame"):
        v.synthesize_encoded("ab. c", cfg, duration=1.0, sentence_silence=0.5)
    with pytest.raises(ValueError, match="below 1 frame"):
        list(v.stream_encoded("ab", cfg, duration=0.005))
    with pytest.raises(ValueError, match="duration_mode must be 'exact' or 'at_most'"):
        v.synthesize_encoded("ab", cfg, duration=1.0, duration_mode="max")
    with pytest.raises(ValueError, match="duration_mode must be"):
        v.stream_encoded("ab", cfg, duration=1.0, duration_mode="max")
    for bad in (0.0, -1.0, float("nan"), float("inf"), "2"):
        with pytest.raises(ValueError, match="duration must be a finite number of seconds > 0"):
            v.synthesize_encoded("ab", cfg, duration=bad)
    class Warps(_Fitting):
        def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", fit=None,
                                 token_semitones=None, token_semitones_end=None, **more):
            raise AssertionError("not reached")

        def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None,
                                      fit=None, token_semitones=None, token_semitones_end=None, **more):
            raise AssertionError("not reached")

    for kw in (dict(phoneme_pitch=1.0), dict(pitch_contour=[(0.0, 0.0), (1.0, 2.0)])):
        with pytest.raises(ValueError, match="duration together with phoneme_pitch / pitch_contour is not covered"):
            _voice(Warps()).stream_encoded("ab", cfg, duration=1.0, **kw)
        with pytest.raises(ValueError, match="duration together with phoneme_pitch / pitch_contour is not covered"):
            _voice(Warps()).synthesize_encoded("ab", cfg, duration=1.0, **kw)

    class Old(_Fitting):
        def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16"):
            raise AssertionError("not reached")

        def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames=64, encoding="pcm16", ref_peak=None, volume=None):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match=r"duration needs a session that fits durations on the device \(synthesize_delivered\(fit=\)\)"):
        _voice(Old()).synthesize_encoded("ab", cfg, duration=1.0)
    with pytest.raises(ValueError, match=r"duration needs a session .*synthesize_stream_encoded\(fit=\)"):
        _voice(Old()).stream_encoded("ab", cfg, duration=1.0)

    class NoDelivery:
        get_inputs, hparam = _Fitting.get_inputs, _Fitting.hparam
        HOP = 256

    with pytest.raises(ValueError, match="duration needs a session that fits"):
        _voice(NoDelivery()).synthesize_encoded("ab", cfg, duration=1.0)
    assert "before trim_silence" in type(v).synthesize_encoded.__doc__.replace("BEFORE", "before")
