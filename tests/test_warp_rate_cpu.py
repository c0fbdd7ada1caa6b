"""Pitch at an output rate (include/vitsmi.h, "pitch at an output rate") without a GPU: the folded plan entries against
tests/warp_rate_ref.py record by record, the integer cutoff rule against the double rule on every admitted step, the gain and
tone figures re-measured on the reference, the integer range of a gliding token, the identity-row rule and the refusals on a
host-only handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glide_ref
import warp_rate_ref as ref
import warp_ref
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")
ONE = ref.ONE
SEMITONES = (-12, -5, 0, 3, 12)


def _lib():
    from phoonnx_amd import _ffi
    return _ffi, _ffi.load()


def _durations(rng, T):
    """durations with zeros, 1-frame tokens and longer ones"""
    return rng.choice([0, 1, 1, 2, 3, 7, 12], size=T).astype(np.int64)


def _rows(rng):
    yield _durations(rng, 24), rng.choice(SEMITONES, size=24).astype(np.float32)
    yield _durations(rng, 17), rng.uniform(-12, 12, size=17).astype(np.float32)
    yield np.ones(9, np.int64), np.full(9, 12, np.float32)                    # 1-frame tokens
    yield np.array([5], np.int64), np.array([-5], np.float32)                 # a row of one token
    yield np.array([0, 0, 4, 0], np.int64), np.array([3, 3, -12, 0], np.float32)
    yield np.zeros(3, np.int64), np.zeros(3, np.float32)                      # nothing kept


def test_the_entries_are_declared_and_exported():
    _ffi, lib = _lib()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_warp_token_rate", "vits_warp_plan_rate", "vits_glide_plan_rate", "vits_glide_cutoff_rate", "vits_glide_pos_rate",
                 "vits_rate_identity_spans", "vits_test_warp_rate", "vits_test_glide_rate", "vits_set_pitch_at_rate"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert "pitch at an output rate" in header and "folding the rate into step is a follow-up" not in header


def test_without_the_setting_a_rate_stays_refused():
    """vits_set_pitch_at_rate is off by default: the pitched calls keep the refusal they always had, word for word"""
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    s = MiSession(PATH, host_only=True)
    ids, lens = np.ones((1, 4), np.int64), np.array([4], np.int64)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    st = np.array([[0, 2, 0, 0]], np.float32)
    s.set_output_rate(8000)
    assert s.pitch_at_rate is False
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, token_semitones=st)
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.synthesize_stream(ids, lens, scales, token_semitones=st)
    s.set_pitch_at_rate(True)
    with pytest.raises(SessionError, match="host-only"):
        s.synthesize_batch(ids, lens, scales, token_semitones=st)
    s.set_pitch_at_rate(False)
    with pytest.raises(SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, token_semitones=st)
    s.close()


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_the_folded_token_and_plans_equal_the_reference_record_by_record(fi, fo):
    from phoonnx_amd import session as ses
    L, M = ref.ratio(fi, fo)
    assert ref.admitted(L, M)
    for st in list(SEMITONES) + [-11.99, 0.01, 7.3]:
        got = ses.warp_token_rate(st, L, M)
        assert got == ref.token(st, L, M), st
        assert ref.MIN_STEP <= got[0] <= ref.MAX_STEP and got[2] <= ref.MAX_HALF
    rng = np.random.default_rng(fi * 7 + fo)
    for hop in (256, 1):
        for D, st in _rows(rng):
            segs, spans, N = ses.warp_plan_rate(D, st, hop, L, M)
            want, wspans, wN = ref.plan(D, st, hop, L, M)
            assert [warp_ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in segs] == want
            assert np.array_equal(spans, wspans) and N == wN and int(spans.sum()) == N
            # the row ends within one output step of its native end: N counts delivered samples
            if len(want):
                assert abs(want[-1].pos0 + want[-1].k * want[-1].step - ((int(D.sum()) * hop) << ref.FB)) < want[-1].step
            st1 = np.clip(st + rng.uniform(-4, 4, size=len(st)), -12, 12).astype(np.float32)
            gsegs, gspans, gN = ses.glide_plan_rate(D, st, st1, hop, L, M)
            gwant, gwspans, gwN = ref.glide_plan(D, st, st1, hop, L, M)
            assert [glide_ref.Seg(g.n0, g.pos0, g.k, g.step0, g.step1) for g in gsegs] == gwant
            assert np.array_equal(gspans, gwspans) and gN == gwN
            # equal ends: the glide plan reproduces the folded warp plan
            esegs, espans, eN = ses.glide_plan_rate(D, st, st, hop, L, M)
            assert [(g.n0, g.pos0, g.k, g.step0, g.step1) for g in esegs] == [(g.n0, g.pos0, g.k, g.step, g.step) for g in want] and eN == wN


def test_equal_rates_are_the_unfolded_plans():
    from phoonnx_amd import session as ses
    rng = np.random.default_rng(5)
    for D, st in _rows(rng):
        a, b = ses.warp_plan_rate(D, st, 256, 1, 1), ses.warp_plan(D, st, 256)
        assert bytes(a[0]) == bytes(b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        a, b = ses.glide_plan_rate(D, st, -st, 256, 1, 1), ses.glide_plan(D, st, -st, 256)
        assert bytes(a[0]) == bytes(b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_the_integer_cutoff_equals_the_double_rule_on_every_admitted_step():
    _, lib = _lib()
    s = np.arange(ref.MIN_STEP, ref.MAX_STEP + 1, dtype=np.int64)
    want_c = np.rint(warp_ref.RHO * np.minimum(1.0, ONE / s.astype(np.float64)) * ONE).astype(np.int64)
    want_Kh = -(-warp_ref.Z * ONE // want_c)
    c, Kh = C.c_int64(), C.c_int32()
    got = np.empty((len(s), 2), np.int64)
    for i, v in enumerate(s.tolist()):
        assert lib.vits_glide_cutoff_rate(v, C.byref(c), C.byref(Kh)) == 0
        got[i] = c.value, Kh.value
    assert np.array_equal(got[:, 0], want_c) and np.array_equal(got[:, 1], want_Kh)
    assert tuple(got[-1]) == (6963, ref.MAX_HALF) and int(got[:, 1].max()) == ref.MAX_HALF
    for bad in (ref.MIN_STEP - 1, ref.MAX_STEP + 1, 0, -3):
        assert lib.vits_glide_cutoff_rate(bad, None, None) != 0
    # the unfolded entry keeps its own limits
    assert lib.vits_glide_cutoff(ref.MAX_STEP, None, None) != 0 and lib.vits_glide_cutoff(ref.MIN_STEP, None, None) != 0


def _listed_steps():
    return sorted({ref.token(st, *ref.ratio(fi, fo))[0] for fi, fo in ref.PAIRS for st in SEMITONES})


def test_the_gain_of_the_reference_stays_below_the_tolerances_bound():
    listed = set(_listed_steps()) | {ref.MIN_STEP, ONE, ref.MAX_STEP}
    g = ref.gain(listed)
    print(f"max s * sum|w| over the {len(listed)} listed steps: {g:.4f}")
    assert g <= warp_ref.GAIN                                                 # 1.947 on the reference
    assert ref.gain([s for s in listed if s <= ONE]) == pytest.approx(1.9302, abs=2e-4)
    # a dense grid passes 1.98 (1.98693 over every step: warp_rate_ref.GAIN) - the bound this reference's tolerance counts with
    dense = ref.gain(set(range(ONE, ref.MAX_STEP + 1, 997)) | {111411, 111412})
    print(f"... over a dense grid: {dense:.4f}")
    assert warp_ref.GAIN < dense <= ref.GAIN


def test_the_tone_lands_at_step_times_its_frequency():
    worst = 0.0
    for fi, fo in ref.PAIRS:
        t = ref.tone(*ref.ratio(fi, fo))
        print(f"{fi} -> {fo}: tone error {t:.3e}")
        worst = max(worst, t)
    assert worst <= 2.5e-5


def test_a_folded_gliding_token_past_2_to_the_22_is_refused_and_one_at_the_limit_is_exact():
    _ffi, lib = _lib()
    # 8000 -> 32000 (L / M = 4): a token gliding -12 -> -11 over 2^20 input samples has some 8 million delivered ones
    D, st0, st1 = np.array([1 << 12], np.int64), np.array([-12], np.float32), np.array([-11], np.float32)
    n = C.c_int64()
    assert lib.vits_glide_plan_rate(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), 1, 256, 4, 1, None, None, C.byref(n)) < 0
    err = lib.vits_last_error(None)
    assert b"token 0" in err and b"gliding token" in err and str(ref.MAX_SPAN).encode() in err
    D[0] = 1 << 10
    assert lib.vits_glide_plan_rate(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), 1, 256, 4, 1, None, None, C.byref(n)) == 1
    # ... and the unfolded plan keeps 2^23: the same token without a rate
    D[0] = 1 << 14                                                           # 2^22 input samples at steps near ONE / 2: < 2^23
    assert lib.vits_glide_plan(_ffi.ptr(D), _ffi.ptr(st0), _ffi.ptr(st1), 1, 256, None, None, C.byref(n)) == 1
    assert ref.MAX_SPAN < n.value <= glide_ref.MAX_SPAN
    # exactly 2^22 samples at the largest |b - a|, both directions: the positions are Python's integers
    pos, step = C.c_int64(), C.c_int64()
    for a, b in ((ref.MIN_STEP, ref.MAX_STEP), (ref.MAX_STEP, ref.MIN_STEP)):
        g = glide_ref.Seg(0, 12345, ref.MAX_SPAN, a, b)
        rec = _ffi.VitsGlideSeg(g.n0, g.pos0, g.k, a, b)
        for j in (0, 1, 2, 12345, ref.MAX_SPAN // 2, ref.MAX_SPAN - 1, ref.MAX_SPAN):
            assert lib.vits_glide_pos_rate(C.byref(rec), j, C.byref(pos), C.byref(step)) == 0
            assert pos.value == glide_ref.pos_at(g, j), (a, b, j)
            assert step.value == glide_ref.step_at(g, min(j, g.k))
        assert (abs(b - a) * ref.MAX_SPAN * (ref.MAX_SPAN - 1)) < 1 << 63 < abs(b - a) * (2 * ref.MAX_SPAN) * (2 * ref.MAX_SPAN - 1)
    rec = _ffi.VitsGlideSeg(0, 0, ref.MAX_SPAN + 1, ref.MIN_STEP, ref.MAX_STEP)
    assert lib.vits_glide_pos_rate(C.byref(rec), 1, C.byref(pos), None) != 0


def test_an_identity_rows_spans_are_the_resamplers_rule():
    from phoonnx_amd import session as ses
    rng = np.random.default_rng(11)
    for fi, fo in ref.PAIRS + [(22050, 22050)]:
        L, M = ref.ratio(fi, fo)
        for hop in (256, 3):
            D = _durations(rng, 19)
            n_in = int(D.sum()) * hop
            for n in (n_in, max(n_in - hop, 0)):                              # (a row cut short: the spans are clamped to N)
                spans, N = ses.rate_identity_spans(D, hop, L, M, n)
                want, wN = ref.identity_spans(D, hop, L, M, n)
                assert np.array_equal(spans, want) and N == wN == -(-n * L // M) and int(spans.sum()) == min(N, -(-n_in * L // M))
                assert (spans >= 0).all() and (spans[D == 0] == 0).all()


def test_a_ratio_outside_the_admitted_range_is_refused_with_pitch():
    _ffi, lib = _lib()
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError
    for L, M in ((1, 5), (5, 1), (80, 441), (0, 1)):
        assert lib.vits_warp_token_rate(1.0, L, M, None, None, None) != 0 and b"outside [1/4, 4]" in lib.vits_last_error(None)
        D, st = np.array([3], np.int64), np.array([1], np.float32)
        assert lib.vits_warp_plan_rate(_ffi.ptr(D), _ffi.ptr(st), 1, 256, L, M, None, None, None) < 0
        assert lib.vits_glide_plan_rate(_ffi.ptr(D), _ffi.ptr(st), None, 1, 256, L, M, None, None, None) < 0
    assert lib.vits_warp_token_rate(1.0, 1, 4, None, None, None) == 0 and lib.vits_warp_token_rate(1.0, 4, 1, None, None, None) == 0
    s = MiSession(PATH, host_only=True, pitch_at_rate=True)
    fi = int(s.meta("sample_rate") or 22050)
    ids, lens = np.ones((1, 4), np.int64), np.array([4], np.int64)
    scales = np.array([0.667, 1.0, 0.8], np.float32)
    st0, st1 = np.array([[0, 2, 0, 0]], np.float32), np.array([[0, 4, 1, 0]], np.float32)
    far = fi // 5
    for setter, arg in ((s.set_output_rate, far), (s.set_output_rates, [far])):
        setter(arg)
        for kw in (dict(token_semitones=st0), dict(token_semitones=st0, token_semitones_end=st1)):
            with pytest.raises(SessionError, match=rf"{fi} -> {far} Hz.*outside \[1/4, 4\]"):
                s.synthesize_batch(ids, lens, scales, **kw)
        # an unpitched row at that rate is the resampler's business: the call gets as far as the device
        with pytest.raises(SessionError, match="host-only"):
            s.synthesize_batch(ids, lens, scales, token_semitones=np.zeros((1, 4), np.float32))
        setter(None)
    # an admitted rate: no refusal of the rate any more - a host-only handle gets as far as the device
    for setter, arg in ((s.set_output_rate, 8000), (s.set_output_rates, [8000])):
        setter(arg)
        with pytest.raises(SessionError, match="host-only"):
            s.synthesize_batch(ids, lens, scales, token_semitones=st0, token_semitones_end=st1)
        setter(None)
    s.close()


@pytest.mark.parametrize("fo", [8000, 48000])
@pytest.mark.parametrize("frames", [1, 7, 64])
def test_the_wide_stream_rules_against_a_brute_force_count(fo, frames):
    """warp_emit_end / warp_stream_cap with the plan's largest Kh and least step: every value against a count over the
    reference's positions, piece by piece"""
    from phoonnx_amd import session as ses
    import resample_ref
    fi, hop = 22050, 16
    L, M = ref.ratio(fi, fo)
    rng = np.random.default_rng(fo + frames)
    D = rng.choice([0, 1, 2, 5, 9], size=40).astype(np.int64)
    st0 = rng.choice(SEMITONES, size=40).astype(np.float32)
    st1 = np.clip(st0 + rng.uniform(-6, 6, 40), -12, 12).astype(np.float32)
    n_in = int(D.sum()) * hop
    plans = [(ses.warp_plan_rate(D, st0, hop, L, M), ref.plan(D, st0, hop, L, M)),
             (ses.glide_plan_rate(D, st0, st1, hop, L, M), ref.glide_plan(D, st0, st1, hop, L, M))]
    K = resample_ref.plan(fi, fo)[2]
    N_id = -(-n_in * L // M)
    id_i = np.arange(N_id, dtype=np.int64) * M // L
    piece = frames * hop
    for (segs, _, N), (rsegs, _, rN) in plans:
        assert N == rN
        half = ref.max_half(rsegs)
        lo = min(min(g.step0, g.step1) if hasattr(g, "step0") else g.step for g in rsegs)
        min_step = min(lo, M * ONE // L)                                      # (an identity row of the same run joins the least)
        i0 = np.array([ref.row_pos(rsegs, n) >> ref.FB for n in range(N)], np.int64)
        assert (np.diff(i0) >= 0).all()
        cap = ses.warp_stream_cap_rate(piece, max(N, N_id), min_step, half)
        assert cap == min(max(N, N_id), -(-(piece + half) * ONE // min_step))
        prev = prev_id = 0
        for X in list(range(piece, n_in, piece)) + [n_in]:
            want = N if X >= n_in else int((i0 + half < X).sum())
            assert ses.warp_emit_end_rate(segs, n_in, N, X, half) == want, X
            want_id = N_id if X >= n_in else int((id_i + K // 2 <= X - 1).sum())
            assert ses.identity_emit_end_rate(L, M, K, n_in, X) == want_id, X
            if X < n_in:                                                      # what one piece completes fits one delivery
                assert want - prev <= cap and want_id - prev_id <= cap, (X, want - prev, want_id - prev_id, cap)
            prev, prev_id = want, want_id
    # a native identity row (a masked copy): sample n is ready once input n exists
    assert ses.identity_emit_end_rate(1, 1, 0, 100, 37) == 37 and ses.identity_emit_end_rate(1, 1, 0, 100, 100) == 100


def test_unfolded_plans_get_exactly_todays_stream_values():
    from phoonnx_amd import session as ses
    rng = np.random.default_rng(3)
    D = rng.choice([0, 1, 2, 5, 9], size=30).astype(np.int64)
    st = rng.choice(SEMITONES, size=30).astype(np.float32)
    segs, _, N = ses.warp_plan(D, st, 16)
    gsegs, _, gN = ses.glide_plan(D, st, -st, 16)
    n_in = int(D.sum()) * 16
    for X in range(0, n_in + 40, 37):
        assert ses.warp_emit_end_rate(segs, n_in, N, X, 38) == ses.warp_emit_end(segs, n_in, N, X)
        assert ses.warp_emit_end_rate(gsegs, n_in, gN, X, 38) == ses.glide_emit_end(gsegs, n_in, gN, X)
    for p, S_w in ((1, 5), (256, 100000), (64 * 256, 10 ** 6), (7, 90)):
        assert ses.warp_stream_cap_rate(p, S_w, ONE // 2, 38) == ses.warp_stream_cap(p, S_w) == min(S_w, 2 * (p + 38))


def test_the_voice_refuses_a_far_rate_with_a_value_error():
    """with pitch_at_rate a rate outside a quarter .. four times the voice's own is the voice's ValueError, like its other
    refusals - before the session is asked"""
    from test_warp_cpu import _Recorder, _voice

    class Folds(_Recorder):
        def set_output_rate(self, rate, input_rate=None):
            self.rate = rate

        def set_pitch_at_rate(self, on=True):
            self.folds = on

    sess = Folds()
    v = _voice(sess, output_sample_rate=4410, pitch_at_rate=True)
    assert sess.folds is True
    with pytest.raises(ValueError, match=r"phoneme_pitch is not covered at 4410 Hz.*outside \[1/4, 4\]"):
        v.synthesize_encoded("ab", phoneme_pitch=1.0)
    near = _voice(Folds(), output_sample_rate=8000, pitch_at_rate=True)
    near.synthesize_encoded("ab", phoneme_pitch=1.0)                        # folded: the semitones reach the session
    assert float(np.abs(near.session.semitones).max()) == 1.0
    with pytest.raises(ValueError, match=r"phoneme_pitch is not covered at 4000 Hz"):
        near.synthesize_requests_encoded([("ab", None)], phoneme_pitch=1.0, output_sample_rates=[4000])
    with pytest.raises(ValueError, match="pitch_at_rate needs a session"):
        _voice(_Recorder(), pitch_at_rate=True)
