"""The per-token time warp on the GPU (include/vitsmi.h, "intonation"): the kernel by value through vits_test_warp, on one
batch with a row for each way it can go wrong; then vits_run_async_warped end to end through MiSession, the delivery on top
of a warped run, the refusals, and TTSVoice.synthesize_encoded(phoneme_pitch=).

Reference: tests/warp_ref.py (the definition in float64) applied to the native waveform of the same run; the bound is
warp_ref.tolerance, derived there."""
import os

import numpy as np
import pytest

import warp_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

B, S, HOP = 4, 900, 4
COUNTS = np.array([900, 700, 130, 0], np.int64)


def _batch():
    """(x [B, S], per row (D, st)): row 0 has boundaries exactly at outputs 256 and 512 (two 64-frame tokens at 0
    semitones), a 1-frame token, a dropped token and +12 next to -12, the rest inside tiles; row 1 is random short tokens;
    row 2 is an identity row whose plan runs 2 samples past its valid ones; row 3 has segments and no valid sample."""
    rng = np.random.default_rng(31)
    x = (rng.standard_normal((B, S)) * 0.5).astype(np.float32)
    for b in range(B):
        x[b, COUNTS[b]:] = 1000.0                                    # what lies behind a row's valid samples must not show
    d1 = []
    while sum(d1) < 175:
        d1.append(int(min(rng.integers(0, 6), 175 - sum(d1))))
    rows = [
        ([64, 64, 1, 0, 10, 10, 7, 5, 30, 34], [0, 0, 5, 3, 12, -12, -3.3, 7, -7, 1]),
        (d1, rng.uniform(-12, 12, len(d1)).round(2).tolist()),
        ([10, 0, 23], [0, 0, 0]),
        ([2, 3], [3, -2]),
    ]
    assert sum(rows[0][0]) * HOP == 900 and sum(rows[1][0]) * HOP == 700
    return x, rows


_CACHE = {}


def _by_value():
    """the batch through the hook and through the reference, once"""
    if not _CACHE:
        from phoonnx_amd import session as ses
        x, rows = _batch()
        plans = [ses.warp_plan(D, st, HOP) for D, st in rows]
        rplans = [ref.plan(D, st, HOP) for D, st in rows]
        for (segs, spans, N), (rsegs, rspans, rN) in zip(plans, rplans):
            assert [ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in segs] == rsegs and N == rN
        y = ses.test_warp(x, COUNTS, [p[0] for p in plans])
        want = [ref.warp64(x[b, :COUNTS[b]], rplans[b][0], rplans[b][2]) for b in range(B)]
        _CACHE.update(x=x, plans=plans, rplans=rplans, y=y, want=want)
        y.setflags(write=False)
    return _CACHE


def test_the_batch_covers_what_it_claims():
    c = _by_value()
    segs = c["rplans"][0][0]
    assert {256, 512} <= {g.n0 for g in segs}                          # boundaries exactly at tile edges
    assert any(g.n0 % 256 and g.k for g in segs)                       # ... and inside tiles
    assert any(a.Kh == 38 and b.step == ref.ONE // 2 for a, b in zip(segs, segs[1:]))   # +12 next to -12
    assert c["rplans"][0][2] > 768 and c["y"].shape == (B, max(p[2] for p in c["rplans"]))
    assert ref.identity(c["rplans"][2][0]) and c["rplans"][2][2] == 132
    assert max(g.k for g in c["rplans"][1][0]) < 64                    # short segments: a tile straddles several


def test_every_sample_is_within_the_tolerance_of_the_definition():
    c = _by_value()
    for b in range(B):
        segs, _, N = c["rplans"][b]
        tol = ref.tolerance(segs, float(np.abs(c["x"][b, :COUNTS[b]]).max()) if COUNTS[b] else 0.0)
        err = float(np.abs(c["y"][b, :N] - c["want"][b]).max()) if N else 0.0
        print(f"row {b}: N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (b, err, tol)
        assert np.abs(c["want"][b]).max() > 0.1 or b >= 2              # (the rows that carry signal carry it)


def test_identity_rows_and_tails_are_exact():
    c = _by_value()
    y, x = c["y"], c["x"]
    assert np.array_equal(y[2, :130], x[2, :130]) and not y[2, 130:].any()   # a masked copy: zeros behind n_b
    assert not y[3].any()                                                     # no valid input sample: zeros
    for b in range(B):
        assert not y[b, c["rplans"][b][2]:].any(), b                          # exact zeros behind every N_b


def test_a_row_alone_is_its_row_in_the_batch():
    from phoonnx_amd import session as ses
    c = _by_value()
    for b in range(B):
        N = c["rplans"][b][2]
        alone = ses.test_warp(c["x"][b:b + 1], COUNTS[b:b + 1], [c["plans"][b][0]])
        assert alone.shape == (1, max(1, N)) and np.array_equal(alone[0, :N], c["y"][b, :N]), b


def test_records_that_do_not_continue_their_row_are_refused():
    from phoonnx_amd import _ffi, session as ses
    c = _by_value()
    segs = list(c["plans"][0][0])
    bad = _ffi.VitsWarpSeg(segs[1].n0, segs[1].pos0 - 65536, segs[1].k, segs[1].step, segs[1].c, segs[1].half_taps, 0)
    with pytest.raises(ses.SessionError, match="row 0: segment 1"):
        ses.test_warp(c["x"][:1], COUNTS[:1], [[segs[0], bad] + segs[2:]])


# ------------------------------------------------------------------ end to end

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _inputs(s, seed=12):
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    sem = np.zeros((3, 40), np.float32)
    pattern = np.array([3, 0, -4, 7, -12, 12, 0.5, -1], np.float32)
    for b in range(3):
        sem[b, :lens[b]] = np.resize(np.roll(pattern, b), lens[b])
    sem[:, 39] = 99.0                                                  # behind lens of rows 1 and 2: ignored ...
    sem[0, 39] = 2.0                                                   # ... a token of row 0
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64), sem


@pytest.mark.parametrize("preset", ["tiny_rb2_ms", "sx_rb1"])
def test_a_compensated_run_is_the_rate_scaled_run_warped(preset):
    s = _session(preset)
    hop = s.hparam("hop")
    ids, lens, scales, sid, seeds, sem = _inputs(s)
    live = np.arange(40)[None, :] < lens[:, None]
    rate = np.where(live, np.exp2(np.where(live, sem, 0).astype(np.float64) / 12.0).astype(np.float32), np.float32(1)).astype(np.float32)
    base = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_rate=rate, return_durations=True)
    native = base["output"][:, 0, 0].copy()
    launches = s.stats()["total_launches"]
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem, compensate=True, return_durations=True)
    assert s.stats()["total_launches"] == launches + 1                 # the one warp launch on top
    assert np.array_equal(r["durations"], base["durations"]) and np.array_equal(r["y_lengths"], base["y_lengths"])
    plans = [ref.plan(base["durations"][b, :lens[b]], sem[b, :lens[b]], hop) for b in range(3)]
    assert r["sample_lengths"].tolist() == [p[2] for p in plans]
    assert np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    assert r["output"].shape == (3, 1, 1, max(p[2] for p in plans))
    for b in range(3):
        segs, spans, N = plans[b]
        n_b = int(base["y_lengths"][b]) * hop
        want = ref.warp64(native[b, :n_b], segs, N)
        tol = ref.tolerance(segs, float(np.abs(native[b, :n_b]).max()))
        got = r["output"][b, 0, 0]
        err = float(np.abs(got[:N] - want).max())
        print(f"{preset} row {b}: n_b = {n_b}, N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol and not got[N:].any(), (b, err, tol)
        assert np.array_equal(r["token_spans"][b, :lens[b]], spans) and not r["token_spans"][b, lens[b]:].any()
        # the tempo is kept: the warped row is as long as the unscaled run's would be, within a sample a token
        assert abs(N - float((base["durations"][b, :lens[b]] * hop / rate[b, :lens[b]].astype(np.float64)).sum())) < 2 + lens[b]
    assert np.array_equal(s.last_token_spans(), r["token_spans"])
    # the pure warp: ctl untouched - the free run's durations, its waveform warped
    free = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    pure = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem, compensate=False, return_durations=True)
    assert np.array_equal(pure["durations"], free["durations"])
    for b in range(3):
        segs, spans, N = ref.plan(free["durations"][b, :lens[b]], sem[b, :lens[b]], hop)
        n_b = int(free["y_lengths"][b]) * hop
        x = free["output"][b, 0, 0, :n_b]
        assert pure["sample_lengths"][b] == N
        assert float(np.abs(pure["output"][b, 0, 0, :N] - ref.warp64(x, segs, N)).max()) <= ref.tolerance(segs, float(np.abs(x).max()))
    s.close()


def test_zero_semitones_are_the_unwarped_run():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, _ = _inputs(s)
    base = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    launches = s.stats()["total_launches"]
    zero = np.zeros((3, 40), np.float32)
    zero[1, 30] = 5.0                                                  # behind lens[1]: ignored
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=zero, return_durations=True)
    assert s.stats()["total_launches"] == launches                     # no warp was planned or launched
    assert np.array_equal(r["output"], base["output"]) and np.array_equal(r["durations"], base["durations"])
    assert np.array_equal(r["sample_lengths"], base["y_lengths"] * s.hparam("hop"))
    assert np.array_equal(r["token_spans"], base["durations"] * s.hparam("hop"))
    with pytest.raises(ses.SessionError, match="not warped"):          # vits_last_token_spans after an unwarped run
        s.last_token_spans()
    s.close()


def test_delivery_on_top_of_a_warped_run():
    from phoonnx_amd import audio_encoding as ae
    from phoonnx_amd.session import Segment
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, sem = _inputs(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem)
    counts = r["sample_lengths"]
    streams = s.deliver([Segment(b, b, 0, 0, 1.0) for b in range(3)], 3, "pcm16")
    for b in range(3):
        want = ae.encode(r["output"][b, 0, 0, :counts[b]], "pcm16")    # the fetched warped waveform over N_b
        assert np.ascontiguousarray(streams[b]).tobytes() == np.ascontiguousarray(want).tobytes(), b
    # ... and in one call: the same bytes, with the warp's counts and spans
    d = s.synthesize_delivered(ids, lens, scales, sid, seeds=seeds, token_semitones=sem, normalize=False, volume=1.0,
                               return_durations=True)
    assert np.array_equal(d["sample_lengths"], counts) and np.array_equal(d["token_spans"].sum(axis=1), counts)
    for b in range(3):
        assert np.ascontiguousarray(d["streams"][b]).tobytes() == np.ascontiguousarray(streams[b]).tobytes(), b
    # the 16-bit rendering works on the warped buffer too
    pcm = s.last_pcm16(False, 1.0, shape=(3, int(counts.max())))
    for b in range(3):
        assert pcm[b, :counts[b]].tobytes() == np.ascontiguousarray(streams[b]).tobytes() and not pcm[b, counts[b]:].any()
    s.close()


def test_refusals_leave_the_previous_run_readable():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds, sem = _inputs(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem)
    s.set_output_rate(8000)
    with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem)
    s.set_output_rate(None)
    s.set_output_rates([8000, 0, 16000])
    with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=sem)
    s.set_output_rates(None)
    bad = sem.copy()
    bad[2, 3] = -13.0
    with pytest.raises(ses.SessionError, match=r"token_semitones\[2,3\]"):
        s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=bad)
    again = np.empty_like(r["output"])
    s._fetch(again, 0, 3)                                              # the warped run is still there
    assert np.array_equal(again, r["output"]) and np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    s.close()


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def test_synthesize_encoded_with_phoneme_pitch():
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    s = _session("tiny_rb2_ms")
    n_vocab, n_spk = s.hparam("n_vocab"), s.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    v = TTSVoice(session=s, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)
    out = v.synthesize_encoded("hello there. go", alignments=True, phoneme_pitch=2.0, sentence_silence=0.01)
    counts = s.last_sample_counts()
    assert out.sentence_samples == [int(n) for n in counts] and np.array_equal(s.last_token_spans().sum(axis=1), counts)
    lead = int(22050 * 0.01 * 2) // 2
    for k, al in enumerate(out.phoneme_alignments):
        assert al[0].start_sample == out.sentence_starts[k] and sum(a.num_samples for a in al) == counts[k]
        assert al[-1].start_sample + al[-1].num_samples == out.sentence_starts[k] + counts[k]   # the last end: the delivered count
    assert out.sentence_starts[0] == lead and len(out.data) == sum(lead + int(n) for n in counts)
    # a value per phoneme, with a volume per phoneme on top: its breakpoints lie within the warped sentence
    per = v.synthesize_encoded("hello there. go", alignments=True, phoneme_pitch=lambda k, tokens: [(-1.0) ** i * 3 for i in range(len(tokens))],
                               phoneme_gain_db=lambda k, tokens: [-6.0 * (i % 2) for i in range(len(tokens))], fade_out=0.002)
    assert per.sentence_samples == [int(n) for n in s.last_sample_counts()]
    s.close()
