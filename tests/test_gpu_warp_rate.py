"""Pitch at an output rate on the GPU (include/vitsmi.h, "pitch at an output rate"): warp_rate_kernel and glide_rate_kernel by
value through vits_test_warp_rate / vits_test_glide_rate on one batch of five rows, then the whole path through MiSession - a
pitched run with an output rate or per-row rates set, the delivery on top of it - and TTSVoice.

Reference: tests/warp_rate_ref.py (the folded token and the identity-row rule on top of warp_ref / glide_ref / resample_ref)
in float64; the bound is warp_rate_ref.tolerance - warp_ref.tolerance's derivation with the gain bound measured over every
admitted step.  The whole path is compared bit for bit against the hooks applied to the run's native waveform."""
import os

import numpy as np
import pytest

import delivery_ref
import glide_ref
import warp_rate_ref as ref
import warp_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

S, HOP = 3000, 4
COUNTS = np.array([3000, 2900, 2801, 2777, 0], np.int64)
IN = np.array([22050, 22050, 16000, 22050, 22050], np.int32)
OUT = np.array([8000, 48000, 8000, 8000, 8000], np.int32)
B = 5


def _batch():
    """(x [B, S], per row (D, st0, st1)):
    0  22050 -> 8000, one-frame tokens at +12: step 5.51, Kh = 104, some 350 segments under a tile, most records without a sample
    1  22050 -> 48000 at -12: step 0.23, 13 000 output samples from 2 900
    2  16000 -> 8000, one token gliding -12 -> +12 (the warp's launch: constant tokens at +3 and -5 in its place)
    3  an identity row at 22050 -> 8000: the resampler's row
    4  an empty row"""
    rng = np.random.default_rng(83)
    x = rng.uniform(-1, 1, (B, S)).astype(np.float32)
    for b in range(B):
        x[b, COUNTS[b]:] = 1000.0                                    # what lies behind a row's valid samples must not show
    rows = [([1] * 750, [12] * 750, [12] * 750), ([725], [-12], [-12]), ([700], [-12], [12]), None, None]
    return x, rows


_CACHE = {}


def _by_value():
    """the batch through both hooks and through the reference, once"""
    if _CACHE:
        return _CACHE
    from phoonnx_amd import session as ses
    x, rows = _batch()
    LM = [ref.ratio(IN[b], OUT[b]) for b in range(B)]
    # the glide's launch: rows 0 and 1 as records with equal ends, row 2 gliding
    gplans, gref = [], []
    for b, row in enumerate(rows):
        if row is None:
            gplans.append(([], None, int(ref.identity_spans([], HOP, *LM[b], COUNTS[b])[1])))
            gref.append(([], None, gplans[-1][2]))
            continue
        gplans.append(ses.glide_plan_rate(row[0], row[1], row[2], HOP, *LM[b]))
        gref.append(ref.glide_plan(row[0], row[1], row[2], HOP, *LM[b]))
        assert [glide_ref.Seg(g.n0, g.pos0, g.k, g.step0, g.step1) for g in gplans[-1][0]] == gref[-1][0] and gplans[-1][2] == gref[-1][2]
    # the warp's launch: row 2 as two constant tokens
    wrows = list(rows)
    wrows[2] = ([300, 400], [3, -5], None)
    wplans, wref = [], []
    for b, row in enumerate(wrows):
        if row is None:
            wplans.append(gplans[b])
            wref.append(gref[b])
            continue
        wplans.append(ses.warp_plan_rate(row[0], row[1], HOP, *LM[b]))
        wref.append(ref.plan(row[0], row[1], HOP, *LM[b]))
        assert [warp_ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in wplans[-1][0]] == wref[-1][0]
    yg, Ng = ses.test_glide_rate(x, COUNTS, [p[0] for p in gplans], IN, OUT)
    yw, Nw = ses.test_warp_rate(x, COUNTS, [p[0] for p in wplans], IN, OUT)

    def want(b, plan, fn):
        xb = x[b, :COUNTS[b]]
        return fn(xb, plan[0], plan[2]) if plan[0] else ref.identity64(xb, int(IN[b]), int(OUT[b]))

    _CACHE.update(x=x, ses=ses, gplans=gplans, gref=gref, wplans=wplans, wref=wref, yg=yg, yw=yw, Ng=Ng, Nw=Nw,
                  want_g=[want(b, gref[b], ref.glide64) for b in range(B)], want_w=[want(b, wref[b], ref.warp64) for b in range(B)])
    yg.setflags(write=False)
    yw.setflags(write=False)
    return _CACHE


def test_the_batch_covers_what_it_claims():
    c = _by_value()
    segs0 = c["wref"][0][0]
    assert len(segs0) == 750 and segs0[0].Kh == 104 and sum(1 for g in segs0 if g.k == 0) > 150
    assert c["Nw"][0] > 512 and c["Nw"][0] % 256                     # more than one tile, not a multiple of it
    assert c["wref"][1][0][0].step < ref.ONE // 4 and c["Nw"][1] > 12000
    g2 = c["gref"][2][0][0]
    assert g2.step0 == ref.ONE and g2.step1 == 4 * ref.ONE and ref.max_half(c["gref"][2][0]) == 76
    assert c["Ng"].tolist() == [p[2] for p in c["gref"]] and c["Nw"].tolist() == [p[2] for p in c["wref"]]
    assert c["Nw"][3] == -(-2777 * 160 // 441) and c["Nw"][4] == 0
    assert c["yw"].shape == (B, c["Nw"].max()) and c["yg"].shape == (B, c["Ng"].max())


@pytest.mark.parametrize("family", ["warp", "glide"])
def test_every_sample_is_within_the_tolerance_of_the_definition(family):
    c = _by_value()
    y, plans, want = (c["yw"], c["wref"], c["want_w"]) if family == "warp" else (c["yg"], c["gref"], c["want_g"])
    import resample_ref
    for b in range(B):
        segs, _, N = plans[b]
        xmax = float(np.abs(c["x"][b, :COUNTS[b]]).max()) if COUNTS[b] else 0.0
        tol = ref.tolerance(segs, xmax) if segs else resample_ref.tolerance(int(IN[b]), int(OUT[b]), xmax)
        err = float(np.abs(y[b, :N] - want[b]).max()) if N else 0.0
        print(f"{family} row {b}: N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (b, err, tol)
        assert b == 4 or np.abs(want[b]).max() > 0.1                   # (the rows that carry signal carry it)


def test_the_identity_row_is_the_resamplers_row_and_tails_are_zero():
    c = _by_value()
    ses = c["ses"]
    y, counts = ses.test_resample(c["x"][3:4], COUNTS[3:4], 22050, 8000)
    N = int(c["Nw"][3])
    assert counts.tolist() == [N]
    for got in (c["yw"], c["yg"]):
        assert np.array_equal(got[3, :N], y[0, :N])                    # bit for bit, from either kernel
        assert not np.isnan(got).any()                                 # every column was written
    for got, Ns in ((c["yw"], c["Nw"]), (c["yg"], c["Ng"])):
        for b in range(B):
            assert not got[b, Ns[b]:].any(), b                         # exact zeros behind every N_b
    # taps masked to [0, n_b): the 1000.0 behind the rows' valid samples never shows
    assert float(np.abs(c["yw"]).max()) < 4.0 and float(np.abs(c["yg"]).max()) < 4.0


def test_a_row_alone_is_its_row_in_the_batch():
    c = _by_value()
    ses = c["ses"]
    for b in range(B - 1):
        yw, _ = ses.test_warp_rate(c["x"][b:b + 1], COUNTS[b:b + 1], [c["wplans"][b][0]], IN[b:b + 1], OUT[b:b + 1])
        assert np.array_equal(yw[0], c["yw"][b, :yw.shape[1]]), b
    yg, _ = ses.test_glide_rate(c["x"][2:3], COUNTS[2:3], [c["gplans"][2][0]], IN[2:3], OUT[2:3])
    assert np.array_equal(yg[0], c["yg"][2, :yg.shape[1]])


def test_windows_joined_are_the_whole_launch():
    c = _by_value()
    ses = c["ses"]
    for fn, plans, whole in ((ses.test_warp_rate, c["wplans"], c["yw"]), (ses.test_glide_rate, c["gplans"], c["yg"])):
        W = whole.shape[1]
        cuts = [0, 1, 300, 301, 811, 1500, W]                          # no multiple of 256 among them
        parts = [fn(c["x"], COUNTS, [p[0] for p in plans], IN, OUT, window=(lo, hi))[0] for lo, hi in zip(cuts, cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_the_hooks_keep_their_limits():
    from phoonnx_amd import _ffi
    c = _by_value()
    ses = c["ses"]
    wide = c["wplans"][0][0]
    with pytest.raises(ses.SessionError, match="within the limits of a token"):
        ses.test_warp(c["x"][:1], COUNTS[:1], [wide])                  # the unfolded hook refuses a folded record
    g = _ffi.VitsWarpSeg(0, 0, 10, 9 * ref.ONE, 6000, 175, 0)
    with pytest.raises(ses.SessionError, match="within the limits of a token"):
        ses.test_warp_rate(c["x"][:1], COUNTS[:1], [[g]], IN[:1], OUT[:1])
    with pytest.raises(ses.SessionError, match=r"outside \[1/4, 4\]"):
        ses.test_warp_rate(c["x"][:1], COUNTS[:1], [wide], [22050], [4000])


# ------------------------------------------------------------------ the whole path

def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), pitch_at_rate=True, **kw)


def _inputs(s, seed=12):
    rng = np.random.default_rng(seed)
    lens = np.array([40, 21, 9], np.int64)
    ids = np.zeros((3, 40), np.int64)
    for b in range(3):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 3).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8]], np.float32)
    st0, st1 = np.zeros((3, 40), np.float32), np.zeros((3, 40), np.float32)
    p0 = np.array([0, 3, -4, 7, -12, 12, 0.5, 2], np.float32)
    p1 = np.array([3, -4, -4, -12, 12, 0, 0.5, -1], np.float32)
    for b in range(3):
        st0[b, :lens[b]] = np.resize(np.roll(p0, b), lens[b])
        st1[b, :lens[b]] = np.resize(np.roll(p1, b), lens[b])
    st0[1:, 39] = 99.0                                                 # behind lens of rows 1 and 2: ignored
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64), st0, st1


def _native(s, ids, lens, scales, sid, seeds):
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    return r["output"][:, 0, 0].copy(), r["durations"], r["y_lengths"] * s.hparam("hop")


def _hook_rows(ses, native, durations, n_in, lens, hop, fi, rates, st0, st1):
    """every row through the hooks at its rate: (rows [N_b], spans per row) - an unpitched row by the identity rule"""
    rows, spans = [], []
    for b in range(len(lens)):
        fo = int(rates[b] or fi)
        L, M = ref.ratio(fi, fo)
        D, a = durations[b, :lens[b]], st0[b, :lens[b]]
        e = a if st1 is None else st1[b, :lens[b]]
        if not a.any() and not e.any():
            sp, N = ref.identity_spans(D, hop, L, M, int(n_in[b]))
            y, _ = ses.test_warp_rate(native[b:b + 1], n_in[b:b + 1], [[]], fi, [fo])
        elif st1 is None:
            segs, sp, N = ses.warp_plan_rate(D, a, hop, L, M)
            assert [warp_ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in segs] == ref.plan(D, a, hop, L, M)[0]
            y, _ = ses.test_warp_rate(native[b:b + 1], n_in[b:b + 1], [segs], fi, [fo])
        else:
            segs, sp, N = ses.glide_plan_rate(D, a, e, hop, L, M)
            assert [glide_ref.Seg(g.n0, g.pos0, g.k, g.step0, g.step1) for g in segs] == ref.glide_plan(D, a, e, hop, L, M)[0]
            y, _ = ses.test_glide_rate(native[b:b + 1], n_in[b:b + 1], [segs], fi, [fo])
        rows.append(y[0, :N])
        spans.append(sp)
    return rows, spans


@pytest.mark.parametrize("preset,rate,glide", [("tiny_rb1", 8000, False), ("tiny_rb2_ms", 48000, True), ("tiny_rb2_ms", 8000, True)])
def test_a_pitched_run_at_a_rate_is_the_hook_over_its_native_waveform(preset, rate, glide):
    from phoonnx_amd import session as ses
    s = _session(preset)
    hop, fi = s.hparam("hop"), int(s.meta("sample_rate") or 22050)
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    st0[1] = 0                                                         # row 1 unpitched: an identity row of the pitched batch
    st1[1] = 0
    native, durations, n_in = _native(s, ids, lens, scales, sid, seeds)
    s.set_output_rate(rate)
    plain = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)   # the resampled run
    launches = s.stats()["total_launches"]
    kw = dict(token_semitones=st0, token_semitones_end=st1) if glide else dict(token_semitones=st0)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, compensate=False, return_durations=True, **kw)
    assert s.stats()["total_launches"] == launches - 1                 # one folded launch in place of counts + resampler
    assert np.array_equal(r["durations"], durations)
    rows, spans = _hook_rows(ses, native, durations, n_in, lens, hop, fi, [rate] * 3, st0, st1 if glide else None)
    assert r["sample_lengths"].tolist() == [len(y) for y in rows] and np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    assert r["output"].shape == (3, 1, 1, max(len(y) for y in rows))
    assert s.last_sample_rates().tolist() == [rate] * 3
    for b in range(3):
        got = r["output"][b, 0, 0]
        assert np.array_equal(got[:len(rows[b])], rows[b]) and not got[len(rows[b]):].any(), b
        assert np.array_equal(r["token_spans"][b, :lens[b]], spans[b]) and not r["token_spans"][b, lens[b]:].any()
        assert int(r["token_spans"][b].sum()) == len(rows[b])
    # the identity row is the resampled run's row, bit for bit: batching with pitched rows did not change it
    N1 = int(plain["sample_lengths"][1])
    assert r["sample_lengths"][1] == N1 and np.array_equal(r["output"][1, 0, 0, :N1], plain["output"][1, 0, 0, :N1])
    # all-zero semitones: the resampled run itself
    z = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=np.zeros_like(st0), return_durations=True)
    assert np.array_equal(z["output"], plain["output"]) and np.array_equal(z["sample_lengths"], plain["sample_lengths"])
    # compensate: the rate-scaled run's native waveform through the same plan rule - durations are native frames
    if not glide:
        rate_t = np.ones(st0.shape, np.float32)
        for b in range(3):
            for t in range(int(lens[b])):
                rate_t[b, t] = ses.glide_token(st0[b, t], st0[b, t])[2]
        s.set_output_rate(None)
        base = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_rate=rate_t, return_durations=True)
        s.set_output_rate(rate)
        c = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, compensate=True, return_durations=True)
        assert np.array_equal(c["durations"], base["durations"])
        crows, _ = _hook_rows(ses, base["output"][:, 0, 0].copy(), base["durations"], base["y_lengths"] * hop, lens, hop, fi, [rate] * 3, st0, None)
        for b in range(3):
            assert np.array_equal(c["output"][b, 0, 0, :len(crows[b])], crows[b]), b
    s.close()


def test_per_row_rates_every_row_is_its_row_at_that_rate():
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    st0[1] = 0                                                         # row 1: unpitched, at the native rate
    st1[1] = 0
    fi = int(s.meta("sample_rate") or 22050)
    rates = [8000, None, 48000]
    kw = dict(seeds=seeds, token_semitones=st0, token_semitones_end=st1, return_durations=True)
    alone = {}
    for r in rates:
        s.set_output_rate(r)
        alone[r] = s.synthesize_batch(ids, lens, scales, sid, **kw)
    s.set_output_rate(None)
    s.set_output_rates(rates)
    m = s.synthesize_batch(ids, lens, scales, sid, **kw)
    assert s.last_sample_rates().tolist() == [8000, fi, 48000]
    for b, r in enumerate(rates):
        N = int(alone[r]["sample_lengths"][b])
        assert m["sample_lengths"][b] == N and np.array_equal(m["token_spans"][b], alone[r]["token_spans"][b]), b
        assert np.array_equal(m["output"][b, 0, 0, :N], alone[r]["output"][b, 0, 0, :N]) and not m["output"][b, 0, 0, N:].any(), b
    assert m["output"].shape[-1] == max(int(m["sample_lengths"].max()), 1)
    # the constant-token kernel under per-row rates too
    s.set_output_rates([8000, 16000, None])
    w = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0)
    s.set_output_rates(None)
    s.set_output_rate(8000)
    w8 = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0)
    N = int(w8["sample_lengths"][0])
    assert np.array_equal(w["output"][0, 0, 0, :N], w8["output"][0, 0, 0, :N])
    s.set_output_rate(None)
    wn = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0)
    N = int(wn["sample_lengths"][2])
    assert w["sample_lengths"][2] == N and np.array_equal(w["output"][2, 0, 0, :N], wn["output"][2, 0, 0, :N])
    s.close()


def test_a_rate_outside_the_admitted_range_is_refused_and_the_previous_run_stays():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds, st0, _ = _inputs(s)
    fi = int(s.meta("sample_rate") or 22050)
    s.set_output_rate(8000)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0)
    s.set_output_rate(fi // 5)
    with pytest.raises(ses.SessionError, match=r"outside \[1/4, 4\]"):
        s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0)
    again = np.empty_like(r["output"])
    s._fetch(again, 0, 3)
    assert np.array_equal(again, r["output"]) and np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    s.close()


def test_delivery_on_top_of_a_pitched_run_at_8_khz():
    from phoonnx_amd.session import Segment
    s = _session("tiny_rb2_ms", output_rate=8000)
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    counts = r["sample_lengths"]
    segs = [delivery_ref.Seg(0, 0, 7, 1, 0.8), delivery_ref.Seg(1, 1, 0, 0, 1.0), delivery_ref.Seg(2, 1, 3, 2, 1.0)]
    for enc in ("pcm16", "ulaw"):
        want = delivery_ref.deliver_ref(r["output"][:, 0, 0], counts, segs, 2, enc)      # over the fetched 8 kHz waveform
        streams = s.deliver([Segment(*g) for g in segs], 2, enc)
        for j in range(2):
            assert np.ascontiguousarray(streams[j]).tobytes() == want[j], (enc, j)
        d = s.synthesize_delivered(ids, lens, scales, sid, seeds=seeds, segments=[Segment(*g) for g in segs], n_streams=2, encoding=enc,
                                   token_semitones=st0, token_semitones_end=st1, return_durations=True)
        assert np.array_equal(d["sample_lengths"], counts) and np.array_equal(d["token_spans"].sum(axis=1), counts)
        for j in range(2):
            assert np.ascontiguousarray(d["streams"][j]).tobytes() == want[j], (enc, j)
    pcm = s.last_pcm16(False, 1.0, shape=(3, int(counts.max())))
    for b in range(3):
        raw = delivery_ref.encode(delivery_ref.postprocess(r["output"][b, 0, 0, :counts[b]], None, 1.0), "pcm16")
        assert pcm[b, :counts[b]].tobytes() == raw and not pcm[b, counts[b]:].any()
    s.close()


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(s, **kw):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    n_vocab, n_spk = s.hparam("n_vocab"), s.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=s, config=cfg, phonemizer=_Phon(), dedupe_sentences=True, pitch_at_rate=True, **kw)


def test_the_voice_speaks_with_pitch_at_8_khz():
    from phoonnx_amd.config import SynthesisConfig
    text = "hello there. go"
    kw = dict(phoneme_pitch=-2, pitch_contour=[(0, 0), (1, 4)], sentence_silence=0.01)
    s = _session("tiny_rb2_ms")
    v = _voice(s, output_sample_rate=8000)
    out = v.synthesize_encoded(text, alignments=True, fade_in=0.005, fade_out=0.01, phoneme_gain_db=lambda k, toks: [-3.0] * len(toks), **kw)
    counts = s.last_sample_counts()
    assert s.last_sample_rates().tolist() == [8000] * len(counts)
    assert out.sentence_samples == [int(n) for n in counts] and np.array_equal(s.last_token_spans().sum(axis=1), counts)
    lead = int(8000 * 0.01 * 2) // 2
    for k, al in enumerate(out.phoneme_alignments):                    # the alignments tile each sentence, in delivered samples
        assert al[0].start_sample == out.sentence_starts[k] and sum(a.num_samples for a in al) == counts[k]
        assert all(a.start_sample + a.num_samples == b.start_sample for a, b in zip(al, al[1:]))
    assert len(out.data) == sum(lead + int(n) for n in counts)
    # The rate was folded in, not dropped: every token's step is 2^(st / 12) * 441 / 160 with st within [-2, 2] here, and a
    # token of the rendered frames ends at most one output sample past its share - N_b lies within n_b * 160 / 441 times
    # 2^(-+2/12), give or take a sample per token.
    n_b = s.last_y_lengths() * s.hparam("hop")
    T = s.last_token_spans().shape[1]
    for b in range(len(counts)):
        mid = float(n_b[b]) * 160 / 441
        assert mid / 2 ** (2 / 12) - T <= counts[b] <= mid * 2 ** (2 / 12) + T, (b, counts[b], mid)
    s.close()
    # the stream, joined, is the same bytes (fresh sessions: the same point of their noise streams)
    cfg = SynthesisConfig(normalize_audio=False)
    s = _session("tiny_rb2_ms")
    want = np.ascontiguousarray(_voice(s, output_sample_rate=8000).synthesize_encoded(text, cfg, **kw).data).tobytes()
    s.close()
    for chunk_frames in (3, 64):
        s = _session("tiny_rb2_ms")
        got = b"".join(_voice(s, output_sample_rate=8000).stream_encoded(text, cfg, chunk_frames=chunk_frames, **kw))
        assert got == want, chunk_frames
        s.close()


def test_requests_at_their_own_rates_with_pitch():
    s = _session("tiny_rb2_ms")
    v = _voice(s)
    reqs = [("hello there", None), ("go on", None)]
    kw = dict(seeds=[5, 6], phoneme_pitch=3.0, pitch_contour=[(0, -2), (1, 2)], alignments=True)
    mixed = v.synthesize_requests_encoded(reqs, output_sample_rates=[8000, 48000], **kw)
    for k, rate in enumerate((8000, 48000)):
        alone = v.synthesize_requests_encoded(reqs, output_sample_rates=[rate, rate], **kw)
        assert np.ascontiguousarray(mixed[k].data).tobytes() == np.ascontiguousarray(alone[k].data).tobytes(), rate
        assert mixed[k].sample_rate == rate
        for j, al in enumerate(mixed[k].phoneme_alignments):
            assert sum(a.num_samples for a in al) == mixed[k].sentence_samples[j]
    assert abs(len(mixed[1].data) / len(mixed[0].data) / 6 - 1) < 1.0     # (different texts: only the order of magnitude)
    s.close()


@pytest.mark.parametrize("enc", ["pcm16", "ulaw"])
def test_shaped_limited_trimmed_delivery_of_a_pitched_8_khz_run_equals_the_host_reference(enc):
    """synthesize_delivered with fades, token_gain_db, limiter and trim_silence on top of a pitched run at 8 kHz against
    limit_ref.deliver_ref (delivery_ref / trim_ref / shape_ref / limit_ref) over the fetched buffer.  The per-token volume's
    breakpoints are derived HERE: token boundaries from the reference's folded plan of the run's durations (an unpitched row:
    the resampler's rule), the ramp in samples at the DELIVERED rate - a wrong ramp rate or wrong bounds from the folded spans
    changes the bytes."""
    import limit_ref
    import shape_ref
    import trim_ref
    from phoonnx_amd import session as ses
    s = _session("tiny_rb2_ms", output_rate=8000)
    hop, fi = s.hparam("hop"), int(s.meta("sample_rate") or 22050)
    L, M = ref.ratio(fi, 8000)
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    st0[1] = 0                                                         # row 1 unpitched: its token bounds follow the resampler's rule
    st1[1] = 0
    kw = dict(seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    r = s.synthesize_batch(ids, lens, scales, sid, return_durations=True, **kw)
    x = r["output"][:, 0, 0, :].copy()
    counts = np.asarray(r["sample_lengths"], np.int64)
    db = np.random.default_rng(3).choice([0.0, 0.0, -6.0, 3.0, -np.inf, -40.0], (3, 40))
    gains = ses.token_gains(db, *db.shape)
    ramp = int(8000 * 0.004)
    assert s.delivered_rate == 8000 and ramp == 32
    segs = [delivery_ref.Seg(2, 0, 5, 2, 0.5), delivery_ref.Seg(0, 0, 5, 2, 0.5), delivery_ref.Seg(1, 1, 3, 0, 2.5)]
    trims = [trim_ref.Trim(2, 0.5, 3, 5, 4), trim_ref.Trim(2, 0.5, 3, 5, 4), trim_ref.Trim(0, 0.0, 0, 0, 7)]
    fades = [ses.Shape(40, 80, "smooth"), ses.Shape(), ses.Shape(0, 100, "linear")]
    limits = [limit_ref.Limit(0.3, 40), limit_ref.Limit(0.3, 7), limit_ref.Limit(0.5, 110)]
    d = s.synthesize_delivered(ids, lens, scales, sid, segments=[ses.Segment(*g) for g in segs], n_streams=2, encoding=enc,
                               trim=[ses.Trim(*t) for t in trims], shapes=fades, token_gain_db=db, gain_ramp=0.004,
                               limits=[ses.Limit(float(l.ceiling), int(l.lookahead)) for l in limits], return_durations=True, **kw)
    assert np.array_equal(d["durations"], r["durations"]) and np.array_equal(d["sample_lengths"], counts)
    # the breakpoints, from the reference's plan of this run's durations
    mine = []
    for g, fade in zip(segs, fades):
        b = g.row
        D = r["durations"][b, :lens[b]]
        if st0[b, :lens[b]].any() or st1[b, :lens[b]].any():
            spans = ref.glide_plan(D, st0[b, :lens[b]], st1[b, :lens[b]], hop, L, M)[1]
        else:
            spans = ref.identity_spans(D, hop, L, M, int(r["y_lengths"][b]) * hop)[0]
        assert int(spans.sum()) == counts[b]
        bounds = np.concatenate([[0], np.cumsum(spans), np.full(40 - lens[b], counts[b])]).astype(np.int64)
        points = ses.token_envelope(bounds, gains[b], ramp)
        mine.append(shape_ref.Shape(fade.fade_in, fade.fade_out, {"linear": 0, "smooth": 1}[fade.curve], tuple(points)))
    assert [list(sh.points) for sh in d["shapes"]] == [list(sh.points) for sh in mine]
    assert sum(len(sh.points) > 4 for sh in mine) >= 2
    want, kept, vals = limit_ref.deliver_ref(x, counts, segs, trims, None, mine, limits, 2, enc)
    assert d["kept_first"].tolist() == [a for a, _ in kept] and d["kept_count"].tolist() == [c for _, c in kept]
    assert any(a > 0 for a, _ in kept), "nothing was trimmed"
    for j in range(2):
        assert np.ascontiguousarray(d["streams"][j]).tobytes() == want[j], (enc, j)
    # every part worked: the bytes differ from the delivery without limiter, and from the one without shapes
    segments = [ses.Segment(*g) for g in segs]
    unshaped = s.deliver(segments, 2, enc, trims=[ses.Trim(*t) for t in trims])
    unlimited = s.deliver(segments, 2, enc, trims=[ses.Trim(*t) for t in trims], shapes=d["shapes"])
    have = [np.ascontiguousarray(a).tobytes() for a in d["streams"]]
    assert [np.ascontiguousarray(a).tobytes() for a in unshaped] != have
    assert [np.ascontiguousarray(a).tobytes() for a in unlimited] != have
    s.close()


def test_the_extreme_admitted_record_by_value():
    """32000 -> 8000 at +12 semitones: step = 8 ONE, c = 6963, Kh = 151 - the outermost taps' table index passes Z * R and gets
    weight 0 from warp_sample's guard - through both kernels, and beside it the other end, 8000 -> 32000 at -12 (step ONE / 8)"""
    from phoonnx_amd import session as ses
    rng = np.random.default_rng(151)
    x = rng.uniform(-1, 1, (2, 2400)).astype(np.float32)
    counts = np.array([2400, 300], np.int64)
    x[1, 300:] = 1000.0
    fis, fos = [32000, 8000], [8000, 32000]
    rows = [([300, 300], [12, 12]), ([75], [-12])]
    plans = [ses.warp_plan_rate(D, st, HOP, *ref.ratio(fi, fo)) for (D, st), fi, fo in zip(rows, fis, fos)]
    want = [ref.plan(D, st, HOP, *ref.ratio(fi, fo)) for (D, st), fi, fo in zip(rows, fis, fos)]
    assert (want[0][0][0].step, want[0][0][0].c, want[0][0][0].Kh) == (8 * ref.ONE, 6963, 151) and want[1][0][0].step == ref.ONE // 8
    assert want[0][2] == 300 and want[1][2] == 2400                    # more than one tile either way
    gplans = [ses.glide_plan_rate(D, st, st, HOP, *ref.ratio(fi, fo)) for (D, st), fi, fo in zip(rows, fis, fos)]
    yw, N = ses.test_warp_rate(x, counts, [p[0] for p in plans], fis, fos)
    yg, _ = ses.test_glide_rate(x, counts, [p[0] for p in gplans], fis, fos)
    assert np.array_equal(yw, yg)                                      # equal ends: the glide kernel renders the warp's bits
    for b in range(2):
        segs, _, n = want[b]
        assert [warp_ref.Seg(g.n0, g.pos0, g.step, g.c, g.half_taps, g.k) for g in plans[b][0]] == segs and N[b] == n
        w64 = ref.warp64(x[b, :counts[b]], segs, n)
        tol = ref.tolerance(segs, 1.0)
        err = float(np.abs(yw[b, :n] - w64).max())
        print(f"row {b}: Kh = {segs[0].Kh}, N = {n}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol and not yw[b, n:].any() and np.abs(w64).max() > 0.1
