"""Pitch contours on the GPU (include/vitsmi.h, "pitch contours"): glide_kernel by value through vits_test_glide, on one batch
with a row for each way it can go wrong; then vits_run_async_glided end to end through MiSession, the delivery on top of a
glided run, the refusals, and TTSVoice.synthesize_encoded(pitch_contour=).

Reference: tests/glide_ref.py (the definition in float64 and Python integers) applied to the native waveform of the same
run; the bound is glide_ref.tolerance, derived in warp_ref.tolerance with the gain bound measured over every cutoff."""
import os

import numpy as np
import pytest

import delivery_ref
import glide_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

S, HOP = 6000, 4
COUNTS = np.array([5800, 5800, 2400, 3000, 1301, 0, 1000, 900, 1000], np.int64)
B = len(COUNTS)


def _batch():
    """(x [B, S], per row (D, st0, st1, hop)):
    0  one long token -12 -> +12: the cutoff and the half-taps change from lane to lane, Kh from 19 to 38
    1  one long token +12 -> -12
    2  600 one-frame tokens with alternating glides: a tile straddles dozens of segments
    3  constant non-unit tokens: the warp's own records, bit for bit what test_warp gives for them
    4  an identity row: a masked copy
    5  a row with segments and no valid sample
    6  a row whose N is neither a multiple of 256 nor the batch's S_w
    7  a row whose valid samples end before its plan does: the taps are masked to [0, n_b)
    8  one- and two-frame tokens planned at hop 1, fast ones among them: records with k == 0 (at hop 4 the overshoot, under
       two samples, never reaches the next boundary four samples on, so such records need a smaller hop)"""
    rng = np.random.default_rng(47)
    x = rng.uniform(-1, 1, (B, S)).astype(np.float32)
    for b in range(B):
        x[b, COUNTS[b]:] = 1000.0                                    # what lies behind a row's valid samples must not show
    alt = [(12, 3), (-12, 7), (0, 12), (5, -5)]
    d8 = rng.integers(1, 3, 460).tolist()
    rows = [
        ([1450], [-12], [12], HOP),
        ([1450], [12], [-12], HOP),
        ([1] * 600, [alt[t % 4][0] for t in range(600)], [alt[t % 4][1] for t in range(600)], HOP),
        ([100, 0, 250, 7, 393], [3, 0, -7, 12, -0.5], [3, 0, -7, 12, -0.5], HOP),
        ([300, 0, 25], [0, 0, 0], [0, 0, 0], HOP),
        ([2, 3], [3, -2], [1, 4], HOP),
        ([90, 160], [-3, 4], [4, 0], HOP),
        ([150, 150], [2, -2], [-2, 6], HOP),
        (d8, rng.choice([12, 12, 7, -12], 460).tolist(), rng.choice([12, 3, -12], 460).tolist(), 1),
    ]
    assert sum(d8) <= COUNTS[8]
    return x, rows


_CACHE = {}


def _by_value():
    """the batch through the hook and through the reference, once"""
    if not _CACHE:
        from phoonnx_amd import session as ses
        x, rows = _batch()
        plans = [ses.glide_plan(D, st0, st1, hop) for D, st0, st1, hop in rows]
        rplans = [ref.plan(D, st0, st1, hop) for D, st0, st1, hop in rows]
        for (segs, spans, N), (rsegs, rspans, rN) in zip(plans, rplans):
            assert [ref.Seg(g.n0, g.pos0, g.k, g.step0, g.step1) for g in segs] == rsegs and N == rN
        y = ses.test_glide(x, COUNTS, [p[0] for p in plans])
        want = [ref.glide64(x[b, :COUNTS[b]], rplans[b][0], rplans[b][2]) for b in range(B)]
        _CACHE.update(x=x, rows=rows, plans=plans, rplans=rplans, y=y, want=want)
        y.setflags(write=False)
    return _CACHE


def test_the_batch_covers_what_it_claims():
    c = _by_value()
    N = [p[2] for p in c["rplans"]]
    assert c["y"].shape == (B, max(N)) and N[0] == N[1] == max(N) > 4096
    assert ref.max_half(c["rplans"][0][0]) == 38 and ref.cutoff(c["rplans"][0][0][0].step0)[1] == 19
    segs2 = c["rplans"][2][0]
    assert len(segs2) == 600 and max(g.k for g in segs2) <= 8          # a tile of 256 outputs straddles 32 segments and more
    assert all(g.step0 == g.step1 != ref.ONE for g in c["rplans"][3][0])
    assert ref.identity(c["rplans"][4][0]) and N[4] == 1300 and COUNTS[4] == 1301
    assert N[6] % 256 and N[6] != max(N) and N[7] % 256
    end7 = ref.pos_at(c["rplans"][7][0][-1], c["rplans"][7][0][-1].k) >> ref.FB
    assert end7 > COUNTS[7] + 100                                      # the plan reaches past the valid samples
    assert sum(1 for g in c["rplans"][8][0] if g.k == 0) >= 5          # several records without an output sample


def test_every_sample_is_within_the_tolerance_of_the_definition():
    c = _by_value()
    for b in range(B):
        segs, _, N = c["rplans"][b]
        tol = ref.tolerance(segs, float(np.abs(c["x"][b, :COUNTS[b]]).max()) if COUNTS[b] else 0.0)
        err = float(np.abs(c["y"][b, :N] - c["want"][b]).max()) if N else 0.0
        print(f"row {b}: N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (b, err, tol)
        assert np.abs(c["want"][b]).max() > 0.1 or b == 5              # (the rows that carry signal carry it)


def test_constant_tokens_are_the_warp_kernels_bits():
    from phoonnx_amd import session as ses
    c = _by_value()
    D, st, _, hop = c["rows"][3]
    wsegs, _, wN = ses.warp_plan(D, st, hop)
    assert wN == c["rplans"][3][2]
    y = ses.test_warp(c["x"][3:4], COUNTS[3:4], [wsegs])
    assert np.array_equal(y[0, :wN], c["y"][3, :wN])


def test_identity_rows_and_tails_are_exact():
    c = _by_value()
    y, x = c["y"], c["x"]
    assert np.array_equal(y[4, :1300], x[4, :1300]) and not y[4, 1300:].any()   # a masked copy, N < n_b here
    assert not y[5].any()                                                        # no valid input sample: zeros
    assert not np.isnan(y).any()                                                 # every column was written
    for b in range(B):
        assert not y[b, c["rplans"][b][2]:].any(), b                             # exact zeros behind every N_b
    # taps masked to [0, n_b): what lies behind row 7's 900 valid samples (1000.0) never shows
    assert float(np.abs(y[7]).max()) < 4.0


def test_a_row_alone_is_its_row_in_the_batch():
    from phoonnx_amd import session as ses
    c = _by_value()
    for b in range(B):
        N = c["rplans"][b][2]
        alone = ses.test_glide(c["x"][b:b + 1], COUNTS[b:b + 1], [c["plans"][b][0]])
        assert alone.shape == (1, max(1, N)) and np.array_equal(alone[0, :N], c["y"][b, :N]), b


def test_records_that_do_not_continue_their_row_are_refused():
    from phoonnx_amd import _ffi, session as ses
    c = _by_value()
    segs = list(c["plans"][3][0])

    def seg(g, **kw):
        f = dict(n0=g.n0, pos0=g.pos0, k=g.k, step0=g.step0, step1=g.step1)
        f.update(kw)
        return _ffi.VitsGlideSeg(f["n0"], f["pos0"], f["k"], f["step0"], f["step1"])

    for bad in (seg(segs[1], pos0=segs[1].pos0 - 65536), seg(segs[1], n0=segs[1].n0 + 1), seg(segs[1], step1=3 * ref.ONE),
                seg(segs[1], k=(1 << 23) + 1)):
        with pytest.raises(ses.SessionError, match="row 1: segment 1"):
            ses.test_glide(c["x"][:2], COUNTS[:2], [list(c["plans"][0][0]), [segs[0], bad] + segs[2:]])
    # a glide's next record starts at the closed form's pos_k, not at pos0 + k * step0
    g = c["plans"][0][0][0]
    after = _ffi.VitsGlideSeg(g.n0 + g.k, g.pos0 + g.k * g.step0, 0, ref.ONE, ref.ONE)
    with pytest.raises(ses.SessionError, match="row 0: segment 1"):
        ses.test_glide(c["x"][:1], COUNTS[:1], [[g, after]])


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
    st0, st1 = np.zeros((3, 40), np.float32), np.zeros((3, 40), np.float32)
    p0 = np.array([0, 3, -4, 7, -12, 12, 0.5, 2], np.float32)
    p1 = np.array([3, -4, -4, -12, 12, 0, 0.5, -1], np.float32)         # glides up, down, across the range, and constant tokens
    for b in range(3):
        st0[b, :lens[b]] = np.resize(np.roll(p0, b), lens[b])
        st1[b, :lens[b]] = np.resize(np.roll(p1, b), lens[b])
    st0[:, 39] = 99.0                                                  # behind lens of rows 1 and 2: ignored ...
    st0[0, 39] = 2.0                                                   # ... a token of row 0
    st1[1:, 38] = -99.0
    return ids, lens, scales, sid, np.array([101, 202, 303], np.uint64), st0, st1


def _rates(st0, st1, lens):
    from phoonnx_amd import session as ses
    rate = np.ones(st0.shape, np.float32)
    for b in range(len(lens)):
        for t in range(int(lens[b])):
            rate[b, t] = ses.glide_token(st0[b, t], st1[b, t])[2]
    return rate


@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms"])
def test_a_compensated_run_is_the_rate_scaled_run_glided(preset):
    s = _session(preset)
    hop = s.hparam("hop")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    rate = _rates(st0, st1, lens)
    free = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    base = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_rate=rate, return_durations=True)
    native = base["output"][:, 0, 0].copy()
    launches = s.stats()["total_launches"]
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=st1, compensate=True,
                           return_durations=True)
    assert s.stats()["total_launches"] == launches + 1                 # the one glide launch on top
    assert np.array_equal(r["durations"], base["durations"]) and np.array_equal(r["y_lengths"], base["y_lengths"])
    plans = [ref.plan(base["durations"][b, :lens[b]], st0[b, :lens[b]], st1[b, :lens[b]], hop) for b in range(3)]
    assert r["sample_lengths"].tolist() == [p[2] for p in plans]
    assert np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    assert r["output"].shape == (3, 1, 1, max(p[2] for p in plans))
    for b in range(3):
        segs, spans, N = plans[b]
        n_b = int(base["y_lengths"][b]) * hop
        want = ref.glide64(native[b, :n_b], segs, N)
        tol = ref.tolerance(segs, float(np.abs(native[b, :n_b]).max()))
        got = r["output"][b, 0, 0]
        err = float(np.abs(got[:N] - want).max())
        print(f"{preset} row {b}: n_b = {n_b}, N = {N}, max |gpu - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol and not got[N:].any(), (b, err, tol)
        assert np.array_equal(r["token_spans"][b, :lens[b]], spans) and not r["token_spans"][b, lens[b]:].any()
        # The tempo is kept, token by token.  With w the token's predicted length in frames, the free run renders
        # D = ceil(w) and the compensated one D' = ceil(w * r), r = (float)((r0 + r1) / 2): D' < r * D + 1 and
        # D' > r * (D - 1).  The plan measures L from where the row really is - up to 0.75 sample short of, or under 2 past,
        # the boundary before -, so D' * hop - 2 < L <= D' * hop + 0.75, and k = ceil(L / rbar) with the mean step rbar
        # = (a + b) / 2 = r up to the steps' rounding, rbar >= 1/2.  Hence
        #   k < (r * D * hop + hop + 0.75) / rbar + 1 <= D * hop + 2 * hop + 2.5   and
        #   k > (r * (D - 1) * hop - 2) / rbar       >= D * hop - hop - 4,
        # and with k an integer and hop >= 2: |k - D * hop| <= 2 * hop + 2.
        D = free["durations"][b, :lens[b]]
        assert hop >= 2 and np.abs(spans - D * hop).max() <= 2 * hop + 2, (b, np.abs(spans - D * hop).max())
    assert np.array_equal(s.last_token_spans(), r["token_spans"])
    # the pure glide: ctl untouched - the free run's durations, its waveform glided
    pure = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=st1, compensate=False,
                              return_durations=True)
    assert np.array_equal(pure["durations"], free["durations"])
    for b in range(3):
        segs, spans, N = ref.plan(free["durations"][b, :lens[b]], st0[b, :lens[b]], st1[b, :lens[b]], hop)
        n_b = int(free["y_lengths"][b]) * hop
        x = free["output"][b, 0, 0, :n_b]
        assert pure["sample_lengths"][b] == N
        assert float(np.abs(pure["output"][b, 0, 0, :N] - ref.glide64(x, segs, N)).max()) <= ref.tolerance(segs, float(np.abs(x).max()))
    s.close()


def test_equal_ends_are_the_warped_run_and_zeros_the_unwarped_one():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, st0, _ = _inputs(s)
    w = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, return_durations=True)
    per_warped = s.stats()["total_launches"]                           # (the launches of the last run)
    same = st0.copy()
    same[1, 30] = 5.0                                                  # behind lens[1]: ignored - the ends stay equal
    g = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=same, return_durations=True)
    assert s.stats()["total_launches"] == per_warped                   # the same launches: warp_kernel served it
    for key in ("output", "durations", "y_lengths", "sample_lengths", "token_spans"):
        assert np.array_equal(g[key], w[key]), key
    # all zeros - given as zeros, or as end values alone -: the unwarped run
    base = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
    per_plain = s.stats()["total_launches"]
    assert per_plain == per_warped - 1
    zero = np.zeros((3, 40), np.float32)
    zero[1, 30] = 5.0
    for kw in ({"token_semitones": zero, "token_semitones_end": zero.copy()}, {"token_semitones_end": zero}):
        r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True, **kw)
        assert s.stats()["total_launches"] == per_plain                # no warp was planned or launched
        assert np.array_equal(r["output"], base["output"]) and np.array_equal(r["durations"], base["durations"])
        assert np.array_equal(r["sample_lengths"], base["y_lengths"] * s.hparam("hop"))
        assert np.array_equal(r["token_spans"], base["durations"] * s.hparam("hop"))
        with pytest.raises(ses.SessionError, match="not warped"):
            s.last_token_spans()
    s.close()


def test_delivery_on_top_of_a_glided_run():
    from phoonnx_amd.session import Segment
    s = _session("tiny_rb2_ms")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    r = s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    counts = r["sample_lengths"]
    segs = [delivery_ref.Seg(0, 0, 7, 1, 0.8), delivery_ref.Seg(1, 1, 0, 0, 1.0), delivery_ref.Seg(2, 1, 3, 2, 1.0)]
    want = delivery_ref.deliver_ref(r["output"][:, 0, 0], counts, segs, 2, "pcm16")   # over the fetched glided waveform
    streams = s.deliver([Segment(*g) for g in segs], 2, "pcm16")
    for j in range(2):
        assert np.ascontiguousarray(streams[j]).tobytes() == want[j], j
    # ... and in one call: the same bytes, with the glide's counts and spans
    d = s.synthesize_delivered(ids, lens, scales, sid, seeds=seeds, segments=[Segment(*g) for g in segs], n_streams=2,
                               token_semitones=st0, token_semitones_end=st1, return_durations=True)
    assert np.array_equal(d["sample_lengths"], counts) and np.array_equal(d["token_spans"].sum(axis=1), counts)
    for j in range(2):
        assert np.ascontiguousarray(d["streams"][j]).tobytes() == want[j], j
    # the 16-bit rendering works on the glided buffer too
    pcm = s.last_pcm16(False, 1.0, shape=(3, int(counts.max())))
    for b in range(3):
        raw = delivery_ref.encode(delivery_ref.postprocess(r["output"][b, 0, 0, :counts[b]], None, 1.0), "pcm16")
        assert pcm[b, :counts[b]].tobytes() == raw and not pcm[b, counts[b]:].any()
    s.close()


def test_refusals_leave_the_previous_run_readable():
    from phoonnx_amd import session as ses
    s = _session("tiny_rb1")
    ids, lens, scales, sid, seeds, st0, st1 = _inputs(s)
    kw = dict(seeds=seeds, token_semitones=st0, token_semitones_end=st1)
    r = s.synthesize_batch(ids, lens, scales, sid, return_durations=True, **kw)
    s.set_output_rate(8000)
    with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, sid, **kw)
    s.set_output_rate(None)
    s.set_output_rates([8000, 0, 16000])
    with pytest.raises(ses.SessionError, match="not covered with an output rate set"):
        s.synthesize_batch(ids, lens, scales, sid, **kw)
    s.set_output_rates(None)
    bad = st1.copy()
    bad[2, 3] = -13.0
    with pytest.raises(ses.SessionError, match=r"token_semitones_end\[2,3\]"):
        s.synthesize_batch(ids, lens, scales, sid, seeds=seeds, token_semitones=st0, token_semitones_end=bad)
    with pytest.raises(ses.SessionError, match="forced durations are the rendered ones"):
        s.synthesize_batch(ids, lens, scales, sid, durations=r["durations"], **kw)
    again = np.empty_like(r["output"])
    s._fetch(again, 0, 3)                                              # the glided run is still there
    assert np.array_equal(again, r["output"]) and np.array_equal(s.last_sample_counts(), r["sample_lengths"])
    assert np.array_equal(s.last_token_spans(), r["token_spans"])
    s.close()


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(s):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    n_vocab, n_spk = s.hparam("n_vocab"), s.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=s, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


def test_synthesize_encoded_with_a_pitch_contour():
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.session import Segment
    from phoonnx_amd.sharding import pad_batch
    text = "hello there. go"
    s = _session("tiny_rb2_ms")
    v = _voice(s)
    out = v.synthesize_encoded(text, alignments=True, pitch_contour=[(0, 0), (1, 4)], sentence_silence=0.01)
    counts = s.last_sample_counts()
    assert out.sentence_samples == [int(n) for n in counts] and np.array_equal(s.last_token_spans().sum(axis=1), counts)
    lead = int(22050 * 0.01 * 2) // 2
    for k, al in enumerate(out.phoneme_alignments):                    # the alignments tile each sentence
        assert al[0].start_sample == out.sentence_starts[k] and sum(a.num_samples for a in al) == counts[k]
        assert all(a.start_sample + a.num_samples == b.start_sample for a, b in zip(al, al[1:]))
        assert al[-1].start_sample + al[-1].num_samples == out.sentence_starts[k] + counts[k]
    assert out.sentence_starts[0] == lead and len(out.data) == sum(lead + int(n) for n in counts)
    s.close()
    # the session-level call with the arrays tests/test_glide_cpu.py pins, on a fresh session at the same point of its noise
    # stream: the same bytes
    s = _session("tiny_rb2_ms")
    v = _voice(s)
    cfg = SynthesisConfig()
    groups = v._sentence_groups(text, cfg)
    ids, lens = pad_batch([[i for _, g in grp for i in g] for grp in groups])
    st0, st1 = np.zeros(ids.shape), np.zeros(ids.shape)
    for b, grp in enumerate(groups):
        a, e = ref.contour_ids([len(g) for _, g in grp], lambda x: 4.0 * x)
        st0[b, :len(a)], st1[b, :len(e)] = a, e
    assert st1.max() == 4.0 and st0.min() == 0.0
    sid = np.full((len(groups),), cfg.speaker_id or 0, np.int64) if "sid" in [i.name for i in s.get_inputs()] else None
    norm = 1 if cfg.normalize_audio else 0
    d = s.synthesize_delivered(ids, lens, v._scales(cfg), sid, segments=[Segment(b, 0, lead, norm, float(cfg.volume)) for b in range(len(groups))],
                               n_streams=1, encoding="pcm16", token_semitones=st0, token_semitones_end=st1)
    assert np.ascontiguousarray(d["streams"][0]).tobytes() == np.ascontiguousarray(out.data).tobytes()
    s.close()
