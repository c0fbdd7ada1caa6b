"""A rate per row on the GPU (include/vitsmi.h, "output rate per row"): resample_rows_kernel by value through
vits_test_resample_rows, and the feature end to end through MiSession and TTSVoice.

What a row of a mixed-rate run must be is already defined: the same row under vits_set_output_rate at its rate.  So the first
reference is the engine's own single-rate entry, held with array_equal.  The second is the float64 NumPy evaluation of the
definition (tests/resample_ref.py), within its derived bound (K + 2) * 2^-24 * max_p sum_j |h[p][j]| * max|x|."""
import os

import numpy as np
import pytest

import resample_ref as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the kernel by value

def _rows_input(lens, S, seed):
    """x [B, S]: noise on each row's valid samples, non-zero garbage behind them - which must not show"""
    rng = np.random.default_rng(seed)
    x = np.zeros((len(lens), S), np.float32)
    for b, n in enumerate(lens):
        n = int(n)
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
        x[b, n:] = 1000.0 + rng.standard_normal(S - n).astype(np.float32)
    return x


def _check_mixed(x, lens, fi, rates, what):
    """the three checks of a mixed launch: each resampled row against the single-rate entry on that row alone (array_equal)
    and against the float64 definition (derived bound); each native row against its input; zeros behind every row's end"""
    from phoonnx_amd.session import test_resample, test_resample_rows
    y, counts = test_resample_rows(x, lens, fi, rates)
    B = len(lens)
    assert not np.isnan(y).any(), "a column of y was not written"
    assert y.shape == (B, max(1, int(counts.max())))
    for b in range(B):
        n, N, fo = int(lens[b]), int(counts[b]), int(rates[b] or 0)
        assert not y[b, N:].any(), (what, b, "samples behind N_b are not exactly 0.0")
        if fo in (0, fi):
            assert N == n and np.array_equal(y[b, :N], x[b, :n]), (what, b, "a native row is not its input")
            continue
        assert N == int(ref.count(n, fi, fo))
        alone, c1 = test_resample(x[b:b + 1], lens[b:b + 1], fi, fo)
        assert int(c1[0]) == N and np.array_equal(y[b, :N], alone[0, :N]), (what, b, "differs from the single-rate entry")
        if not N:
            continue
        want = ref.resample64(x[b, :n], fi, fo)
        tol = ref.tolerance(fi, fo, np.abs(x[b, :n]).max())
        err = float(np.abs(y[b, :N].astype(np.float64) - want).max())
        print(f"{what} {fi}->{fo} row {b}: n={n} N={N} max|err|={err:.3e} tol={tol:.3e}")
        assert err <= tol, (what, b, err, tol)
    return y, counts


def test_kernel_by_value():
    """B = 6, S = 1500 at 22050 Hz: a row of two output tiles and more, a native row, a row shorter than its filter, an empty
    row, a row at the input rate, and the row whose every output sees both edges (K / 2 - 1 samples)"""
    fi, S = 22050, 1500
    K = ref.plan(fi, 8000)[2]
    rates = [8000, 0, 48000, 16000, 22050, 8000]
    lens = np.array([1500, 513, 37, 0, 1500, K // 2 - 1], np.int64)
    y, counts = _check_mixed(_rows_input(lens, S, 7), lens, fi, rates, "mixed")
    assert int(counts[0]) > 256 and int(counts[3]) == 0 and y.shape[1] == 1500     # row 0: more than one tile; S_out = max N_b


def test_a_launch_that_mixes_a_staged_and_an_unstaged_row():
    """384000 -> 1000 Hz has K = 14458: the span of a tile is above what a workgroup may stage (16000 floats), so that row
    reads its input through the caches, next to a staged row (-> 192000 Hz) and a native one, in ONE launch"""
    fi, S = 384000, 20000
    L, M, K = ref.plan(fi, 1000)[:3]
    assert 63 * M // L + 2 + K == 38652 > 16000
    lens = np.array([20000, 19001, 777], np.int64)
    _check_mixed(_rows_input(lens, S, 8), lens, fi, [1000, 192000, 0], "staged+unstaged")


def test_all_rows_at_one_rate_and_refusals_of_the_hook():
    from phoonnx_amd.session import SessionError, test_resample, test_resample_rows
    fi, S = 22050, 700
    lens = np.array([700, 300, 0], np.int64)
    x = _rows_input(lens, S, 9)
    y, counts = test_resample_rows(x, lens, fi, [16000] * 3)
    want, wc = test_resample(x, lens, fi, 16000)
    assert np.array_equal(counts, wc) and np.array_equal(y, want)
    with pytest.raises(SessionError, match=r"row 1\b.*400000"):
        test_resample_rows(x, lens, fi, [8000, 400000, 0])


# ------------------------------------------------------------------ end to end

RATES = [8000, 0, 48000, 16000]


def _session(preset, **kw):
    from phoonnx_amd import MiSession
    return MiSession(os.path.join(GOLDEN, preset + ".onnx"), **kw)


def _batch(s, per_token=None, seed=31):
    """four rows with their own settings and seeds (per_token: forced durations, for rows long enough to have a loudness)"""
    rng = np.random.default_rng(seed)
    lens = np.array([12, 9, 10, 7], np.int64)
    ids = np.zeros((4, 12), np.int64)
    for b in range(4):
        ids[b, :lens[b]] = rng.integers(1, s.hparam("n_vocab"), lens[b])
    sid = rng.integers(0, s.hparam("n_speakers"), 4).astype(np.int64) if s.hparam("n_speakers") > 1 else None
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 1.3, 0.6], [0.667, 0.9, 0.8], [0.3, 1.1, 0.5]], np.float32)
    kw = {"seeds": np.array([11, 22, 33, 44], np.uint64)}
    if per_token:
        kw["durations"] = np.where(np.arange(12)[None, :] < lens[:, None], per_token, 0).astype(np.int64)
    return (ids, lens, scales, sid), kw


def _fi(s):
    return int(s.meta("sample_rate") or 22050)


@pytest.mark.parametrize("tails", ["zero", "reference"])
@pytest.mark.parametrize("preset", ["tiny_rb1", "tiny_rb2_ms"])
def test_each_row_is_that_row_at_its_rate_alone(preset, tails):
    s = _session(preset, tails=tails)
    fi, hop = _fi(s), s.hparam("hop")
    args, kw = _batch(s)
    s.set_output_rates(RATES)
    r = s.synthesize_batch(*args, **kw)
    counts = r["sample_lengths"]
    assert np.array_equal(r["sample_rates"], [8000, fi, 48000, 16000]) and np.array_equal(s.last_sample_rates(), r["sample_rates"])
    assert np.array_equal(counts, s.last_sample_counts())
    assert np.array_equal(counts, [ref.count(int(n) * hop, fi, fo or fi) if fo else int(n) * hop for n, fo in zip(r["y_lengths"], RATES)])
    assert r["output"].shape == (4, 1, 1, int(counts.max()))
    pcm = s.last_pcm16(True, 0.9, shape=(4, int(counts.max())))
    for b, fo in enumerate(RATES):
        s.set_output_rate(fo or None)
        assert s.output_rates is None
        one = s.synthesize_batch(*args, **kw)
        n = one["sample_lengths"] if fo else one["y_lengths"] * hop
        N = int(n[b])
        assert N == int(counts[b]) and np.array_equal(one["y_lengths"], r["y_lengths"])
        assert np.array_equal(r["output"][b, 0, 0, :N], one["output"][b, 0, 0, :N]), (b, fo)
        assert not r["output"][b, 0, 0, N:].any(), (b, "samples behind N_b are not zero")
        assert np.array_equal(s.last_sample_rates(), [fo or fi] * 4)
        one_pcm = s.last_pcm16(True, 0.9, shape=(4, one["output"].shape[3]))
        assert np.array_equal(pcm[b, :N], one_pcm[b, :N]) and not pcm[b, N:].any(), (b, fo)
    s.close()


def test_uniform_rows_are_the_handle_rate_and_native_rows_the_native_path():
    s = _session("tiny_rb1")
    fi = _fi(s)
    args, kw = _batch(s)
    s.set_timing(True)
    native = s.synthesize_batch(*args, **kw)
    launches = s.stats()["total_launches"]
    kernels = [r["kernel"] for r in s.launch_records()]
    s.set_output_rate(8000)
    want = s.synthesize_batch(*args, **kw)
    assert s.stats()["total_launches"] == launches + 2         # the counts kernel and the resampler
    s.set_output_rates([8000] * 4)
    got = s.synthesize_batch(*args, **kw)
    assert np.array_equal(got["output"], want["output"]) and np.array_equal(got["sample_lengths"], want["sample_lengths"])
    assert s.stats()["total_launches"] == launches + 2
    # every row native: nothing is launched behind the generator, and the result is the native run's
    s.set_output_rates([0, fi, None, 0])
    same = s.synthesize_batch(*args, **kw)
    assert s.stats()["total_launches"] == launches and [r["kernel"] for r in s.launch_records()] == kernels
    assert np.array_equal(same["output"], native["output"]) and np.array_equal(same["sample_rates"], [fi] * 4)
    assert np.array_equal(same["sample_lengths"], native["y_lengths"] * s.hparam("hop"))
    # output_rates= of one call: set for it, and what was set before is back afterwards
    s.set_output_rate(16000)
    r = s.synthesize_batch(*args, output_rates=[8000] * 4, **kw)
    assert np.array_equal(r["output"], want["output"]) and s.output_rate == 16000 and s.output_rates is None
    assert s.synthesize_batch(*args, **kw)["output"].shape[3] == int(ref.count(native["y_lengths"].max() * s.hparam("hop"), fi, 16000))
    s.set_output_rates([8000, 0, 0, 0])
    s.synthesize_batch(*args, output_rates=[0] * 4, **kw)
    assert s.output_rates == (8000, 0, 0, 0) and s.output_rate is None
    s.close()


def test_a_vocoder_run_with_row_rates():
    s = _session("tiny_rb1")
    rng = np.random.default_rng(5)
    z = rng.standard_normal((3, s.hparam("inter"), 23)).astype(np.float32)
    s.set_output_rates([8000, 0, 48000])
    y = s.vocoder(z)[:, 0, 0, :]
    N = [int(ref.count(23 * s.hparam("hop"), _fi(s), fo)) if fo else 23 * s.hparam("hop") for fo in (8000, 0, 48000)]
    assert y.shape == (3, max(N)) and np.array_equal(s.last_sample_rates(), [8000, _fi(s), 48000])
    for b, fo in enumerate((8000, None, 48000)):
        s.set_output_rate(fo)
        one = s.vocoder(z)[:, 0, 0, :]
        assert one.shape[1] == N[b] and np.array_equal(y[b, :N[b]], one[b]) and not y[b, N[b]:].any(), b
    s.close()


# ------------------------------------------------------------------ delivery

def _bytes(streams):
    return [a.tobytes() for a in streams]


def test_a_mixed_batch_delivered_once_per_rate():
    """rows 0 and 2 at 8 kHz as mu-law, rows 1 and 3 at the voice's rate as PCM16 - two calls on one run - are the bytes the
    single-rate sessions deliver; a levelled delivery must name the rate of its rows"""
    from phoonnx_amd.session import Level, Segment, SessionError, Trim
    s = _session("tiny_rb2_ms")
    fi = _fi(s)
    args, kw = _batch(s, per_token=40)
    tel = [Segment(2, 0, 5, 1, 0.8), Segment(0, 0, 0, 1, 0.8)]           # one stream: row 2, then row 0
    web = [Segment(1, 0, 0, 0, 0.5), Segment(3, 1, 7, 1, 1.0)]
    trims = [Trim(2, 0.05, 3, 5, 4), Trim(2, 0.05, 0, 0, 0)]
    levels = [Level(1, -20.0, 40.0, 0.9), Level(1, -23.0, 40.0, 0.0)]
    flat = [Segment(g.row, g.stream, g.lead_samples, 0, g.volume) for g in tel]     # (levelling replaces peak normalisation)

    def deliveries(rate_of_web):
        out = {"tel": _bytes(s.deliver(tel, 1, "ulaw"))} if rate_of_web is None else {"web": _bytes(s.deliver(web, 2, "pcm16"))}
        if rate_of_web is None:
            st, kf, kc, loud, gain = s.deliver(flat, 1, "ulaw", trims=trims, levels=levels, sample_rate=8000, return_kept=True,
                                               return_levels=True)
            out["lev"] = (_bytes(st), kf.tolist(), kc.tolist(), loud.tolist(), gain.tolist())
        return out

    s.set_output_rate(8000)
    s.synthesize_batch(*args, **kw)
    assert s.last_sample_counts().min() >= 0.5 * 8000, "the rows are too short to have a loudness"
    want = deliveries(None)
    s.set_output_rate(None)
    s.synthesize_batch(*args, **kw)
    want.update(deliveries(fi))
    s.set_output_rates([8000, 0, 8000, 0])
    s.synthesize_batch(*args, **kw)
    got = deliveries(None)
    got.update(deliveries(fi))
    assert got["tel"] == want["tel"] and got["web"] == want["web"]
    assert np.isfinite(got["lev"][3]).all() and got["lev"] == want["lev"]
    # a levelled delivery at a rate that is not its rows': refused, naming the segment and both rates; the run stays
    with pytest.raises(SessionError, match=rf"segment 0\b.*{fi}.*8000"):
        s.deliver(flat, 1, "ulaw", trims=trims, levels=levels, sample_rate=fi)
    both = [flat[0], Segment(1, 0, 0, 0, 1.0)]                               # a row at 8 kHz and a native one in one call
    with pytest.raises(SessionError, match=rf"segment 1\b.*8000.*{fi}"):
        s.deliver(both, 1, "ulaw", levels=levels, sample_rate=8000)
    assert _bytes(s.deliver(both, 1, "ulaw", levels=[levels[0], Level(0, 0.0, 0.0, 0.0)], sample_rate=8000))   # (unlevelled: any rate)
    assert _bytes(s.deliver(tel, 1, "ulaw")) == want["tel"]
    # run and grouped delivery in one call: an encoding per segment, one delivery per (rate, encoding)
    segs = [Segment(0, 0, 0, 1, 0.8), Segment(1, 1, 0, 0, 0.5), Segment(2, 2, 5, 1, 0.8), Segment(3, 3, 7, 1, 1.0)]
    d = s.synthesize_delivered(*args, segments=segs, n_streams=4, encoding=["ulaw", "pcm16", "ulaw", "pcm16"], **kw)
    assert [a.dtype for a in d["streams"]] == [np.uint8, np.int16, np.uint8, np.int16]
    assert np.array_equal(d["sample_rates"], [8000, fi, 8000, fi]) and np.array_equal(d["kept_count"], d["sample_lengths"])
    a = s.deliver([segs[0], segs[2]], 3, "ulaw")
    b = s.deliver([segs[1], segs[3]], 4, "pcm16")
    assert _bytes(d["streams"]) == [a[0].tobytes(), b[1].tobytes(), a[2].tobytes(), b[3].tobytes()]
    with pytest.raises(SessionError, match="stream 0"):
        s.synthesize_delivered(*args, segments=[Segment(0, 0), Segment(1, 0)], n_streams=1, **kw)
    s.close()


# ------------------------------------------------------------------ refusals

def test_what_row_rates_do_not_cover_is_refused_and_the_run_stays():
    from phoonnx_amd.session import Limit, Onset, Segment, SessionError, Shape
    s = _session("tiny_rb1")
    (ids, lens, scales, sid), kw = _batch(s)
    s.set_output_rates(RATES)
    s.synthesize_batch(ids, lens, scales, sid, **kw)
    segs = [Segment(b, b, 0, 1, 1.0) for b in range(4)]
    want = _bytes(s.deliver(segs, 4, "pcm16"))
    z = np.random.default_rng(3).standard_normal((4, s.hparam("inter"), 9)).astype(np.float32)
    three = dict(seeds=kw["seeds"][:3])
    refused = [
        ("B = 3.*named 4", lambda: s.synthesize_batch(ids[:3], lens[:3], scales[:3], None, **three)),
        ("B = 3.*named 4", lambda: s.vocoder(z[:3])),
        ("per-row output rates", lambda: list(s.synthesize_stream(ids, lens, scales, sid, chunk_frames=4, **kw))),
        ("per-row output rates", lambda: list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=4, encoding="ulaw", **kw))),
        ("per-row output rates", lambda: list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=4, shapes=Shape(8, 8, "linear"),
                                                                          limit=Limit(0.9, 16), **kw))),
        ("per-row output rates", lambda: list(s.synthesize_stream_encoded(ids, lens, scales, sid, chunk_frames=4, ref_peak=1.0,
                                                                          onsets=Onset(2, 0.01, 4), **kw))),
        ("per-row output rates", lambda: list(s.vocoder_stream(z, chunk_frames=4))),
        ("per-row output rates", lambda: list(s.vocoder_stream_encoded(z, chunk_frames=4, encoding="alaw"))),
        ("per-row output rates", lambda: s.run_device(0, 0, 4, 12, scales[0])),
        ("per-row output rates", lambda: s.run_device(0, 0, 4, 12, scales, seeds=kw["seeds"])),
    ]
    for match, call in refused:
        with pytest.raises(SessionError, match=match):
            call()
        assert _bytes(s.deliver(segs, 4, "pcm16")) == want, match     # the previous run is still deliverable
    s.close()


# ------------------------------------------------------------------ the voice layer

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(session, rate=None):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    n_vocab, n_spk = session.hparam("n_vocab"), session.hparam("n_speakers")
    cfg = VoiceConfig(num_symbols=n_vocab, num_speakers=n_spk, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i % (n_vocab - 1)] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True, output_sample_rate=rate)


@pytest.mark.parametrize("scope", [None, "sentence", "text"])
def test_every_request_is_what_a_voice_at_its_rate_and_encoding_returns(scope):
    """three callers in the same runs: telephony (8 kHz mu-law), the voice's own rate as PCM16, a browser (48 kHz float32).
    Batch composition does not depend on the rates, so every request equals the same call on a voice loaded at its rate."""
    import struct
    from phoonnx_amd.config import SynthesisConfig
    preset = "tiny_rb2_ms"
    norm = scope is None          # (levelling replaces peak normalisation)
    requests = [("the quick brown fox. jumps over", SynthesisConfig(speaker_id=1, volume=0.8, normalize_audio=norm, length_scale=16.0)),
                ("a lazy dog. sleeps all day. in the sun", SynthesisConfig(speaker_id=0, volume=1.0, normalize_audio=norm, length_scale=20.0)),
                ("hello there", SynthesisConfig(speaker_id=2, volume=1.2, normalize_audio=False, length_scale=18.0))]
    wants = [(8000, "ulaw"), (None, "pcm16"), (48000, "f32")]
    kw = dict(seeds=[5, 6, 7], max_batch=4, sentence_silence=0.013, alignments=True, trim_silence=0.02, trailing_silence=0.031,
              fade_in=0.004, fade_out=0.011, fade_curve="smooth", limit_ceiling=0.7, limit_lookahead=0.004,
              phoneme_gain_db=lambda k, tokens: [(-6.0 if t in "aeiou" else 0.0) - k for t in tokens])
    if scope:
        kw.update(loudness=-21.0, loudness_scope=scope, max_gain_db=40.0, peak_ceiling=0.9)
    mixed = _voice(_session(preset))
    got = mixed.synthesize_requests_encoded(requests, output_sample_rates=[w[0] for w in wants], encodings=[w[1] for w in wants], **kw)
    assert mixed.session.output_rates is None and mixed.session.output_rate is None         # (put back)
    mixed.session.close()
    for r, (rate, enc) in enumerate(wants):
        v = _voice(_session(preset), rate)
        want = v.synthesize_requests_encoded(requests, encoding=enc, **kw)[r]
        v.session.close()
        g = got[r]
        assert (g.sample_rate, g.encoding) == (rate or 22050, enc) == (want.sample_rate, want.encoding)
        assert g.sentence_starts == want.sentence_starts and g.sentence_samples == want.sentence_samples, r
        assert g.data.dtype == want.data.dtype and g.tobytes() == want.tobytes(), r
        assert g.wav_bytes() == want.wav_bytes()
        assert struct.unpack_from("<I", g.wav_bytes(), 24)[0] == (rate or 22050)          # the header's sample rate
        for ag, aw in zip(g.phoneme_alignments, want.phoneme_alignments):
            assert [(p.phoneme, p.start_sample, p.num_samples) for p in ag] == [(p.phoneme, p.start_sample, p.num_samples) for p in aw]
        if scope:
            print(f"request {r} at {g.sample_rate} Hz as {enc}, scope {scope}: loudness {g.loudness} gain {g.gain}")
            assert np.isfinite(g.loudness).all(), "the sentences are too short to have a loudness"
            assert g.loudness == want.loudness and g.gain == want.gain, (r, g.loudness, want.loudness)
