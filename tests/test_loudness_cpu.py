"""Levelled delivery (include/vitsmi.h, "levelled delivery") without a GPU: the K-weighting's coefficients, the gates, the gain
and the refusals through the library's pure host entries against tests/loudness_ref.py (float64); the NumPy fallback; the
workspace walk in a stand-alone driver; the voice layer on stub sessions."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import delivery_ref as dref
import loudness_ref as ref
import trim_ref as tref
from conftest import ROOT
from delivery_ref import COUNTS, GOOD, Seg
from loudness_ref import Level

from phoonnx_amd import _ffi
from phoonnx_amd import audio_encoding as ae
from phoonnx_amd import session as ses
from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
from phoonnx_amd.session import Segment, SessionError
from phoonnx_amd.voice import TTSVoice

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")


def _segs(segs):
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _levels(levels):
    return [ses.Level(*l) for l in levels]


# ------------------------------------------------------------------ coefficients

def test_the_filter_at_48_khz_is_the_table_of_bs1770():
    coef, hop = ses.loudness_filter(48000)
    got = [coef[0], coef[1], coef[2], coef[3], coef[4], coef[8], coef[9]]
    assert np.abs(np.array(got) - np.array(ref.BS1770_48K)).max() <= 1e-12
    assert coef[5:8].tolist() == [1.0, -2.0, 1.0] and hop == 4800


@pytest.mark.parametrize("rate, hop", [(22050, 2205), (8000, 800), (11025, 1103), (192000, 19200)])
def test_hop_and_coefficients_at_other_rates(rate, hop):
    coef, h = ses.loudness_filter(rate)
    assert h == hop == ref.hop(rate)
    b1, a1, b2, a2 = ref.coefficients(rate)
    assert np.abs(coef - np.array(b1 + a1[1:] + b2 + a2[1:])).max() <= 1e-15
    shelf, hp = ae.k_weighting(rate)
    assert shelf == (b1, a1) and hp == (b2, a2)


@pytest.mark.parametrize("rate", [7999, 0, -1, 192001])
def test_the_filter_refuses_rates_outside_its_range(rate):
    with pytest.raises(SessionError, match=f"sample_rate {rate}"):
        ses.loudness_filter(rate)


# ------------------------------------------------------------------ gating

@pytest.fixture(scope="module")
def signals():
    """rate -> (signal, its float64 sub-block energies): computed once"""
    return {fs: (x, ref.sub_blocks(x, fs)) for fs in (22050, 8000) for x in [ref.gating_signal(fs)]}


@pytest.mark.parametrize("fs, L", [(22050, -16.987), (8000, -17.199)])
def test_the_gates_on_the_test_signal(signals, fs, L):
    x, e = signals[fs]
    want = ref.gate([e], fs)
    assert want[1:] == (37, 35, 30) and abs(want[0] - L) < 1e-3
    assert ref.ungated(x, fs) < want[0] - 0.9              # (a missing gate would show as 0.9 LU)
    got = ses.loudness_gate([e], ref.hop(fs))
    assert got[1:] == (37, 35, 30)
    assert abs(got[0] - want[0]) <= 1e-6
    assert abs(ae.loudness(x, fs) - want[0]) <= 1e-6        # the fallback's statement of the same


@pytest.mark.parametrize("fs", [48000, 22050, 16000, 8000])
def test_a_full_scale_997_hz_sine_reads_minus_3(fs):
    e = ref.sub_blocks(ref.sine(fs), fs)
    assert abs(ses.loudness_gate([e], ref.hop(fs))[0] - -3.01) <= 0.05
    assert abs(ae.gated_loudness([e], fs) - -3.01) <= 0.05


def test_gate_edge_cases(signals):
    fs = 22050
    _, e = signals[fs]
    loud = e[10:14]                                         # (sub-blocks at the full amplitude)
    for n, blocks in ((0, 0), (3, 0), (4, 1)):
        got = ses.loudness_gate([loud[:n]], ref.hop(fs))
        want = ref.gate([loud[:n]], fs)
        assert got[1:] == want[1:] == (blocks, blocks, blocks)
        assert got[0] == want[0] == -math.inf if n < 4 else abs(got[0] - want[0]) <= 1e-6
    assert ses.loudness_gate([], ref.hop(fs)) == (-math.inf, 0, 0, 0)
    # every block below -70 LUFS: none passes, the gain is 1
    quiet = np.full(8, 1e-9 * ref.hop(fs), np.float32)
    assert ses.loudness_gate([quiet], ref.hop(fs)) == (-math.inf, 5, 0, 0) == ref.gate([quiet], fs)
    assert ses.level_gain(-math.inf, 0.5, ses.Level(1, -19.0, 30.0, 0.5)) == np.float32(1.0)
    # exactly silent sub-blocks (log10 0) are gated, not an error
    assert ses.loudness_gate([np.zeros(6, np.float32)], ref.hop(fs)) == (-math.inf, 3, 0, 0)
    with pytest.raises(SessionError, match="hop"):
        ses.loudness_gate([loud], 0)


def test_stream_pooling_of_two_rows(signals):
    fs = 8000
    _, e = signals[fs]
    a, b = e[:17], (e[17:] * 0.1)
    want = ref.gate([a, b], fs)
    got = ses.loudness_gate([a, b], ref.hop(fs))
    assert got[1:] == want[1:] and got[1] == (17 - 3) + (e.size - 17 - 3)       # no block straddles the two rows
    assert abs(got[0] - want[0]) <= 1e-6
    assert abs(got[0] - ses.loudness_gate([np.concatenate([a, b])], ref.hop(fs))[0]) > 1e-3
    assert abs(ae.gated_loudness([a, b], fs) - want[0]) <= 1e-6


# ------------------------------------------------------------------ the gain

@pytest.mark.parametrize("name, L, peak, level", [
    ("plain", -30.0, 0.1, Level(1, -19.0, 30.0, 0.0)),
    ("the max-gain cap binds", -60.0, 0.01, Level(1, -16.0, 20.0, 0.0)),
    ("the ceiling binds", -30.0, 0.5, Level(1, -19.0, 30.0, 0.9)),
    ("the ceiling does not bind", -30.0, 0.1, Level(1, -19.0, 30.0, 0.9)),
    ("peak = 0", -30.0, 0.0, Level(2, -19.0, 30.0, 0.9)),
    ("L = -inf", -math.inf, 0.5, Level(1, -19.0, 30.0, 0.9)),
    ("attenuation", -10.0, 0.9, Level(2, -23.0, 0.0, 0.0)),
])
def test_level_gain(name, L, peak, level):
    got = ses.level_gain(L, peak, ses.Level(*level))
    assert got == ref.gain(L, np.float32(peak), level) and got.dtype == np.float32
    assert got == ae.level_gain(L, np.float32(peak), level.target_lufs, level.max_gain_db, level.peak_ceiling)
    want = {"plain": 10 ** (11 / 20), "the max-gain cap binds": 10.0, "the ceiling binds": float(np.float32(0.9)) / 0.5,
            "the ceiling does not bind": 10 ** (11 / 20), "peak = 0": 10 ** (11 / 20), "L = -inf": 1.0,
            "attenuation": 10 ** (-13 / 20)}[name]
    assert got == np.float32(want)


def test_level_gain_refuses_bad_arguments():
    with pytest.raises(SessionError, match="max_gain_db 121"):
        ses.level_gain(-20.0, 0.5, ses.Level(1, -19.0, 121.0, 0.0))
    for L, peak in ((float("nan"), 0.5), (math.inf, 0.5), (-20.0, -0.5), (-20.0, float("nan"))):
        with pytest.raises(SessionError, match="loudness"):
            ses.level_gain(L, peak, ses.Level(1, -19.0, 30.0, 0.0))


# ------------------------------------------------------------------ refusals, through the pure plan entry

def _plan_with_canaries(segs, levels, rate, trims=None, J=2):
    out = (np.full(J, -77, np.int64), np.full(J + 1, -77, np.int64))
    return out, lambda: ses.level_plan(COUNTS, _segs(segs), levels, rate, J, "pcm16", trims=trims, out=out)


@pytest.mark.parametrize("name", sorted(ref.LEVEL_REFUSALS))
def test_level_refusals_name_the_segment_and_the_value(name):
    norms, levels, rate, index, word = ref.LEVEL_REFUSALS[name]
    segs = [s._replace(normalize=n) for s, n in zip(GOOD, norms)]
    with pytest.raises(ValueError) as exc_ref:
        ref.check(COUNTS, segs, None, levels, 2, "pcm16", rate)
    assert str(exc_ref.value) == ("rate" if index is None else f"segment {index}")
    out, call = _plan_with_canaries(segs, _levels(levels), rate)
    with pytest.raises(SessionError) as exc:
        call()
    msg = str(exc.value)
    assert word in msg and (index is None or f"segment {index}: " in msg), msg
    assert (out[0] == -77).all() and (out[1] == -77).all()            # a refusal writes nothing


def test_what_the_trimmed_delivery_refuses_is_refused():
    good = _levels([Level(1, -19.0, 30.0, 0.0)] * 3)
    plain = [s._replace(normalize=0) for s in GOOD]
    for name, (segs, J, enc, index, word) in dref.REFUSALS.items():
        with pytest.raises(SessionError) as exc:
            ses.level_plan(COUNTS, _segs(segs), ses.Level(0), 22050, J, enc)
        assert word in str(exc.value), name
    for name, (trims, index, word) in tref.TRIM_REFUSALS.items():
        out, call = _plan_with_canaries(plain, good, 22050, trims=[ses.Trim(*t) for t in trims])
        with pytest.raises(SessionError) as exc:
            call()
        assert f"segment {index}: " in str(exc.value) and word in str(exc.value), name
        assert (out[0] == -77).all()
    with pytest.raises(SessionError, match="one Level or one per segment"):
        ses.level_plan(COUNTS, _segs(plain), good[:2], 22050, 2)


def test_levels_never_change_the_layout():
    plain = [s._replace(normalize=0) for s in GOOD]
    trims = [ses.Trim(0, 0.0, 0, 0, 4), ses.Trim(), ses.Trim(0, 0.0, 0, 0, 1)]
    for enc in ENCODINGS:
        base = ses.delivery_plan(COUNTS, _segs(plain), 2, enc, trims=trims)
        for levels in (None, ses.Level(), ses.Level(1, -19.0, 30.0, 0.5),
                       _levels([Level(1, -16.0, 10.0, 0.0), Level(2, -19.0, 30.0, 0.5), Level(2, -19.0, 30.0, 0.5)])):
            got = ses.level_plan(COUNTS, _segs(plain), levels, 8000, 2, enc, trims=trims)
            assert got["total_bytes"] == base["total_bytes"]
            assert np.array_equal(got["stream_offsets"], base["stream_offsets"])
            assert np.array_equal(got["stream_samples"], base["stream_samples"])
    # mode 0 everywhere: neither the rate nor a normalising segment is looked at
    assert ses.level_plan(COUNTS, _segs(GOOD), ses.Level(0, -19.0, 30.0, 0.0), 0, 2)["total_bytes"] > 0
    assert ses.Level() == ses.Level(0, -23.0, 30.0, 0.0)


def test_abi_surface():
    lib = _ffi.load()
    for name in ("vits_loudness_filter", "vits_loudness_gate", "vits_level_gain", "vits_delivery_plan_leveled", "vits_deliver_leveled",
                 "vits_test_loudness_blocks", "vits_test_deliver_leveled"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS
    assert C.sizeof(_ffi.VitsLevel) == 16                   # int32 and three floats: the header's struct
    assert C.sizeof(_ffi.VitsSegment) == 24 and C.sizeof(_ffi.VitsTrim) == 24
    assert ses.loudness_chunk() >= 800                      # (a chunk touches at most three sub-blocks at every admitted rate)
    from conftest import GOLDEN
    from phoonnx_amd import MiSession
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    assert s.delivered_rate == int(s.meta("sample_rate") or 22050)
    with pytest.raises(SessionError, match="host-only"):
        s.deliver([Segment(0, 0, 0, 0)], 1, "pcm16", levels=ses.Level(1, -19.0))
    s.close()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    assert "levelled delivery" in header and "loudness (RMS) levelling" not in header


# ------------------------------------------------------------------ the workspace walk: a stand-alone driver

def test_the_level_buffers_have_a_walk_of_their_own(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "loudness_driver")
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                        os.path.join(ROOT, "tests", "loudness_driver.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines()]
    walks = [d for d in lines if "walk" in d]
    assert [(d["B"], d["S"]) for d in walks] == [(1, 1), (1, 799), (3, 1025), (32, 215040), (7, 100000)]
    for d in walks:
        assert d["fits"] == 1 and d["short_fits"] == 0 and d["level"] > 0, d
        # what a plan can ask of the buffers: every row whole, in one segment each, at the smallest hop
        assert d["chunks"] >= d["B"] * -(-d["S"] // d["Lc"]) and d["subs"] >= d["B"] * (d["S"] // 800) and d["peaks"] == d["B"]
    big = walks[3]
    assert big["level"] < 0.02 * big["delivery"]            # (small beside the delivery's own buffers)
    # the transition matrix: a chunk run from a state equals (run from rest) + M state, and the filter's table
    t = [d for d in lines if "transition" in d][0]
    assert t["err"] < 1e-12 and t["hop"] == 2205 and t["parts"] == 3


# ------------------------------------------------------------------ the NumPy fallback

def _rows(fs):
    x = ref.gating_signal(fs, 1.5)
    rng = np.random.default_rng(5)
    return [x[int(0.5 * fs):].copy() * np.float32(0.3), rng.uniform(-0.9, 0.9, int(0.7 * fs)).astype(np.float32),
            rng.uniform(-0.2, 0.2, int(0.3 * fs)).astype(np.float32), np.zeros(0, np.float32)]


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("mode", [1, 2])
def test_fallback_equals_the_reference(encoding, mode):
    fs = 8000
    rows = _rows(fs)
    x = np.full((len(rows), max(map(len, rows)) + 3), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    for level, trim, lead, vol in ((Level(mode, -19.0, 30.0, 0.0), None, 0, 1.0), (Level(mode, -12.0, 6.0, 0.0), None, 3, 0.5),
                                   (Level(mode, -14.0, 40.0, 0.25), tref.Trim(2, 0.5, 2, 2, 4), 5, 2.0)):
        tail = trim.tail_samples if trim else 0
        data, kept, loud, gains = ae.join_leveled(rows, fs, level, encoding, lead, tail, trim, vol)
        segs = [Seg(b, 0, lead, 0, np.float32(vol)) for b in range(len(rows))]
        trims = [trim or tref.OFF] * len(rows)
        want_l, want_g, want_kept = ref.measure(x, counts, segs, trims, [level] * len(rows), 1, fs)
        assert kept == want_kept
        assert np.allclose(loud, want_l, rtol=0, atol=1e-9, equal_nan=True) or all(
            (a == b) or abs(a - b) <= 1e-9 for a, b in zip(loud, want_l))
        assert [np.float32(g) for g in gains] == want_g.tolist()
        assert data.tobytes() == ref.deliver_ref(x, counts, segs, trims, [level] * len(rows), 1, encoding, want_g)[0]
        assert loud[2] == -math.inf or mode == 2            # (0.3 s: no block of its own)
        if mode == 1:
            assert gains[2] == 1.0 and gains[3] == 1.0 and loud[3] == -math.inf
        else:
            assert len(set(gains)) == 1 and len(set(loud)) == 1
    with pytest.raises(ValueError, match="mode 0"):
        ae.join_leveled(rows, fs, Level(0, -19.0, 30.0, 0.0), encoding)


def test_a_levelled_row_reads_its_target():
    fs = 22050
    x = ref.gating_signal(fs, 2.0)[int(0.5 * fs):]
    data, _, loud, gains = ae.join_leveled([x], fs, Level(1, -23.0, 30.0, 0.0), "f32")
    assert abs(ref.loudness(data, fs) - -23.0) <= 1e-3 and abs(loud[0] + 20.0 * math.log10(gains[0]) - -23.0) <= 1e-5
    capped = ae.join_leveled([x], fs, Level(1, -3.0, 60.0, 0.5), "f32")
    assert np.abs(capped[0]).max() <= np.float32(0.5) and abs(float(np.abs(capped[0]).max()) - 0.5) <= 0.5 * 2.0 ** -23


# ------------------------------------------------------------------ the voice layer on stub sessions

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


class _Stub:
    """A session without delivery: a row is a tone whose amplitude follows its first id, long enough to have blocks; 100
    frames per id at a hop of 8 (16 kHz: 0.05 s per id), garbage behind each row's end."""
    HOP = 8

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": 4}[key]

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None, return_durations=False):
        B = ids.shape[0]
        frames = lens.astype(np.int64) * 100
        out = np.full((B, 1, 1, int(frames.max()) * self.HOP + 4), 9.0, np.float32)
        for b in range(B):
            n = int(frames[b]) * self.HOP
            t = np.arange(n, dtype=np.float32)
            out[b, 0, 0, :n] = np.float32(0.02 * (1 + int(ids[b, 0]) % 7)) * np.sin(t * np.float32(0.2 + 0.01 * b))
        return {"output": out, "y_lengths": frames}


class _Delivering(_Stub):
    """... and one that delivers: the plan it is given, measured and applied by the reference on the same waveforms"""

    def __init__(self):
        self.calls = []

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", seeds=None,
                             return_durations=False, trim=None, levels=None):
        r = self.synthesize_batch(ids, lens, scales, sid, seeds=seeds)
        x, counts = r["output"][:, 0, 0, :], r["y_lengths"] * self.HOP
        self.calls.append((levels, encoding))
        n = len(segments)
        trims = [tref.OFF if trim is None else tref.Trim(trim.mode, trim.threshold, trim.keep_lead, trim.keep_tail, trim.tail_samples)] * n
        lv = [ref.OFF if levels is None else Level(levels.mode, levels.target_lufs, levels.max_gain_db, levels.peak_ceiling)] * n
        loud, gains, kept = ref.measure(x, counts, segments, trims, lv, n_streams, 16000)
        got = ref.deliver_ref(x, counts, segments, trims, lv, n_streams, encoding, gains)
        streams = [np.frombuffer(b, dref.DTYPE[encoding]) for b in got]
        out = {"streams": streams, "stream_samples": np.array([len(a) for a in streams]), "y_lengths": r["y_lengths"],
               "sample_lengths": counts, "kept_first": np.array([a for a, _ in kept]), "kept_count": np.array([c for _, c in kept])}
        if levels is not None:
            out["loudness"], out["gain"] = loud, gains
        return out


def _voice(session):
    cfg = VoiceConfig(num_symbols=64, num_speakers=4, num_langs=1, sample_rate=16000, lang_code="en",
                      phoneme_id_map={c: [i + 1] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


TEXT = "the quick brown fox. a. over a lazy dog"          # the middle sentence: a few ids at 0.05 s each, no block


@pytest.mark.parametrize("scope", ["sentence", "text"])
@pytest.mark.parametrize("encoding", ["pcm16", "ulaw", "f32"])
def test_synthesize_encoded_levels_on_stub_sessions(encoding, scope):
    cfg = SynthesisConfig(speaker_id=1, volume=0.9, normalize_audio=False)
    host, dev = _voice(_Stub()), _voice(_Delivering())
    kw = dict(encoding=encoding, sentence_silence=0.01, loudness=-19.0, loudness_scope=scope, peak_ceiling=0.9, trailing_silence=0.02)
    a, d = host.synthesize_encoded(TEXT, cfg, **kw), dev.synthesize_encoded(TEXT, cfg, **kw)
    assert a.tobytes() == d.tobytes() and a.sentence_starts == d.sentence_starts and a.sentence_samples == d.sentence_samples
    lv, enc = dev.session.calls[-1]
    assert (lv.mode, lv.target_lufs, lv.max_gain_db, lv.peak_ceiling) == (1 if scope == "sentence" else 2, -19.0, 30.0, 0.9)
    for e in (a, d):
        assert len(e.loudness) == len(e.gain) == 3
        if scope == "sentence":
            assert e.loudness[1] == -math.inf and e.gain[1] == 1.0       # under 400 ms: no integrated loudness, gain 1
            assert abs(e.loudness[0] + 20 * math.log10(e.gain[0]) - -19.0) < 1e-4
        else:
            assert len(set(e.gain)) == 1 and len(set(e.loudness)) == 1 and e.gain[0] > 1.0
    assert np.allclose(a.gain, d.gain, rtol=1e-6) and np.allclose(a.loudness, d.loudness, atol=1e-6)
    # the defaults: no level reaches the session, no figures come back
    base = dev.synthesize_encoded(TEXT, cfg, encoding=encoding)
    assert dev.session.calls[-1][0] is None and base.loudness is None and base.gain is None
    with pytest.raises(ValueError, match="normalize_audio"):
        host.synthesize_encoded(TEXT, SynthesisConfig(normalize_audio=True), loudness=-19.0)
    for bad in (dict(loudness=1.0), dict(loudness=float("nan")), dict(loudness=-19.0, loudness_scope="row"),
                dict(loudness=-19.0, peak_ceiling=1.5), dict(loudness=-19.0, max_gain_db=-1.0)):
        with pytest.raises(ValueError):
            host.synthesize_encoded(TEXT, cfg, **bad)


@pytest.mark.parametrize("scope", ["sentence", "text"])
def test_synthesize_requests_encoded_levels_on_stub_sessions(scope):
    texts = ["the quick brown fox. jumps over the", "a lazy dog sleeps in the sun. all day long", "hello there you"]
    cfgs = [SynthesisConfig(speaker_id=i, volume=(1.0, 0.5, 2.0)[i], normalize_audio=False) for i in range(3)]
    reqs = list(zip(texts, cfgs))
    host, dev = _voice(_Stub()), _voice(_Delivering())
    kw = dict(max_batch=2, encoding="alaw", sentence_silence=0.01, loudness=-20.0, loudness_scope=scope, trailing_silence=0.01)
    a, d = host.synthesize_requests_encoded(reqs, **kw), dev.synthesize_requests_encoded(reqs, **kw)
    for r in range(3):
        assert a[r].tobytes() == d[r].tobytes() and a[r].sentence_samples == d[r].sentence_samples
        assert np.allclose(a[r].gain, d[r].gain, rtol=1e-6) and len(a[r].gain) == len(a[r].sentence_samples)
        if scope == "text":
            assert len(set(a[r].gain)) == 1
    # sentence scope levels on the device; text scope fetches float32 and levels a request's sentences together on the host
    assert all((lv is not None and lv.mode == 1 and enc == "alaw") if scope == "sentence" else (lv is None and enc == "f32")
               for lv, enc in dev.session.calls)
    with pytest.raises(ValueError, match="normalize_audio"):
        host.synthesize_requests_encoded([(texts[0], None)], loudness=-20.0)
