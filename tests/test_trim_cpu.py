"""Trimmed delivery (include/vitsmi.h, "trimmed delivery") without a GPU: the kept-range rule and the plan with tails - in a
stand-alone driver built with the host compiler, and through the library's pure host entries - against tests/trim_ref.py;
the refusals; the NumPy fallback; the voice layer on stub sessions.  Everything is compared exactly."""
import ctypes as C
import json
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import delivery_ref as dref
import trim_ref as ref
from conftest import ROOT
from delivery_ref import COUNTS, GOOD, Seg
from trim_ref import OFF, Trim

from phoonnx_amd import _ffi
from phoonnx_amd import audio_encoding as ae
from phoonnx_amd import session as ses
from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
from phoonnx_amd.session import Segment, SessionError, delivery_plan
from phoonnx_amd.voice import TTSVoice

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")


def _segs(segs):
    return [Segment(int(s.row), int(s.stream), int(s.lead_samples), int(s.normalize), float(s.volume)) for s in segs]


def _trims(trims):
    return [ses.Trim(*t) for t in trims]


# ------------------------------------------------------------------ the driver: rule and plan, a few hundred random plans

@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("trim") / "trim_driver")
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + csrc, os.path.join(ROOT, "tests", "trim_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()]


def test_driver_plans_equal_the_reference(driver_lines):
    plans = [d for d in driver_lines if "walk" not in d]
    assert len(plans) == 400
    seen = {k: 0 for k in ("front cut", "back cut", "emptied", "n = 0", "lead clipped", "tail clipped", "tail behind lead",
                           "tail without lead", "merged", "split by a tail", "untrimmed")}
    lib = _ffi.load()
    for d in plans:
        assert d["err"] == "", d
        B, J, enc, w = d["B"], d["J"], ENCODINGS[d["enc"]], d["width"]
        assert w == dref.WIDTH[enc]
        segs = [Seg(r, j, lead, nz, 1.0) for r, j, lead, nz in d["segs"]]
        trims = [Trim(m, 0.25, kl, kt, tail) for m, kl, kt, tail in d["trims"]] if d["with_trims"] else None
        # the rule, row by row: the driver's trim_range, the library's vits_trim_range and the reference agree
        first, kept = [0] * B, list(d["counts"])
        for g, s in enumerate(segs):
            if trims is None:
                continue
            t, n, f, l = trims[g], d["counts"][s.row], d["f"][s.row], d["l"][s.row]
            first[s.row], kept[s.row] = ref.kept_range(n, f, l, t)
            a, c = C.c_int64(-1), C.c_int64(-1)
            ct = _ffi.VitsTrim(t.mode, t.threshold, t.keep_lead, t.keep_tail, t.tail_samples)
            assert lib.vits_trim_range(n, f, l, C.byref(ct), C.byref(a), C.byref(c)) == 0, _ffi.last_error(None)
            assert (a.value, c.value) == (first[s.row], kept[s.row])
            assert 0 <= a.value and a.value + c.value <= n
            if t.mode and f <= l:
                assert a.value <= f and l < a.value + c.value
                seen["front cut"] += a.value > 0
                seen["back cut"] += a.value + c.value < n
                seen["lead clipped"] += f - t.keep_lead < 0
                seen["tail clipped"] += l + 1 + t.keep_tail > n
            elif t.mode:
                assert c.value == 0
                seen["emptied"] += n > 0
                seen["n = 0"] += n == 0
            seen["tail behind lead"] += t.tail_samples > 0 and s.lead_samples > 0
            seen["tail without lead"] += t.tail_samples > 0 and s.lead_samples == 0
        assert d["first"] == first and d["kept"] == kept
        # the layout
        samples, offsets, total = ref.plan_ref(kept, segs, trims, J, enc)
        assert d["samples"] == samples.tolist() and d["offsets"] == offsets.tolist() and d["total"] == total
        emap, per_stream = ref.element_map(kept, segs, trims, J)
        assert per_stream == d["samples"] and emap.size * w == total
        assert d["packed"] == int((emap >= 0).sum())
        # copies: exactly the maximal silence-free runs of dst, each from where its first element lies in the packed audio
        want = [[int(emap[a]) * w, a * w, n * w] for a, n in ref.runs(emap >= 0)]
        assert d["copies"] == want, (d, want)
        # fills: disjoint, and together exactly the silent elements
        silent = np.zeros(emap.size, int)
        for off, n in d["fills"]:
            assert off % w == 0 and n > 0
            silent[off // w:off // w + n] += 1
        assert np.array_equal(silent, (emap < 0).astype(int))
        # the table the kernels read: dst order, each segment's first packed element, its source range, its peak slot
        order = [g for j in range(J) for g, s in enumerate(segs) if s.stream == j]
        assert d["order"] == order
        start = 0
        for k, g in enumerate(order):
            s = segs[g]
            slot = {0: -1, 1: s.row, 2: B + s.stream}[s.normalize]
            assert d["table"][k] == [start, s.row * 1000 + first[s.row], kept[s.row], slot]
            start += kept[s.row]
        assert d["max_n"] == max([kept[s.row] for s in segs], default=0)
        seen["merged"] += len(d["copies"]) < sum(1 for s in segs if kept[s.row] > 0)
        if trims is not None:
            for k in range(len(order) - 1):
                g, h = order[k], order[k + 1]
                seen["split by a tail"] += (trims[g].tail_samples > 0 and segs[h].lead_samples == 0 and kept[segs[g].row] > 0
                                            and kept[segs[h].row] > 0)
        else:
            seen["untrimmed"] += 1
            got = delivery_plan(d["counts"], _segs(segs), J, enc)       # the untrimmed entry, the same inputs
            assert got["stream_samples"].tolist() == d["samples"] and got["total_bytes"] == d["total"]
    assert all(v >= 5 for v in seen.values()), seen


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program itself, built with -fsanitize=address,undefined (nothing loaded into Python is sanitised): rule,
    plan and walks without a report, and the same output as the plain build's."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    exe = str(tmp_path / "trim_driver_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                        os.path.join(ROOT, "tests", "trim_driver.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert len(r.stdout.splitlines()) == 404


def test_the_trim_slots_have_a_walk_of_their_own(driver_lines):
    walks = [d for d in driver_lines if "walk" in d]
    assert [d["walk"] for d in walks] == [1, 3, 32, 256]
    for d in walks:
        assert d["ok"] == 1 and 12 * d["walk"] <= d["with_trim"] - d["delivery"] <= 12 * d["walk"] + 2 * 256, d


# ------------------------------------------------------------------ the library's host entries

PLANS = {
    "tails and leads": ([Seg(4, 1, 3, 1, 1.0), Seg(0, 1, 0, 2, 0.5), Seg(2, 0, 1, 0, 2.5)], [Trim(1, 0.1, 0, 0, 4), OFF, Trim(2, 0.5, 1, 1, 2)], 3),
    "an empty row with a tail": ([Seg(1, 0, 0, 1, 1.0)], [Trim(0, 0.0, 0, 0, 9)], 1),
    "the largest tails": ([Seg(5, 0, dref.INT_MAX, 0, 1.0), Seg(3, 0, 0, 0, 1.0)], [Trim(0, 0.0, 0, 0, dref.INT_MAX)] * 2, 1),
    "no segments": ([], [], 2),
}


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_equals_the_reference(name, encoding):
    segs, trims, J = PLANS[name]
    kept = np.array([3, 0, 7, 1, 11, 0], np.int64)          # (what a scan might have kept of COUNTS)
    assert (kept <= COUNTS).all()
    got = delivery_plan(COUNTS, _segs(segs), J, encoding, trims=_trims(trims), kept=kept)
    samples, offsets, total = ref.plan_ref(kept, segs, trims, J, encoding)
    assert np.array_equal(got["stream_samples"], samples) and np.array_equal(got["stream_offsets"], offsets)
    assert got["total_bytes"] == total == offsets[-1]
    one = delivery_plan(COUNTS, _segs(segs), J, encoding, trims=ses.Trim(0, 0.0, 0, 0, 2), kept=kept) if segs else None
    if one is not None:          # one Trim for every segment
        assert one["total_bytes"] == ref.plan_ref(kept, segs, [Trim(0, 0.0, 0, 0, 2)] * len(segs), J, encoding)[2]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_without_trims_the_plan_is_the_untrimmed_one(encoding):
    for name, (segs, J) in {"a": (GOOD, 2), "b": ([Seg(b, b % 3, b % 2, b % 3, 1.0) for b in range(6)], 3), "c": ([], 1)}.items():
        base = delivery_plan(COUNTS, _segs(segs), J, encoding)
        for trims in ([ses.Trim()] * len(segs), ses.Trim(), [ses.Trim(0, 0.7, 5, 5, 0)] * len(segs)):
            got = delivery_plan(COUNTS, _segs(segs), J, encoding, trims=trims)
            for key in ("stream_samples", "stream_offsets"):
                assert np.array_equal(got[key], base[key]), (name, key)
            assert got["total_bytes"] == base["total_bytes"]
        # trims == NULL through the trimmed entry
        got = delivery_plan(COUNTS, _segs(segs), J, encoding, kept=COUNTS)
        assert got["total_bytes"] == base["total_bytes"] and np.array_equal(got["stream_offsets"], base["stream_offsets"])
    assert ses.Trim() == ses.Trim(0, 0.0, 0, 0, 0)           # the defaults: off, no tail


@pytest.mark.parametrize("name", sorted(ref.TRIM_REFUSALS))
def test_trim_refusals_name_the_segment_and_the_value(name):
    trims, index, word = ref.TRIM_REFUSALS[name]
    with pytest.raises(ValueError) as exc_ref:
        ref.plan_ref(COUNTS, GOOD, trims, 2, "pcm16")
    assert str(exc_ref.value) == f"segment {index}"
    with pytest.raises(SessionError) as exc:
        delivery_plan(COUNTS, _segs(GOOD), 2, "pcm16", trims=_trims(trims))
    msg = str(exc.value)
    assert f"segment {index}: " in msg and word in msg, msg
    # the rule's own entry refuses the same trim, naming the value
    bad = trims[index]
    a, c = C.c_int64(-1), C.c_int64(-1)
    ct = _ffi.VitsTrim(bad.mode, bad.threshold, bad.keep_lead, bad.keep_tail, bad.tail_samples)
    assert _ffi.load().vits_trim_range(5, 1, 2, C.byref(ct), C.byref(a), C.byref(c)) == -3
    assert word in _ffi.last_error(None) and (a.value, c.value) == (-1, -1)


@pytest.mark.parametrize("name", sorted(dref.REFUSALS))
def test_what_the_delivery_refuses_is_refused(name):
    segs, J, enc, index, word = dref.REFUSALS[name]
    with pytest.raises(SessionError) as exc:
        delivery_plan(COUNTS, _segs(segs), J, enc, trims=ses.Trim(2, 0.5, 0, 0, 1))
    assert word in str(exc.value) and (index is None or f"segment {index}:" in str(exc.value))
    with pytest.raises(SessionError, match="one Trim or one per segment"):
        delivery_plan(COUNTS, _segs(GOOD), 2, "pcm16", trims=[ses.Trim()] * 2)


def test_abi_surface():
    lib = _ffi.load()
    for name in ("vits_trim_range", "vits_delivery_plan_trimmed", "vits_deliver_trimmed", "vits_test_deliver_trimmed"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS
    assert C.sizeof(_ffi.VitsTrim) == 24            # int32, float, int32, int32, int64: the header's struct
    a, c = C.c_int64(), C.c_int64()
    t = _ffi.VitsTrim(1, 0.1, 2, 3, 0)
    assert lib.vits_trim_range(100, 10, 50, C.byref(t), C.byref(a), C.byref(c)) == 0 and (a.value, c.value) == (8, 46)
    assert lib.vits_trim_range(100, 1, 99, C.byref(t), C.byref(a), C.byref(c)) == 0 and (a.value, c.value) == (0, 100)
    assert lib.vits_trim_range(100, 5, 4, C.byref(t), C.byref(a), C.byref(c)) == 0 and (a.value, c.value) == (0, 0)
    assert lib.vits_trim_range(0, dref.INT_MAX, -1, C.byref(t), C.byref(a), C.byref(c)) == 0 and (a.value, c.value) == (0, 0)
    assert lib.vits_trim_range(100, 10, 100, C.byref(t), C.byref(a), C.byref(c)) == -3 and "outside" in _ffi.last_error(None)
    assert lib.vits_trim_range(100, 10, 50, None, C.byref(a), C.byref(c)) == -3
    total = C.c_int64(-1)
    seg = (_ffi.VitsSegment * 1)(_ffi.VitsSegment(0, 0, 2, 1, 1.0))
    trim = (_ffi.VitsTrim * 1)(_ffi.VitsTrim(0, 0.0, 0, 0, 3))
    assert lib.vits_delivery_plan_trimmed(_ffi.ptr(COUNTS), 6, seg, trim, 1, 1, 1, None, None, C.byref(total)) == 0 and total.value == 10
    # a host-only handle answers the pure entries and refuses the delivery itself
    from conftest import GOLDEN
    from phoonnx_amd import MiSession
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    with pytest.raises(SessionError, match="host-only"):
        s.deliver([Segment(0)], 1, "pcm16", trims=ses.Trim(2, 0.5))
    s.close()


# ------------------------------------------------------------------ the NumPy fallback

def _rows():
    rng = np.random.default_rng(11)
    rows = []
    for n, lo, hi in ((200, 30, 150), (64, 0, 64), (90, 10, 11), (50, 0, 0), (0, 0, 0), (120, 60, 120)):
        r = rng.uniform(-0.02, 0.02, n).astype(np.float32)
        r[lo:hi] = rng.uniform(0.3, 1.1, hi - lo).astype(np.float32) * rng.choice([-1.0, 1.0], hi - lo).astype(np.float32)
        rows.append(r)
    return rows


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_fallback_equals_the_reference(encoding):
    rows = _rows()
    x = np.full((len(rows), 256), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    cut = {"front": 0, "back": 0, "empty": 0}
    for trim in (Trim(2, 0.25, 0, 0, 0), Trim(1, 0.1, 7, 200, 3), Trim(2, 1.0, 0, 0, 5), Trim(0, 0.0, 0, 0, 2), None):
        for b, r in enumerate(rows):
            a, c = ae.trim_range(x[b], counts[b], trim)
            assert (a, c) == ref.trim_range_ref(x[b], counts[b], trim or OFF)
            cut["front"] += a > 0
            cut["back"] += 0 < a + c < counts[b]
            cut["empty"] += c == 0 and counts[b] > 0
        for lead, norm, vol in ((0, 1, 1.0), (4, 2, 0.8), (1, 0, 2.5)):
            tail = trim.tail_samples if trim else 0
            data, kept = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol)
            segs = [Seg(b, 0, lead, norm, np.float32(vol)) for b in range(len(rows))]
            want, first, count = ref.deliver_ref(x, counts, segs, [trim or OFF] * len(rows), 1, encoding)
            assert data.tobytes() == want[0] and data.dtype == ae.DTYPES[encoding]
            assert [a for a, _ in kept] == first.tolist() and [c for _, c in kept] == count.tolist()
    assert min(cut.values()) >= 2, cut
    # off and without a tail: the untrimmed reference
    data, kept = ae.join_trimmed(rows, encoding, 3, 0, None, 1, 0.5)
    assert data.tobytes() == dref.deliver_ref(x, counts, [Seg(b, 0, 3, 1, np.float32(0.5)) for b in range(len(rows))], 1, encoding)[0]
    with pytest.raises(ValueError, match="mode 5"):
        ae.trim_range(x[0], 10, Trim(5, 0.1, 0, 0, 0))


# ------------------------------------------------------------------ the voice layer on stub sessions

class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


class _Stub:
    """A session without delivery: a row's audio is a burst between a quiet front and a quiet back - the front as long as its
    first phoneme and more, so that trimming empties that phoneme - with garbage behind each row's end; 2 frames per id."""
    HOP = 3

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": 4}[key]

    def last_durations(self):
        raise AssertionError("durations come back with the run")

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None, return_durations=False):
        B = ids.shape[0]
        frames = lens.astype(np.int64) * 2
        out = np.full((B, 1, 1, int(frames.max()) * self.HOP + 4), 9.0, np.float32)
        for b in range(B):
            n = int(frames[b]) * self.HOP
            t = np.arange(n, dtype=np.float32)
            row = np.float32(0.001) * np.sin(t * np.float32(1.3))
            lo, hi = 16 + b, n - 5 - 2 * b           # (12 samples per phoneme: the first one lies wholly in the quiet front)
            row[lo:hi] = np.float32(0.2 * (1 + int(ids[b, 0]) % 5)) * np.cos(t[lo:hi] * np.float32(0.37)) + np.float32(0.05)
            out[b, 0, 0, :n] = row
        res = {"output": out, "y_lengths": frames}
        if return_durations:
            res["durations"] = np.where(np.arange(ids.shape[1])[None, :] < lens[:, None], 2, 0).astype(np.int64)
        return res


class _Delivering(_Stub):
    """... and one that delivers: the plan it is given, applied by the reference to the same waveforms"""

    def __init__(self):
        self.calls = []

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", seeds=None,
                             return_durations=False, trim=None):
        r = self.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=return_durations)
        counts = r["y_lengths"] * self.HOP
        self.calls.append(trim)
        trims = [OFF if trim is None else Trim(trim.mode, trim.threshold, trim.keep_lead, trim.keep_tail, trim.tail_samples)] * len(segments)
        got, first, count = ref.deliver_ref(r["output"][:, 0, 0, :], counts, segments, trims, n_streams, encoding)
        streams = [np.frombuffer(b, dref.DTYPE[encoding]) for b in got]
        out = {"streams": streams, "stream_samples": np.array([len(a) for a in streams]), "y_lengths": r["y_lengths"],
               "sample_lengths": counts, "kept_first": first, "kept_count": count}
        if return_durations:
            out["durations"] = r["durations"]
        return out


def _voice(session):
    cfg = VoiceConfig(num_symbols=64, num_speakers=4, num_langs=1, sample_rate=16000, lang_code="en",
                      phoneme_id_map={c: [i + 1] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


TEXT = "the quick brown fox. jumps. over a lazy dog"


def _reference_stream(voice, cfg, encoding, lead, trim, scope):
    rows = voice.phoneme_ids_batch_to_audio(voice._sentence_ids(TEXT, cfg), cfg)
    x = np.full((len(rows), max(map(len, rows)) + 2), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    norm = 0 if not cfg.normalize_audio else (2 if scope == "text" else 1)
    segs = [Seg(b, 0, lead, norm, np.float32(cfg.volume)) for b in range(len(rows))]
    want, first, count = ref.deliver_ref(x, counts, segs, [trim] * len(rows), 1, encoding)
    return want[0], first.tolist(), count.tolist(), counts


@pytest.mark.parametrize("scope", ["sentence", "text"])
@pytest.mark.parametrize("encoding", ENCODINGS)
def test_synthesize_encoded_trims_on_stub_sessions(encoding, scope):
    cfg = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=True)
    host, dev = _voice(_Stub()), _voice(_Delivering())
    lead, tail = 160, 320                      # 0.01 s and 0.02 s at 16 kHz
    for trim_silence, trim in ((0.25, Trim(2, 0.25, 0, 0, tail)),
                               (ses.Trim(1, 0.02, 0.000125, 0.00025, 0), Trim(1, 0.02, 2, 4, tail)),     # keep_* in seconds
                               (None, Trim(0, 0.0, 0, 0, tail))):
        want, first, count, counts = _reference_stream(host, cfg, encoding, lead, trim, scope)
        if trim.mode:
            assert all(a > 0 for a in first) and all(a + c < n for a, c, n in zip(first, count, counts))      # both ends move
        kw = dict(encoding=encoding, sentence_silence=0.01, normalize_scope=scope, alignments=True, trim_silence=trim_silence,
                  trailing_silence=0.02)
        a, d = host.synthesize_encoded(TEXT, cfg, **kw), dev.synthesize_encoded(TEXT, cfg, **kw)
        assert a.tobytes() == want == d.tobytes()
        t = dev.session.calls[-1]
        assert (t.mode, t.keep_lead, t.keep_tail, t.tail_samples) == (trim.mode, trim.keep_lead, trim.keep_tail, tail)
        starts = [lead + sum(lead + c + tail for c in count[:k]) for k in range(len(count))]
        emptied = 0
        for e in (a, d):
            assert e.sentence_starts == starts and e.sentence_samples == count
            assert len(e.data) == sum(count) + (lead + tail) * len(count)
            for k, al in enumerate(e.phoneme_alignments):          # contiguous from the sentence's start, covering what is kept
                pos = starts[k]
                for p in al:
                    assert p.start_sample == pos and p.num_samples >= 0
                    pos += p.num_samples
                    emptied += p.num_samples == 0
                assert pos == starts[k] + count[k]
        if trim.mode:
            assert emptied >= 2, "no phoneme was trimmed to nothing"
            assert all(al[0].num_samples == 0 for al in a.phoneme_alignments)        # the first phoneme lies in the quiet front
        else:
            assert emptied == 0
    # the defaults: what the call returned before, and no trim reaches the session
    base = dev.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=0.01, normalize_scope=scope)
    assert dev.session.calls[-1] is None
    assert base.tobytes() == host.synthesize_encoded(TEXT, cfg, encoding=encoding, sentence_silence=0.01, normalize_scope=scope).tobytes()
    assert base.sentence_samples == _reference_stream(host, cfg, encoding, lead, OFF, scope)[3]
    for bad in (dict(trim_silence=-0.1), dict(trim_silence=float("nan")), dict(trailing_silence=-1.0)):
        with pytest.raises(ValueError):
            host.synthesize_encoded(TEXT, cfg, **bad)


@pytest.mark.parametrize("encoding", ["ulaw", "f32"])
def test_synthesize_requests_encoded_trims_on_stub_sessions(encoding):
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=i, volume=(1.0, 0.5, 2.0)[i], normalize_audio=i != 1) for i in range(3)]
    reqs = list(zip(texts, cfgs))
    host, dev = _voice(_Stub()), _voice(_Delivering())
    kw = dict(max_batch=4, encoding=encoding, sentence_silence=0.01, alignments=True, trim_silence=0.25, trailing_silence=0.02)
    a, d = host.synthesize_requests_encoded(reqs, **kw), dev.synthesize_requests_encoded(reqs, **kw)
    plain = host.synthesize_requests_encoded(reqs, max_batch=4, encoding=encoding, sentence_silence=0.01)
    for r in range(3):
        assert a[r].tobytes() == d[r].tobytes() and a[r].sentence_starts == d[r].sentence_starts
        assert a[r].sentence_samples == d[r].sentence_samples
        assert all(c < n for c, n in zip(a[r].sentence_samples, plain[r].sentence_samples))
        assert len(a[r].data) == sum(a[r].sentence_samples) + 480 * len(a[r].sentence_samples)
        for e in (a[r], d[r]):
            assert [al[0].start_sample for al in e.phoneme_alignments] == e.sentence_starts
            assert [sum(p.num_samples for p in al) for al in e.phoneme_alignments] == e.sentence_samples
        # each sentence: the reference's bytes of its row alone
        for k, (st, n) in enumerate(zip(a[r].sentence_starts, a[r].sentence_samples)):
            assert a[r].tobytes()[(st - 160) * a[r].data.itemsize:st * a[r].data.itemsize] == dref.SILENCE[encoding] * 160
    assert all(t.tail_samples == 0 and t.mode == 2 for t in dev.session.calls)       # the tail is joined on the host


class _RunOnly:
    """The onnxruntime duck type: run() alone - no batches, no durations (so no alignments, trimmed or not)"""

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

    def run(self, _, feed):
        ids = feed["input"]
        r = _Stub().synthesize_batch(ids, feed["input_lengths"], feed["scales"], feed["sid"])
        n = int(r["y_lengths"][0]) * _Stub.HOP
        return [r["output"][:, :, :, :n] * np.float32(3.0)]        # (beyond [-1, 1]: the cut comes before any clipping)


@pytest.mark.parametrize("encoding", ["pcm16", "alaw"])
def test_the_trimmed_fallback_on_a_session_that_only_runs(encoding):
    voice = _voice(_RunOnly())
    texts = ["the quick brown fox. jumps over", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=1, volume=0.5, normalize_audio=True), SynthesisConfig(speaker_id=0, normalize_audio=False)]
    reqs = list(zip(texts, cfgs))
    kw = dict(encoding=encoding, sentence_silence=0.01, alignments=True)
    plain = voice.synthesize_requests_encoded(reqs, **kw)
    got = voice.synthesize_requests_encoded(reqs, trim_silence=0.25, trailing_silence=0.02, **kw)
    trim, w = Trim(2, 0.25, 0, 0, 0), dref.WIDTH[encoding]
    for r, (text, cfg) in enumerate(reqs):
        assert plain[r].phoneme_alignments is None and got[r].phoneme_alignments is None        # no durations either way
        rows = [np.atleast_1d(voice.phoneme_ids_to_audio(ids, cfg)) for ids in voice._sentence_ids(text, cfg)]
        assert max(np.abs(a).max() for a in rows) > 1.0
        want = b""
        for a in rows:
            x = a[None, :]
            piece = ref.deliver_ref(x, [a.size], [Seg(0, 0, 160, 1 if cfg.normalize_audio else 0, np.float32(cfg.volume))],
                                    [trim._replace(tail_samples=320)], 1, encoding)[0][0]
            want += piece
        assert got[r].tobytes() == want and len(got[r].tobytes()) < len(plain[r].tobytes()) + 320 * w * len(rows)
        assert [n < m for n, m in zip(got[r].sentence_samples, plain[r].sentence_samples)] == [True] * len(rows)
    one = voice.synthesize_encoded(texts[0], cfgs[0], encoding=encoding, sentence_silence=0.01, trim_silence=0.25, trailing_silence=0.02)
    assert one.tobytes() == got[0].tobytes()            # (sentence scope: the same stream through the single-text entry)
