"""Shaped delivery (include/vitsmi.h, "shaped delivery") without a GPU: the multiplier rule and the validation - in a stand-alone
driver built with the host compiler over csrc/shape.hpp, and through the library's pure host entries - against
tests/shape_ref.py; token_envelope against a brute-force restatement; the NumPy fallback; the voice layer on stub sessions.
Everything is compared exactly, multipliers by their bits."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import delivery_ref as dref
import loudness_ref as lref
import shape_ref as ref
import trim_ref as tref
from conftest import ROOT
from delivery_ref import COUNTS, GOOD, Seg
from shape_ref import Shape
from test_trim_cpu import TEXT, _Stub, _rows, _voice
from trim_ref import Trim

from phoonnx_amd import _ffi
from phoonnx_amd import audio_encoding as ae
from phoonnx_amd import session as ses
from phoonnx_amd.config import SynthesisConfig
from phoonnx_amd.session import SessionError

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
CURVE = {0: "linear", 1: "smooth"}


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _ses_shape(s):
    return ses.Shape(s.fade_in, s.fade_out, CURVE[s.curve], tuple(s.points))


def _hex(g):
    return "%08x" % int(np.float32(g).view(np.uint32))


# ------------------------------------------------------------------ the driver: rule and validation

def _kept(batch):
    x, counts, segs, trims, *_ = batch
    return [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segs, trims)]


def _cases(path, batch):
    lines = []
    for name in sorted(ref.SHAPE_REFUSALS):
        records, points, stated, _, _ = ref.SHAPE_REFUSALS[name]
        lines.append(f"C {len(records)} {stated} {len(points)}")
        lines += [" ".join(str(v) for v in r) for r in records]
        lines += [f"{p} {_hex(g)}" for p, g in points]
    shapes = batch[5]
    for (a, c), s in zip(_kept(batch), shapes):
        lines.append(f"G {s.fade_in} {s.fade_out} {s.curve} {len(s.points)} {a} {c}")
        lines += [f"{p} {_hex(g)}" for p, g in s.points]
    with open(path, "w") as f:
        f.write(f"{len(ref.SHAPE_REFUSALS) + len(shapes)}\n" + "\n".join(lines) + "\n")


def _build(exe, *flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", *flags, "-I" + csrc, os.path.join(ROOT, "tests", "shape_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def batch():
    return ref.batch()


@pytest.fixture(scope="module")
def driver(tmp_path_factory, batch):
    d = tmp_path_factory.mktemp("shape")
    exe, cases = str(d / "shape_driver"), str(d / "cases.txt")
    _cases(cases, batch)
    _build(exe)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()], cases


def test_driver_multipliers_equal_the_reference_bit_for_bit(driver, batch):
    lines, _ = driver
    gains = [d["gain"] for d in lines if "gain" in d]
    assert all(d["knots"] == 1 for d in lines if "gain" in d)         # the kernel's form of the envelope: the same bits
    shapes, kept = batch[5], _kept(batch)
    assert len(gains) == len(shapes) == 17 and not any("error" in d for d in lines)
    lib = _ffi.load()
    for g, ((a, c), s, got) in enumerate(zip(kept, shapes, gains)):
        want = ref.multiplier(a, c, s)
        assert np.array_equal(np.array(got, np.uint32), _bits(want)), g
        # the NumPy fallback's statement
        assert np.array_equal(_bits(ae.shape_multiplier(a, c, _ses_shape(s))), _bits(want)), g
        # the library's entry, on the ends, around every point and a stride through the rest
        sarr, parr, _ = ses._shapes(_ses_shape(s), 1)
        near = {a + j for j in range(c) if j < 8 or j >= c - 8 or j % 97 == 0}
        near |= {p + d for p, _ in s.points for d in (-1, 0, 1) if a <= p + d < a + c}
        mul = C.c_float()
        for i in sorted(near):
            assert lib.vits_shape_gain(sarr, parr, a, c, i, C.byref(mul)) == 0, _ffi.last_error(None)
            assert _bits(mul.value) == _bits(want[i - a]), (g, i)
    # what the definition promises of a faded segment: exact zeros at either end, ones in the middle of a segment without points
    for g in (2, 3):
        m = ref.multiplier(*kept[g], shapes[g])
        assert m[0] == 0 and m[-1] == 0 and (m[441:2000] == 1).all() and (np.diff(m[:441]) > 0).all() and (np.diff(m[2000:]) < 0).all()
    assert ses.shape_gain(ses.Shape(), 0, 5, 3) == 1.0 and ses.shape_gain(ses.Shape(2, 0, "smooth"), 7, 5, 8) == 0.5
    for bad in ((0, 5, 5), (0, 5, -1), (-1, 5, 0), (2 ** 31 - 2, 5, 2 ** 31 - 1)):
        with pytest.raises(SessionError, match="kept range"):
            ses.shape_gain(ses.Shape(), *bad)


@pytest.mark.parametrize("name", sorted(ref.SHAPE_REFUSALS))
def test_refusals_name_the_segment_and_the_value(driver, name):
    lines, _ = driver
    records, points, stated, index, words = ref.SHAPE_REFUSALS[name]
    with pytest.raises(ValueError) as exc_ref:
        ref.check_shapes(records, points, stated)
    assert str(exc_ref.value).startswith("call" if index is None else f"segment {index}")
    msgs = [lines[sorted(ref.SHAPE_REFUSALS).index(name)]["check"]]
    with pytest.raises(SessionError) as exc:
        ses.shape_check(ses.RawShapes(records, points, stated), len(records))
    msgs.append(str(exc.value))
    for msg in msgs:
        assert all(w in msg for w in words), msg
        assert index is None or f"segment {index}: " in msg, msg
        if "point " in str(exc_ref.value):
            assert f"point {str(exc_ref.value).split()[-1]}:" in msg, msg
    assert msgs[1].endswith(msgs[0])           # (the library's message is shape.hpp's)


def test_what_is_not_refused():
    ses.shape_check(None, 3)
    ses.shape_check([ses.Shape(2 ** 31 - 1, 2 ** 31 - 1, "smooth", ((0, 2.0 ** -20), (2 ** 31 - 1, 64.0), )), ses.Shape(points=((5, 0.0),))])
    ref.check_shapes([(2 ** 31 - 1, 0, 1, 2, 0)], [(0, 2.0 ** -20), (2 ** 31 - 1, 64.0)], 2)
    # ranges may overlap: a slope depends on its two points alone
    ses.shape_check(ses.RawShapes([(0, 0, 0, 3, 0), (0, 0, 0, 2, 1)], [(1, 1.0), (4, 0.5), (9, 2.0)]), 2)
    with pytest.raises(SessionError, match="one Shape or one per segment"):
        ses._shapes([ses.Shape()] * 2, 3)
    with pytest.raises(SessionError, match="segment 1: shape: curve 'cubic'"):
        ses._shapes([ses.Shape(), ses.Shape(curve="cubic")], 2)
    with pytest.raises(SessionError, match="pos 4294967296"):
        ses._shapes(ses.Shape(points=((2 ** 32, 1.0),)), 1)


def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, driver):
    """The stand-alone program itself, built with -fsanitize=address,undefined (nothing loaded into Python is sanitised)."""
    lines, cases = driver
    exe = str(tmp_path / "shape_driver_san")
    _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert [json.loads(ln) for ln in r.stdout.splitlines()] == lines


def test_the_shape_tables_have_a_walk_of_their_own(driver):
    walks = [d for d in driver[0] if "walk" in d]
    assert [d["walk"] for d in walks] == [1, 3, 32, 256]
    for d in walks:
        need = d["record"] * d["walk"] + 16 * d["points"]
        assert d["ok"] == 1 and d["record"] == 32 and need <= d["with_shape"] - d["level"] <= need + 2 * 256, d


def test_abi_surface():
    lib = _ffi.load()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_shape_check", "vits_shape_gain", "vits_deliver_shaped", "vits_test_deliver_shaped"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsEnvPoint) == 8 and C.sizeof(_ffi.VitsShape) == 24
    assert "shaped delivery" in header and not re.search(r"[,.] fades\b", header)     # the older sections point to the new one
    from conftest import GOLDEN
    from phoonnx_amd import MiSession
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    with pytest.raises(SessionError, match="host-only"):
        s.deliver([ses.Segment(0)], 1, "pcm16", shapes=ses.Shape(4, 4))
    s.close()


# ------------------------------------------------------------------ token_envelope

def _brute_envelope(bounds, gains, ramp):
    """The rule from the samples' side: give every sample its token, find the samples where the gain changes, measure the
    runs on either side."""
    n = int(bounds[-1])
    tok = np.full(n, -1, np.int64)
    for t in range(len(gains)):
        tok[int(bounds[t]):int(bounds[t + 1])] = t
    if n == 0:
        return []
    g = np.asarray(gains, np.float32)[tok]
    if (g == g[0]).all():
        return [] if g[0] == 1 else [(0, float(g[0]))]
    out = {}
    for s in range(1, n):
        if g[s] == g[s - 1]:
            continue
        len_u, len_v = int((tok == tok[s - 1]).sum()), int((tok == tok[s]).sum())
        h = min(ramp // 2, len_u // 2, len_v // 2)
        for pos, val in (((s - h, g[s - 1]), (s + h, g[s])) if h else ((s - 1, g[s - 1]), (s, g[s]))):
            out.setdefault(int(pos), float(val))          # (dict order = insertion order: the first point at a position stays)
    return list(out.items())


def test_token_envelope_equals_a_brute_force_restatement():
    rng = np.random.default_rng(77)
    seen = {"zero-length": 0, "length 1": 0, "dropped": 0, "h = 0": 0, "ramp clipped": 0, "constant": 0, "ones": 0}
    for case in range(300):
        T = int(rng.integers(1, 12))
        lens = rng.choice([0, 0, 1, 1, 2, 3, 7, 20, 41], T)
        bounds = np.concatenate([[0], np.cumsum(lens)])
        ramp = int(rng.choice([0, 1, 5, 8, 16, 1000]))
        kind = case % 10
        gains = (np.ones(T) if kind == 0 else np.full(T, 0.5) if kind == 1 else rng.choice([0.0, 0.25, 1.0, 1.0, 2.0], T)).astype(np.float32)
        got = ses.token_envelope(bounds, gains, ramp)
        want = _brute_envelope(bounds, gains, ramp)
        assert got == want, (bounds, gains, ramp)
        pos = [p for p, _ in got]
        assert all(b > a for a, b in zip(pos, pos[1:])) and all(p >= 0 for p in pos)
        # the envelope equals g_t on each token outside its ramps
        n = int(bounds[-1])
        e = ref.envelope(0, n, got)
        for t in range(T):
            lo, hi = int(bounds[t]) + ramp // 2, int(bounds[t + 1]) - 1 - ramp // 2
            if lo <= hi:
                assert (e[lo:hi + 1] == gains[t]).all(), (bounds, gains, ramp, t)
            if ramp <= 1 and lens[t]:
                assert (e[int(bounds[t]):int(bounds[t + 1])] == gains[t]).all()       # no ramp: a step at every boundary
        if n:
            ses.shape_check([ses.Shape(points=tuple(got))])
        seen["zero-length"] += (lens == 0).any()
        seen["length 1"] += (lens == 1).any()
        raw = sum(2 for s in range(1, n) if _gain_at(bounds, gains, s) != _gain_at(bounds, gains, s - 1))
        seen["dropped"] += len(got) < raw
        seen["h = 0"] += ramp <= 1 and len(got) > 1
        seen["ramp clipped"] += ramp == 1000 and len(got) > 1
        seen["constant"] += got == [(0, 0.5)]
        seen["ones"] += got == [] and n > 0
    assert all(v >= 5 for v in seen.values()), seen
    with pytest.raises(SessionError):
        ses.token_envelope([0, 5], [1.0, 2.0], 4)
    with pytest.raises(SessionError):
        ses.token_envelope([0, 5, 3], [1.0, 2.0], 4)


def _gain_at(bounds, gains, s):
    return gains[int(np.searchsorted(bounds, s, side="right")) - 1]


def test_token_bounds_follow_the_alignment_rule():
    from phoonnx_amd.voice import build_alignments
    rng = np.random.default_rng(5)
    for ratio in (None, (160, 441), (320, 147)):
        for _ in range(20):
            T = int(rng.integers(1, 9))
            dur = rng.integers(0, 6, T)
            pad = np.concatenate([dur, np.zeros(3, np.int64)])
            frames = max(1, int(dur.sum()))
            L, M = ratio or (1, 1)
            N = -(-frames * 256 * L // M)
            al = build_alignments([(str(t), [t]) for t in range(T)], dur, 256, total_frames=frames, ratio=ratio)
            b = ses.token_bounds(pad, T, 256, N, ratio)
            assert b[0] == 0 and (b[T:] == N).all() and b.size == T + 4
            assert [int(v) for v in b[:T]] == [a.start_sample for a in al]
            assert [int(v) for v in np.diff(b[:T + 1])] == [a.num_samples for a in al]
    g = ses.token_gains([[0.0, -np.inf, 6.0, -120.0]], 1, 4)
    assert g.dtype == np.float32 and g[0, 0] == 1 and g[0, 1] == 0 and g[0, 2] == np.float32(10 ** 0.3) and g[0, 3] >= 2.0 ** -20
    for bad in ([[0.0, 37.0]], [[float("nan"), 0.0]], [[float("inf"), 0.0]], [[-121.0, 0.0]], [[0.0]]):
        with pytest.raises(SessionError, match="token_gain_db"):
            ses.token_gains(bad, 1, 2)


# ------------------------------------------------------------------ the NumPy fallback

@pytest.mark.parametrize("encoding", ENCODINGS)
def test_without_shapes_the_fallback_is_what_it_was(encoding):
    rows = _rows()                        # the inputs of test_trim_cpu
    x = np.full((len(rows), 256), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    for trim in (Trim(2, 0.25, 0, 0, 0), Trim(1, 0.1, 7, 200, 3), None):
        for lead, norm, vol in ((0, 1, 1.0), (4, 2, 0.8), (1, 0, 2.5)):
            tail = trim.tail_samples if trim else 0
            base, kept = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol)
            segs = [Seg(b, 0, lead, norm, np.float32(vol)) for b in range(len(rows))]
            want = tref.deliver_ref(x, counts, segs, [trim or tref.OFF] * len(rows), 1, encoding)[0][0]
            assert base.tobytes() == want
            for shapes in (None, ses.Shape(), [ses.Shape()] * len(rows)):
                got, k2 = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, shapes=shapes)
                assert got.tobytes() == want and k2 == kept and got.dtype == base.dtype


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_shaped_fallback_equals_the_reference(encoding):
    rows = _rows()
    x = np.full((len(rows), 256), np.nan, np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    counts = [len(r) for r in rows]
    shapes = [Shape(10, 20, 1, ((5, 0.5), (40, 2.0), (41, 0.25), (400, 1.0))), Shape(0, 0, 0, ((30, 3.0),)), Shape(64, 64, 0, ()),
              ref.NONE, Shape(3, 3, 0, ()), Shape(0, 500, 1, ((0, 0.0), (100, 1.0)))]
    mine = [_ses_shape(s) for s in shapes]
    changed = 0
    for trim in (Trim(2, 0.25, 0, 0, 0), Trim(1, 0.1, 7, 200, 3), None):
        tail = trim.tail_samples if trim else 0
        for lead, norm, vol in ((0, 1, 1.0), (4, 2, 0.8), (1, 0, 2.5)):
            segs = [Seg(b, 0, lead, norm, np.float32(vol)) for b in range(len(rows))]
            want, kept = ref.deliver_ref(x, counts, segs, [trim or tref.OFF] * len(rows), None, shapes, 1, encoding)
            got, k2 = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, shapes=mine)
            assert got.tobytes() == want[0] and k2 == kept
            changed += got.tobytes() != ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol)[0].tobytes()
            one, _ = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, shapes=mine[2])         # one shape for every row
            assert one.tobytes() == ref.deliver_ref(x, counts, segs, [trim or tref.OFF] * len(rows), None, [shapes[2]] * len(rows), 1, encoding)[0][0]
    assert changed == 9
    # levelled: the loudness is that of the unshaped audio, the shape comes behind the gain
    fs = 8000
    long_rows = [lref.sine(fs, 440.0, 0.6, 0.2), lref.sine(fs, 300.0, 0.5, 0.05)]
    lv = ses.Level(1, -20.0, 30.0, 0.0)
    sh = [Shape(100, 300, 1, ((1000, 1.0), (1200, 0.5))), Shape(0, 50, 0, ())]
    base = ae.join_leveled(long_rows, fs, lv, encoding, 2, 3, None, 0.9)
    got = ae.join_leveled(long_rows, fs, lv, encoding, 2, 3, None, 0.9, shapes=[_ses_shape(s) for s in sh])
    assert got[2] == base[2] and [_bits(g) for g in got[3]] == [_bits(g) for g in base[3]] and got[1] == base[1]
    xl = np.zeros((2, 4800), np.float32)
    for b, r in enumerate(long_rows):
        xl[b, :len(r)] = r
    segs = [Seg(b, 0, 2, 0, np.float32(0.9)) for b in range(2)]
    want, _ = ref.deliver_ref(xl, [len(r) for r in long_rows], segs, [Trim(0, 0.0, 0, 0, 3)] * 2, [lref.Level(1, -20.0, 30.0, 0.0)] * 2, sh, 1,
                              encoding, gains=got[3])
    assert got[0].tobytes() == want[0] and got[0].tobytes() != base[0].tobytes()
    with pytest.raises(ValueError, match="one shape or one per row"):
        ae.join_trimmed(rows, encoding, shapes=[ses.Shape()] * 2)
    with pytest.raises(ValueError, match="curve"):
        ae.shape_multiplier(0, 4, ses.Shape(curve="cubic"))
    with pytest.raises(ValueError, match="ascend"):
        ae.shape_multiplier(0, 4, ses.Shape(points=((3, 1.0), (3, 0.5))))


# ------------------------------------------------------------------ the voice layer on stub sessions

class _Shaping(_Stub):
    """A session that delivers: the plan, the shapes and the token gains it is given, applied by the reference to the same
    waveforms - the points from its own durations, as MiSession.synthesize_delivered makes them"""

    def __init__(self):
        self.calls = []

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", seeds=None,
                             return_durations=False, trim=None, shapes=None, token_gain_db=None, gain_ramp=0.01):
        r = self.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=True)
        counts = r["y_lengths"] * self.HOP
        self.calls.append((shapes, token_gain_db))
        used = [ses.Shape()] * len(segments) if shapes is None else ([shapes] * len(segments) if isinstance(shapes, ses.Shape) else list(shapes))
        if token_gain_db is not None:
            B, T = ids.shape
            bounds = [ses.token_bounds(r["durations"][b], lens[b], self.HOP, counts[b]) for b in range(B)]
            used = ses.token_gain_shapes(segments, used, ses.token_gains(token_gain_db, B, T), bounds, int(16000 * gain_ramp))
        trims = [tref.OFF if trim is None else Trim(trim.mode, trim.threshold, trim.keep_lead, trim.keep_tail, trim.tail_samples)] * len(segments)
        mine = [Shape(s.fade_in, s.fade_out, {"linear": 0, "smooth": 1}[s.curve], tuple(s.points)) for s in used]
        got, kept = ref.deliver_ref(r["output"][:, 0, 0, :], counts, segments, trims, None, mine, n_streams, encoding)
        streams = [np.frombuffer(b, dref.DTYPE[encoding]) for b in got]
        out = {"streams": streams, "stream_samples": np.array([len(a) for a in streams]), "y_lengths": r["y_lengths"],
               "sample_lengths": counts, "kept_first": np.array([a for a, _ in kept]), "kept_count": np.array([c for _, c in kept]),
               "shapes": used}
        if return_durations:
            out["durations"] = r["durations"]
        return out


def _db(k, tokens):
    """louder vowels, a silent 'q', sentence 1 as a whole 6 dB down"""
    return [(-np.inf if t == "q" else 4.0 if t in "aeiou" else 0.0) - (6.0 if k == 1 else 0.0) for t in tokens]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_synthesize_encoded_shapes_on_stub_sessions(encoding):
    cfg = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=True)
    host, dev = _voice(_Stub()), _voice(_Shaping())
    kw = dict(encoding=encoding, sentence_silence=0.01, trim_silence=0.25, trailing_silence=0.02, alignments=True)
    plain = host.synthesize_encoded(TEXT, cfg, **kw)
    for more in (dict(fade_in=0.0005, fade_out=0.001), dict(fade_in=0.0005, fade_out=0.001, fade_curve="smooth", phoneme_gain_db=_db),
                 dict(phoneme_gain_db=_db)):
        a, d = host.synthesize_encoded(TEXT, cfg, **kw, **more), dev.synthesize_encoded(TEXT, cfg, **kw, **more)
        assert a.tobytes() == d.tobytes() != plain.tobytes()
        assert a.sentence_starts == d.sentence_starts == plain.sentence_starts and a.sentence_samples == plain.sentence_samples
        shapes, db = dev.session.calls[-1]
        if "fade_in" in more:
            assert (shapes.fade_in, shapes.fade_out, shapes.curve) == (8, 16, more.get("fade_curve", "linear"))     # int(16000 * s)
            zero = ae.encode(np.zeros(1, np.float32), encoding)[0]
            for st, n in zip(a.sentence_starts, a.sentence_samples):
                assert a.data[st] == zero and a.data[st + n - 1] == zero
        else:
            assert shapes is None
        assert (db is not None) == ("phoneme_gain_db" in more)
        if db is not None:          # one value per id, the group's; 0 dB behind a row's end
            groups = host._sentence_groups(TEXT, cfg)
            assert db.shape[0] == len(groups)
            for k, g in enumerate(groups):
                want = [v for v, (_, ids) in zip(_db(k, [t for t, _ in g]), g) for _ in ids]
                assert db[k, :len(want)].tolist() == want and not db[k, len(want):].any()
    # the defaults: no shape reaches the session, and the bytes are the unshaped call's
    base = dev.synthesize_encoded(TEXT, cfg, **kw)
    assert dev.session.calls[-1] == (None, None) and base.tobytes() == plain.tobytes()
    for bad in (dict(fade_in=-0.1), dict(fade_out=float("nan")), dict(fade_in=0.1, fade_curve="cubic")):
        with pytest.raises(ValueError):
            host.synthesize_encoded(TEXT, cfg, **bad)
    with pytest.raises(ValueError, match="2 values"):
        host.synthesize_encoded(TEXT, cfg, phoneme_gain_db=lambda k, tokens: [0.0, 0.0])


@pytest.mark.parametrize("encoding", ["ulaw", "f32"])
def test_synthesize_requests_encoded_shapes_on_stub_sessions(encoding):
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=i, volume=(1.0, 0.5, 2.0)[i], normalize_audio=i != 1) for i in range(3)]
    reqs = list(zip(texts, cfgs))
    host, dev = _voice(_Stub()), _voice(_Shaping())
    for trim in (0.25, None):
        kw = dict(max_batch=4, encoding=encoding, sentence_silence=0.01, trim_silence=trim, trailing_silence=0.02 if trim else 0.0)
        plain = host.synthesize_requests_encoded(reqs, **kw)
        for more in (dict(fade_in=0.0005, fade_out=0.001, fade_curve="smooth"), dict(fade_out=0.001, phoneme_gain_db=_db)):
            a, d = host.synthesize_requests_encoded(reqs, **kw, **more), dev.synthesize_requests_encoded(reqs, **kw, **more)
            for r in range(3):
                assert a[r].tobytes() == d[r].tobytes() != plain[r].tobytes()
                assert a[r].sentence_starts == plain[r].sentence_starts and a[r].sentence_samples == plain[r].sentence_samples
        assert [p.tobytes() for p in dev.synthesize_requests_encoded(reqs, **kw)] == [p.tobytes() for p in plain]
        assert dev.session.calls[-1] == (None, None)
