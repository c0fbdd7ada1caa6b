"""Limited delivery (include/vitsmi.h, "limited delivery") without a GPU: the rule and the validation - in a stand-alone driver
built with the host compiler over csrc/limit.hpp, and through the library's pure host entries - against tests/limit_ref.py;
the NumPy fallback; the voice layer on stand-in sessions.  Everything is compared exactly, gains by their bits."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import limit_ref as ref
import loudness_ref as lref
import shape_ref as sref
import trim_ref as tref
from conftest import ROOT
from delivery_ref import Seg
from limit_ref import Limit
from test_shape_cpu import _Shaping
from test_trim_cpu import TEXT, _Stub, _rows, _voice
from trim_ref import Trim

from phoonnx_amd import _ffi
from phoonnx_amd import audio_encoding as ae
from phoonnx_amd import session as ses
from phoonnx_amd.config import SynthesisConfig
from phoonnx_amd.session import SessionError

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")
LOOKAHEADS = (1, 7, 255, 1024)
LENGTHS = (1, 5, 300, 5000)
F = np.float32


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def _hex(v):
    return "%08x" % int(np.float32(v).view(np.uint32))


def _seeded(L, c):
    rng = np.random.default_rng(1000 * L + c)
    return (rng.standard_normal(c) * 0.8).astype(F)


def _edges():
    """name -> (u, ceiling, L): the named edges of the rule"""
    quiet = np.full(400, 0.25, F)
    first, last = quiet.copy(), quiet.copy()
    first[0], last[-1] = 0.95, -0.95
    at = quiet.copy()
    at[100] = F(0.7)                       # |u| at the ceiling exactly
    huge = quiet.copy()
    huge[200] = 6e10
    short = (np.random.default_rng(3).standard_normal(40) * 0.9).astype(F)
    return {"loud first": (first, 0.7, 110), "loud last": (last, 0.7, 110), "c <= L": (short, 0.5, 255), "c == L": (short, 0.5, 40),
            "all below": (quiet, 0.7, 110), "at the ceiling": (at, 0.7, 7), "huge": (huge, 0.7, 7)}


GAIN_CASES = [(_seeded(L, c), 0.7, L) for L in LOOKAHEADS for c in LENGTHS] + list(_edges().values())


def _cases(path):
    lines = []
    for name in sorted(ref.LIMIT_REFUSALS):
        limits, vol, _, _ = ref.LIMIT_REFUSALS[name]
        lines.append(f"C {len(limits)}")
        lines += [f"{m} {_hex(cl)} {la} {rs} {_hex(vol if g == 1 and vol is not None else 1.0)}" for g, (m, cl, la, rs) in enumerate(limits)]
    for u, ceiling, L in GAIN_CASES:
        lines.append(f"G {_hex(ceiling)} {L} {len(u)}")
        lines.append(" ".join(_hex(v) for v in u))
    with open(path, "w") as f:
        f.write(f"{len(ref.LIMIT_REFUSALS) + len(GAIN_CASES)}\n" + "\n".join(lines) + "\n")


def _build(exe, *flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "phoonnx_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", *flags, "-I" + csrc, os.path.join(ROOT, "tests", "limit_driver.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("limit")
    exe, cases = str(d / "limit_driver"), str(d / "cases.txt")
    _cases(cases)
    _build(exe)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return [json.loads(ln) for ln in r.stdout.splitlines()], cases


@pytest.fixture(scope="module")
def want():
    """the reference's gains of every gain case: computed once"""
    return [ref.gains(u, Limit(ceiling, L)) for u, ceiling, L in GAIN_CASES]


# ------------------------------------------------------------------ the rule

def test_gains_equal_the_reference_bit_for_bit(driver, want):
    lines = [d for d in driver[0] if "gain" in d]
    assert len(lines) == len(GAIN_CASES) and not any("error" in d for d in driver[0])
    for (u, ceiling, L), w, d in zip(GAIN_CASES, want, lines):
        assert np.array_equal(np.array(d["gain"], np.uint32), _bits(w)), (L, len(u))               # csrc/limit.hpp, host compiler
        assert d["q"] == ref.q_of(u, ceiling).tolist(), (L, len(u))
        assert np.array_equal(_bits(ses.limit_gains(u, ses.Limit(ceiling, L))), _bits(w)), (L, len(u))  # the library's entry
        assert np.array_equal(_bits(ae.limit_gains(u, ceiling, L)), _bits(w)), (L, len(u))          # the NumPy fallback
    seeded = [(u, w) for (u, _, L), w in zip(GAIN_CASES[:16], want)]
    assert sum((w < 1).any() for _, w in seeded) >= 12 and all(w.min() > 0 for _, w in seeded)     # not a vacuous pass
    assert (ses.limit_gains(_seeded(7, 300), None) == 1).all()                                      # mode 0: all 1


def test_the_named_edges(want):
    got = dict(zip(_edges(), want[16:]))
    edges = _edges()
    one = F(1.0)
    # the only loud sample first / last: the gain is lowest AT it, rises strictly over the L samples next to it and is 1
    # beyond them; nothing outside the segment pulls it further down
    g, (u, ceiling, L) = got["loud first"], edges["loud first"]
    assert g[0] == g.min() < one and (g[L + 1:] == one).all() and (np.diff(g[:L + 2]) > 0).all()
    assert abs(u[0]) * g[0] <= ceiling
    g, (u, ceiling, L) = got["loud last"], edges["loud last"]
    assert g[-1] == g.min() < one and (g[:-L - 1] == one).all() and (np.diff(g[-L - 2:]) < 0).all()
    assert abs(u[-1]) * g[-1] <= ceiling
    # c <= L: every window holds the whole segment's minimum somewhere; the bound still holds sample by sample
    for name in ("c <= L", "c == L"):
        g, (u, ceiling, L) = got[name], edges[name]
        assert len(u) <= L and (g < one).all() and (np.abs(u).astype(np.float64) * g <= ceiling * (1 + 2.0 ** -22)).all()
    assert (got["all below"] == one).all()
    u, ceiling, L = edges["at the ceiling"]
    assert ref.q_of(u, ceiling)[100] == 65536 and (got["at the ceiling"] == one).all()
    u, ceiling, L = edges["huge"]
    assert ref.q_of(u, ceiling)[200] == 0 and got["huge"][200] == 0 and (got["huge"][200 - L:200 + L + 1] < one).all()
    assert (got["huge"][:200 - L] == one).all() and (got["huge"][200 + L + 1:] == one).all()
    # the window is symmetric: a lone peak's gains mirror around it
    lone = np.full(401, 0.1, F)
    lone[200] = 2.0
    g = ref.gains(lone, Limit(0.5, 50))
    assert np.array_equal(g, g[::-1]) and (g[:150] == one).all() and g[150] < one and g[200] == g.min()
    # in exact arithmetic g <= ceiling / |u|: the clamp only absorbs rounding
    u = _seeded(255, 5000)
    v = u.astype(np.float64) * ref.gains(u, Limit(0.7, 255))
    assert np.abs(v).max() <= 0.7 * (1 + 2.0 ** -22) and np.abs(ref.apply(u, Limit(0.7, 255))).max() <= F(0.7)


# ------------------------------------------------------------------ the validation

@pytest.mark.parametrize("name", sorted(ref.LIMIT_REFUSALS))
def test_refusals_name_the_segment_and_the_value(driver, name):
    lines, _ = driver
    limits, vol, index, words = ref.LIMIT_REFUSALS[name]
    assert [ref.limit_bad(l, vol if g == 1 and vol is not None else 1.0) for g, l in enumerate(limits)].index(True) == index
    msgs = [lines[sorted(ref.LIMIT_REFUSALS).index(name)]["check"]]
    segs = [ses.Segment(g, volume=vol if g == 1 and vol is not None else 1.0) for g in range(len(limits))]
    with pytest.raises(SessionError, match=r"\[-3\]") as exc:
        ses.limit_check(ses.RawLimits(limits), segs)
    msgs.append(str(exc.value))
    for msg in msgs:
        assert all(w in msg for w in words) and f"segment {index}: " in msg, msg
    assert msgs[1].endswith(msgs[0])           # (the library's message is limit.hpp's)
    if vol is not None:                         # without the segments the volumes are not looked at
        ses.limit_check(ses.RawLimits(limits))


def test_what_is_not_refused():
    ses.limit_check(None, n=3)
    ses.limit_check([ses.Limit(1.0, 1), None, ses.Limit(2.0 ** -20, 1024)], [ses.Segment(0, volume=1024.0), ses.Segment(1, volume=5000.0),
                                                                            ses.Segment(2, volume=-1024.0)])
    ses.limit_check(ses.RawLimits([(0, 0.0, 0, 0), (0, 7.0, -5, 0)]))           # an off limit's ceiling and lookahead are not read
    with pytest.raises(SessionError, match="one Limit or one per segment"):
        ses._limits([ses.Limit()] * 2, 3)
    with pytest.raises(SessionError, match="segment 1: limit"):
        ses._limits([None, ses.Limit("loud", 3)], 2)
    for bad in (ses.RawLimits([(1, 0.5, 0, 0)]), ses.RawLimits([(1, 1.5, 8, 0)]), ses.RawLimits([(3, 0.5, 8, 0)])):
        with pytest.raises(SessionError, match="vits_limit_gains"):
            ses.limit_gains(np.zeros(4, F), bad)


def test_abi_surface():
    lib = _ffi.load()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_limit_check", "vits_limit_gains", "vits_deliver_limited", "vits_test_deliver_limited"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert C.sizeof(_ffi.VitsLimit) == 16
    assert "limited delivery" in header and re.search(r"#define VITS_LIMIT_MAX_LOOKAHEAD 1024\b", header)
    assert not re.search(r"crossfades that overlap two segments; a\s*\*?\s*limiter", header)    # the older section points to the new one
    from conftest import GOLDEN
    from phoonnx_amd import MiSession
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    with pytest.raises(SessionError, match="host-only"):
        s.deliver([ses.Segment(0)], 1, "pcm16", limits=ses.Limit(0.5, 8))
    s.close()


# ------------------------------------------------------------------ the driver itself

def test_the_driver_runs_clean_under_the_sanitizers(tmp_path, driver):
    """The stand-alone program itself, built with -fsanitize=address,undefined (nothing loaded into Python is sanitised)."""
    lines, cases = driver
    exe = str(tmp_path / "limit_driver_san")
    _build(exe, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert [json.loads(ln) for ln in r.stdout.splitlines()] == lines


def test_the_limiter_has_a_walk_of_its_own(driver):
    walks = [d for d in driver[0] if "walk" in d]
    assert [d["walk"] for d in walks] == [1, 3, 32, 256]
    for d in walks:
        need = d["record"] * d["walk"] + 4 * d["walk"] * 4097
        assert d["ok"] == 1 and d["record"] == 16 and need <= d["with_limit"] - d["shape"] <= need + 2 * 256, d


# ------------------------------------------------------------------ the NumPy fallback

def _loud_rows():
    """the rows of test_trim_cpu, three times as loud: with a volume of 0.8 and a ceiling of 0.5 the limiter works"""
    return [np.asarray(r, F) * F(3.0) for r in _rows()]


def _padded(rows):
    x = np.full((len(rows), max(len(r) for r in rows) + 3), np.nan, F)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, [len(r) for r in rows]


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_the_limited_fallback_equals_the_reference(encoding):
    rows = _loud_rows()
    x, counts = _padded(rows)
    shapes = [sref.Shape(10, 20, 1, ((5, 0.5), (40, 2.0), (41, 0.25))), sref.NONE, sref.Shape(8, 8, 0, ()), sref.NONE, sref.NONE,
              sref.Shape(0, 30, 1, ((0, 0.0), (100, 1.5)))]
    mine = [ses.Shape(s.fade_in, s.fade_out, ("linear", "smooth")[s.curve], tuple(s.points)) for s in shapes]
    limits = [Limit(0.5, 7), Limit(0.25, 1), None, Limit(0.5, 255), Limit(0.5, 3), Limit(0.6, 1024)]
    changed = 0
    for trim in (Trim(2, 0.25, 0, 0, 0), Trim(1, 0.1, 7, 200, 3), None):
        tail = trim.tail_samples if trim else 0
        for lead, norm, vol in ((0, 1, 1.0), (4, 2, 0.8), (1, 0, 2.5)):
            segs = [Seg(b, 0, lead, norm, F(vol)) for b in range(len(rows))]
            trims = [trim or tref.OFF] * len(rows)
            for sh_ref, sh_mine in ((shapes, mine), (None, None)):
                w, kept, _ = ref.deliver_ref(x, counts, segs, trims, None, sh_ref, limits, 1, encoding)
                got, k2 = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, shapes=sh_mine, limits=limits)
                assert got.tobytes() == w[0] and k2 == kept
                changed += got.tobytes() != ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, shapes=sh_mine)[0].tobytes()
            one, _ = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, limits=ses.Limit(0.5, 7))    # one limit for every row
            assert one.tobytes() == ref.deliver_ref(x, counts, segs, trims, None, None, [Limit(0.5, 7)] * len(rows), 1, encoding)[0][0]
    assert changed == 18
    # levelled: the loudness and the gain are those of the unlimited audio; shape and limiter come behind the gain
    fs = 8000
    long_rows = [lref.sine(fs, 440.0, 0.6, 0.2), lref.sine(fs, 300.0, 0.5, 0.05)]
    lv = ses.Level(1, -6.0, 30.0, 0.0)                                      # (a target the sines only reach above full scale)
    sh = [sref.Shape(100, 300, 1, ((1000, 1.0), (1200, 0.5))), sref.NONE]
    lm = [Limit(0.5, 40), Limit(0.3, 110)]
    base = ae.join_leveled(long_rows, fs, lv, encoding, 2, 3, None, 0.9)
    got = ae.join_leveled(long_rows, fs, lv, encoding, 2, 3, None, 0.9, shapes=[ses.Shape(100, 300, "smooth", ((1000, 1.0), (1200, 0.5))), ses.Shape()],
                          limits=lm)
    assert got[2] == base[2] and [_bits(g) for g in got[3]] == [_bits(g) for g in base[3]] and got[1] == base[1]
    xl, cl = _padded(long_rows)
    segs = [Seg(b, 0, 2, 0, F(0.9)) for b in range(2)]
    w, _, vals = ref.deliver_ref(xl, cl, segs, [Trim(0, 0.0, 0, 0, 3)] * 2, [lref.Level(1, -6.0, 30.0, 0.0)] * 2, sh, lm, 1, encoding,
                                 level_gains=got[3])
    assert got[0].tobytes() == w[0] and got[0].tobytes() != base[0].tobytes()
    assert all(np.abs(v).max() <= F(l.ceiling) for v, l in zip(vals, lm)) and all(float(g) * 0.9 * np.abs(r).max() > l.ceiling
                                                                                  for g, r, l in zip(got[3], long_rows, lm))
    with pytest.raises(ValueError, match="one limit or one per row"):
        ae.join_trimmed(rows, encoding, limits=[ses.Limit()] * 2)
    with pytest.raises(ValueError, match="lookahead"):
        ae.limit_gains(np.zeros(4, F), 0.5, 1025)
    with pytest.raises(ValueError, match="ceiling"):
        ae.limit_gains(np.zeros(4, F), 0.0, 8)


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_with_limits_off_the_fallback_is_what_it_was(encoding):
    rows = _loud_rows()
    for trim in (Trim(2, 0.25, 0, 0, 0), None):
        for lead, norm, vol in ((0, 1, 1.0), (1, 0, 2.5)):
            tail = trim.tail_samples if trim else 0
            base, kept = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol)
            for limits in (None, [None] * len(rows), ses.Limit(1.0, 110) if norm else None):    # (normalised: nothing reaches 1.0)
                got, k2 = ae.join_trimmed(rows, encoding, lead, tail, trim, norm, vol, limits=limits)
                assert got.tobytes() == base.tobytes() and k2 == kept and got.dtype == base.dtype
    fs = 8000
    long_rows = [lref.sine(fs, 440.0, 0.6, 0.2)]
    base = ae.join_leveled(long_rows, fs, ses.Level(1, -30.0, 30.0, 0.0), encoding, 2, 3, None, 0.9)
    for limits in (None, [None], ses.Limit(0.99, 64)):                                          # (-30 LUFS: far below 0.99)
        got = ae.join_leveled(long_rows, fs, ses.Level(1, -30.0, 30.0, 0.0), encoding, 2, 3, None, 0.9, limits=limits)
        assert got[0].tobytes() == base[0].tobytes() and got[1:3] == base[1:3]


# ------------------------------------------------------------------ the voice layer on stand-in sessions

class _Limiting(_Stub):
    """A session that delivers: the plan, the trim and the limits it is given, applied by the reference to the same waveforms"""

    def __init__(self):
        self.calls = []

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16", seeds=None,
                             return_durations=False, trim=None, limits=None):
        r = self.synthesize_batch(ids, lens, scales, sid, seeds=seeds, return_durations=return_durations)
        counts = r["y_lengths"] * self.HOP
        self.calls.append(limits)
        trims = [tref.OFF if trim is None else Trim(trim.mode, trim.threshold, trim.keep_lead, trim.keep_tail, trim.tail_samples)] * len(segments)
        lims = None if limits is None else [Limit(limits.ceiling, limits.lookahead)] * len(segments)
        got, kept, _ = ref.deliver_ref(r["output"][:, 0, 0, :], counts, segments, trims, None, None, lims, n_streams, encoding)
        streams = [np.frombuffer(b, ref.dref.DTYPE[encoding]) for b in got]
        out = {"streams": streams, "stream_samples": np.array([len(a) for a in streams]), "y_lengths": r["y_lengths"],
               "sample_lengths": counts, "kept_first": np.array([a for a, _ in kept]), "kept_count": np.array([c for _, c in kept])}
        if return_durations:
            out["durations"] = r["durations"]
        return out


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_synthesize_encoded_limits_on_stand_in_sessions(encoding):
    cfg = SynthesisConfig(speaker_id=2, volume=0.8, normalize_audio=True)
    host, dev = _voice(_Stub()), _voice(_Limiting())
    kw = dict(encoding=encoding, sentence_silence=0.01, trim_silence=0.25, trailing_silence=0.02)
    plain = host.synthesize_encoded(TEXT, cfg, **kw)
    for more, L in ((dict(limit_ceiling=0.5), 80), (dict(limit_ceiling=0.25, limit_lookahead=0.001), 16)):     # round(16000 * s)
        a, d = host.synthesize_encoded(TEXT, cfg, **kw, **more), dev.synthesize_encoded(TEXT, cfg, **kw, **more)
        assert a.tobytes() == d.tobytes() != plain.tobytes()
        assert a.sentence_starts == d.sentence_starts == plain.sentence_starts and a.sentence_samples == plain.sentence_samples
        lim = dev.session.calls[-1]
        assert isinstance(lim, ses.Limit) and (lim.ceiling, lim.lookahead) == (more["limit_ceiling"], L)
        if encoding == "f32":
            assert np.abs(a.data).max() <= F(more["limit_ceiling"]) < np.abs(plain.data).max()
    # the default: no keyword reaches the session - one that has never heard of limits still serves - and the bytes are the
    # call's without a limiter
    base = dev.synthesize_encoded(TEXT, cfg, **kw)
    assert dev.session.calls[-1] is None and base.tobytes() == plain.tobytes()
    old = _voice(_Shaping())
    assert old.synthesize_encoded(TEXT, cfg, **kw, limit_ceiling=0.0).tobytes() == plain.tobytes()
    with pytest.raises(TypeError, match="limits"):
        old.synthesize_encoded(TEXT, cfg, **kw, limit_ceiling=0.5)
    for bad, words in ((dict(limit_ceiling=1.5), ("1.5",)), (dict(limit_ceiling=-0.1), ("-0.1",)), (dict(limit_ceiling=float("nan")), ("nan",)),
                       (dict(limit_ceiling=0.5, limit_lookahead=0.1), ("0.1", "1600")), (dict(limit_ceiling=0.5, limit_lookahead=0.0), ("0.0", "0 samples")),
                       (dict(limit_ceiling=0.5, limit_lookahead=float("inf")), ("inf",))):
        with pytest.raises(ValueError) as exc:
            host.synthesize_encoded(TEXT, cfg, **bad)
        assert all(w in str(exc.value) for w in words), str(exc.value)


@pytest.mark.parametrize("encoding", ["ulaw", "f32"])
def test_synthesize_requests_encoded_limits_on_stand_in_sessions(encoding):
    texts = ["the quick brown fox. jumps over", "a lazy dog sleeps in the sun. all day long", "hello there"]
    cfgs = [SynthesisConfig(speaker_id=i, volume=(1.0, 0.5, 2.0)[i], normalize_audio=i != 1) for i in range(3)]
    reqs = list(zip(texts, cfgs))
    host, dev = _voice(_Stub()), _voice(_Limiting())
    for trim in (0.25, None):
        kw = dict(max_batch=4, encoding=encoding, sentence_silence=0.01, trim_silence=trim, trailing_silence=0.02 if trim else 0.0)
        plain = host.synthesize_requests_encoded(reqs, **kw)
        a = host.synthesize_requests_encoded(reqs, **kw, limit_ceiling=0.4, limit_lookahead=0.002)
        d = dev.synthesize_requests_encoded(reqs, **kw, limit_ceiling=0.4, limit_lookahead=0.002)
        lim = dev.session.calls[-1]
        assert isinstance(lim, ses.Limit) and (lim.ceiling, lim.lookahead) == (0.4, 32)
        for r in range(3):
            assert a[r].tobytes() == d[r].tobytes()
            assert a[r].sentence_starts == plain[r].sentence_starts and a[r].sentence_samples == plain[r].sentence_samples
            if encoding == "f32":
                assert np.abs(a[r].data).max() <= F(0.4)
        assert any(a[r].tobytes() != plain[r].tobytes() for r in range(3))
        assert [p.tobytes() for p in dev.synthesize_requests_encoded(reqs, **kw)] == [p.tobytes() for p in plain]
        assert dev.session.calls[-1] is None
