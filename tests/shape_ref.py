"""An independent NumPy float32 statement of the shaped delivery (include/vitsmi.h, "shaped delivery"): the multiplier of every
kept sample - envelope, fades, their product -, the refusals, and the byte streams.  Nothing here imports the package; the
sample formula's front and the encoders are delivery_ref's, the kept ranges trim_ref's, the gains loudness_ref's.

A shape is anything with the attributes fade_in, fade_out, curve (0 linear, 1 smooth), points ((pos, gain) pairs); Shape
below.  Every operation is one on np.float32 scalars or arrays, so each is rounded to float32 by itself."""
from collections import namedtuple

import numpy as np

import delivery_ref as dref
import loudness_ref as lref
import trim_ref as tref
from delivery_ref import INT_MAX, SILENCE, Seg
from loudness_ref import Level
from trim_ref import Trim

Shape = namedtuple("Shape", "fade_in fade_out curve points")
NONE = Shape(0, 0, 0, ())
F = np.float32
MIN_GAIN = 2.0 ** -20
MAX_POINTS = 1 << 20


def curve(t, kind):
    t = np.asarray(t, F)
    if kind == 0:
        return t
    tt = (t * t).astype(F)
    two_t = (F(2.0) * t).astype(F)
    return (tt * (F(3.0) - two_t).astype(F)).astype(F)


def envelope(a, c, points):
    """e of row samples a .. a + c - 1, interval by interval"""
    e = np.ones(c, F)
    if not len(points):
        return e
    pos = [int(p) for p, _ in points]
    g = [F(v) for _, v in points]
    i = a + np.arange(c, dtype=np.int64)
    e[:] = g[-1]                                    # i >= p_{m-1}
    e[i <= pos[0]] = g[0]
    for k in range(len(pos) - 1):
        m = (i >= pos[k]) & (i < pos[k + 1]) & (i > pos[0])
        if not m.any():
            continue
        s = F(F(g[k + 1] - g[k]) / F(pos[k + 1] - pos[k]))
        d = (i[m] - pos[k]).astype(F)
        e[m] = (g[k] + (s * d).astype(F)).astype(F)
    return e


def multiplier(a, c, shape):
    """float32 [c]: mul of the kept samples j = 0 .. c - 1 (row samples a + j)"""
    a, c = int(a), int(c)
    j = np.arange(c, dtype=np.int64)
    w_in, w_out = np.ones(c, F), np.ones(c, F)
    if shape.fade_in > 0:
        m = j < shape.fade_in
        w_in[m] = curve((j[m].astype(F) / F(shape.fade_in)).astype(F), shape.curve)
    if shape.fade_out > 0:
        r = c - 1 - j
        m = r < shape.fade_out
        w_out[m] = curve((r[m].astype(F) / F(shape.fade_out)).astype(F), shape.curve)
    e = envelope(a, c, shape.points)
    return ((e * w_in).astype(F) * w_out).astype(F)


def gain_bad(g):
    g = float(g)
    return not np.isfinite(g) or g < 0 or 0 < g < MIN_GAIN or g > 64


def check_shapes(shapes, points, n_points):
    """The raw form (records of (fade_in, fade_out, curve, n_points, first_point) over one point array whose stated count
    is n_points): ValueError("segment g") / ValueError("segment g point k") for the first thing the definition refuses,
    ValueError("call") for the point count."""
    if not 0 <= n_points <= MAX_POINTS:
        raise ValueError("call")
    for g, (fi, fo, cv, n, first) in enumerate(shapes):
        if fi < 0 or fo < 0 or cv not in (0, 1) or n < 0 or first < 0 or first + n > n_points:
            raise ValueError(f"segment {g}")
        for k in range(n):
            pos, gain = points[first + k]
            if not 0 <= pos <= INT_MAX or (k > 0 and pos <= points[first + k - 1][0]) or gain_bad(gain):
                raise ValueError(f"segment {g} point {k}")


def deliver_ref(x, counts, segments, trims, levels, shapes, n_streams, encoding, gains=None):
    """x [B, S] float32 -> ([bytes per stream], kept [(a, c)]).  gains: the levelled segments' (float32 [G]; None: none is
    levelled).  Peaks and kept ranges are those of the unshaped audio."""
    trims = trims if trims is not None else [tref.OFF] * len(segments)
    levels = levels if levels is not None else [lref.OFF] * len(segments)
    shapes = shapes if shapes is not None else [NONE] * len(segments)
    x = np.asarray(x, F)
    kept = [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segments, trims)]
    rows = {s.row: x[s.row, a:a + c] for s, (a, c) in zip(segments, kept)}
    peak_row = {r: (np.max(np.abs(v)) if v.size else F(0)) for r, v in rows.items()}
    out = []
    for j in range(n_streams):
        mine = [(g, s, t) for g, (s, t) in enumerate(zip(segments, trims)) if s.stream == j]
        scope2 = [peak_row[s.row] for _, s, _ in mine if s.normalize == 2]
        peak_stream = max(scope2) if scope2 else None
        parts = []
        for g, s, t in mine:
            v = rows[s.row]
            if levels[g].mode:
                v = (v * F(gains[g])).astype(F)
            elif s.normalize:
                peak = peak_row[s.row] if s.normalize == 1 else peak_stream
                v = np.zeros_like(v) if F(peak) < F(1e-8) else (v / F(peak)).astype(F)
            if F(s.volume) != F(1.0):
                v = (v * F(s.volume)).astype(F)
            v = (v * multiplier(*kept[g], shapes[g])).astype(F)
            v = np.minimum(np.maximum(v, F(-1.0)), F(1.0)).astype(F)
            parts += [SILENCE[encoding] * int(s.lead_samples), dref.encode(v, encoding), SILENCE[encoding] * int(t.tail_samples)]
        out.append(b"".join(parts))
    return out, kept


# ---- what the definition refuses, on delivery_ref.GOOD (three segments) over delivery_ref.COUNTS, in the raw form.
# name -> (shape records, points, the call's stated point count, segment the message names or None, words of the message)
_N = (0, 0, 0, 0, 0)
_PTS = [(0, 1.0), (3, 0.5), (4, 2.0), (9, 0.0)]
SHAPE_REFUSALS = {
    "fade_in negative": ([_N, (-1, 0, 0, 0, 0), _N], [], 0, 1, ("fade_in -1",)),
    "fade_out negative": ([_N, _N, (0, -3, 1, 0, 0)], [], 0, 2, ("fade_out -3",)),
    "curve 2": ([(1, 1, 2, 0, 0), _N, _N], [], 0, 0, ("curve 2",)),
    "curve -1": ([_N, (1, 1, -1, 0, 0), _N], [], 0, 1, ("curve -1",)),
    "n_points negative": ([_N, _N, (0, 0, 0, -2, 0)], _PTS, 4, 2, ("n_points -2",)),
    "first_point negative": ([(0, 0, 0, 2, -1), _N, _N], _PTS, 4, 0, ("-1",)),
    "points beyond the call's": ([_N, (0, 0, 0, 3, 2), _N], _PTS, 4, 1, ("[2, +3)", "4 points")),
    "too many points": ([_N, _N, _N], _PTS, MAX_POINTS + 1, None, (f"n_points = {MAX_POINTS + 1}",)),
    "call's count negative": ([_N, _N, _N], _PTS, -1, None, ("n_points = -1",)),
    "pos negative": ([_N, _N, (0, 0, 0, 2, 0)], [(-5, 1.0), (3, 1.0)], 2, 2, ("point 0", "pos -5")),
    "pos equal": ([(0, 0, 0, 3, 0), _N, _N], [(1, 1.0), (7, 1.0), (7, 0.5)], 3, 0, ("point 2", "pos 7")),
    "pos descends": ([_N, (0, 0, 0, 2, 1), _N], [(0, 1.0), (8, 1.0), (6, 0.5)], 3, 1, ("point 1", "pos 6")),
    "gain nan": ([(0, 0, 0, 1, 0), _N, _N], [(2, float("nan"))], 1, 0, ("point 0", "gain nan")),
    "gain inf": ([_N, _N, (0, 0, 0, 2, 0)], [(2, 1.0), (5, float("inf"))], 2, 2, ("point 1", "gain inf")),
    "gain negative": ([_N, (0, 0, 0, 1, 0), _N], [(2, -0.5)], 1, 1, ("point 0", "gain -0.5")),
    "gain below 2^-20": ([(0, 0, 0, 1, 0), _N, _N], [(2, 2.0 ** -21)], 1, 0, ("point 0", "gain 4.76837e-07")),
    "gain above 64": ([_N, _N, (0, 0, 0, 1, 0)], [(2, 64.5)], 1, 2, ("point 0", "gain 64.5")),
}


# ---- the by-value batch of the device test and of the driver: one row for each way the shaped pack can go wrong
RATE = 8000


def batch():
    """-> (x [B, S] float32, counts, segments, trims, levels, shapes, n_streams).  Every sample is 0 or at least 0.05 in
    magnitude (so no product with a gain >= 2^-20 and a fade weight is subnormal); NaN behind every row's end."""
    rng = np.random.default_rng(515)
    rows, segs, trims, levels, shapes = [], [], [], [], []

    def loud(n, lo=0.05, hi=0.9):
        return (rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)).astype(F)

    def add(row, stream, shape, lead=0, normalize=0, volume=1.0, trim=tref.OFF, level=lref.OFF):
        rows.append(np.asarray(row, F))
        segs.append(Seg(len(rows) - 1, stream, lead, normalize, volume))
        trims.append(trim)
        levels.append(level)
        shapes.append(shape)

    # stream 0: odd lengths, so that the segment boundaries fall inside 16-byte cells; the middle one has NO shape
    add(loud(37), 0, Shape(5, 5, 0, ()))                                                   # 0
    add(loud(23), 0, NONE)                                                                 # 1: no shape between shaped neighbours
    add(loud(3000), 0, Shape(441, 1000, 0, ()), volume=0.8)                                # 2: fades only, linear
    add(loud(3000), 0, Shape(441, 1000, 1, ()), lead=3)                                    # 3: the same fades, smooth
    add(loud(100), 0, Shape(80, 70, 1, ()))                                                # 4: fade_in + fade_out > c
    # stream 1: the short rows, c = 0, 1, 2 with fades of 1 and of 5
    add(loud(0), 1, Shape(1, 5, 0, ()))                                                    # 5
    add(loud(1), 1, Shape(1, 5, 0, ()))                                                    # 6
    add(loud(2), 1, Shape(5, 1, 1, ()), trim=Trim(0, 0.0, 0, 0, 2))                        # 7
    # stream 2: points only.  Row 8 has 9000 samples - more than one tile in every encoding - with two points one sample
    # apart, 600 points 1 to 3 samples apart (a lane's next pass, 256 samples on, steps over a hundred of them) and points
    # beyond the row's end; row 9 a single point
    pos = [700, 701]
    gains = [0.25, 1.5]
    p = 4000
    for _ in range(600):
        p += int(rng.integers(1, 4))
        pos.append(p)
        gains.append(float(F(rng.uniform(0.1, 2.0))))
    pos += [8000, 9500, 20000]
    gains += [1.0, 0.5, 3.0]
    add(loud(9000, 0.05, 0.4), 2, Shape(0, 0, 0, tuple(zip(pos, gains))))                  # 8
    add(loud(50), 2, Shape(0, 0, 0, ((10, 0.5),)))                                         # 9
    # stream 3: points, fades and a trim with a > 0: points in front of a, inside, and behind a + c
    r = loud(2000, 0.3, 0.9)
    r[:300] = 0.0
    r[1700:] = 0.0
    add(r, 3, Shape(60, 90, 1, ((100, 2.0), (250, 0.5), (330, 1.0), (900, 0.25), (1600, 1.5), (1900, 0.125), (2500, 4.0))),
        normalize=1, trim=Trim(1, 0.1, 20, 30, 5))                                         # 10
    # stream 4: a levelled segment with a shape (half a second at 8 kHz)
    t = np.arange(4400) / RATE
    add((0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.1).astype(F), 4, Shape(100, 200, 0, ((1000, 1.0), (1400, 0.5))),
        level=Level(1, -20.0, 30.0, 0.0))                                                  # 11
    # stream 5 / 6: normalize 1 and normalize 2 with shapes: the peaks are those of the unshaped audio
    add(loud(300, 0.05, 0.5), 5, Shape(0, 0, 0, ((0, 0.5), (299, 1.0))), normalize=1)      # 12
    add(loud(400, 0.05, 0.3), 6, Shape(50, 50, 0, ()), normalize=2)                        # 13
    add(loud(333, 0.05, 0.6), 6, Shape(0, 40, 1, ((100, 0.75),)), normalize=2, lead=2)     # 14
    # stream 7: a gain-0 plateau, and a gain of 4 that clips
    add(loud(300), 7, Shape(0, 0, 0, ((100, 1.0), (110, 0.0), (200, 0.0), (210, 1.0))))    # 15
    add(loud(200, 0.3, 0.9), 7, Shape(0, 0, 0, ((0, 4.0),)))                               # 16
    S = max(len(r) for r in rows) + 3
    x = np.full((len(rows), S), np.nan, F)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return x, np.array([len(r) for r in rows], np.int64), segs, trims, levels, shapes, 8


def flatten(shapes):
    """shapes -> the raw form: (records, points)"""
    records, points = [], []
    for s in shapes:
        records.append((s.fade_in, s.fade_out, s.curve, len(s.points), len(points)))
        points += [(int(p), float(g)) for p, g in s.points]
    return records, points
