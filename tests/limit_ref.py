"""An independent NumPy statement of the limited delivery (include/vitsmi.h, "limited delivery"): q, M and S in int64, the two
divisions and the product in np.float32; the refusals; the byte streams.  Nothing here imports the package; the sample
formula's front and the encoders are delivery_ref's, the kept ranges trim_ref's, the gains loudness_ref's, the multiplier
shape_ref's.

A limit is anything with the attributes ceiling and lookahead (Limit below), or None: the segment is not limited."""
from collections import namedtuple

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import delivery_ref as dref
import loudness_ref as lref
import shape_ref as sref
import trim_ref as tref
from delivery_ref import SILENCE, Seg

Limit = namedtuple("Limit", "ceiling lookahead")
F = np.float32
UNITY = 65536
MAX_LOOKAHEAD = 1024
RATE = 8000


def q_of(u, ceiling):
    """int64 [c]: the gain every sample would need on its own, in units of 2^-16"""
    u = np.asarray(u, F)
    mag = np.abs(u)
    q = np.full(u.size, UNITY, np.int64)
    over = mag > F(ceiling)
    with np.errstate(over="ignore"):
        quot = (F(ceiling) / mag[over]).astype(F)
        q[over] = np.floor((quot * F(65536.0)).astype(F)).astype(np.int64)
    return q


def min_sum(q, L):
    """(M [c + L]: M[j] at index j + L, j in [-L, c);  S [c]) from q [c], window by window"""
    c = q.size
    pad = np.concatenate([np.full(L, UNITY, np.int64), q, np.full(L, UNITY, np.int64)])      # q[j] at index j + L
    M = sliding_window_view(pad, L + 1).min(axis=1)                                              # c + L windows
    S = sliding_window_view(M, L + 1).sum(axis=1) if c else np.zeros(0, np.int64)                # c windows
    return M, S


def gains(u, limit):
    """float32 [c]: g of every sample of a segment whose unlimited values are u"""
    u = np.asarray(u, F)
    if limit is None:
        return np.ones(u.size, F)
    L = int(limit.lookahead)
    _, S = min_sum(q_of(u, limit.ceiling), L)
    assert S.size == u.size and (S <= (L + 1) * UNITY).all() and (S >= 0).all()
    return (S.astype(F) / F((L + 1) * UNITY)).astype(F)


def apply(u, limit):
    """the limited values in front of the clip: one product, then the clamp to +-ceiling"""
    u = np.asarray(u, F)
    if limit is None:
        return u
    v = (u * gains(u, limit)).astype(F)
    return np.minimum(np.maximum(v, F(-limit.ceiling)), F(limit.ceiling)).astype(F)


def limit_bad(l, volume=1.0):
    """what the definition refuses of one raw limit (mode, ceiling, lookahead, reserved) on a segment of `volume`"""
    mode, ceiling, lookahead, reserved = l
    if mode not in (0, 1) or reserved != 0:
        return True
    if mode == 0:
        return False
    return not (np.isfinite(ceiling) and 0 < ceiling <= 1) or not 1 <= lookahead <= MAX_LOOKAHEAD or not abs(volume) <= 1024


def unlimited(x, counts, segments, trims, levels, shapes, n_streams, level_gains=None):
    """u of every segment (float32 [c]) and the kept ranges: shape_ref.deliver_ref's formula up to the multiplier's product"""
    trims = trims if trims is not None else [tref.OFF] * len(segments)
    levels = levels if levels is not None else [lref.OFF] * len(segments)
    shapes = shapes if shapes is not None else [sref.NONE] * len(segments)
    x = np.asarray(x, F)
    kept = [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segments, trims)]
    rows = {s.row: x[s.row, a:a + c] for s, (a, c) in zip(segments, kept)}
    peak_row = {r: (np.max(np.abs(v)) if v.size else F(0)) for r, v in rows.items()}
    u = [None] * len(segments)
    for j in range(n_streams):
        mine = [(g, s) for g, s in enumerate(segments) if s.stream == j]
        scope2 = [peak_row[s.row] for _, s in mine if s.normalize == 2]
        peak_stream = max(scope2) if scope2 else None
        for g, s in mine:
            v = rows[s.row]
            if levels[g].mode:
                v = (v * F(level_gains[g])).astype(F)
            elif s.normalize:
                peak = peak_row[s.row] if s.normalize == 1 else peak_stream
                v = np.zeros_like(v) if F(peak) < F(1e-8) else (v / F(peak)).astype(F)
            if F(s.volume) != F(1.0):
                v = (v * F(s.volume)).astype(F)
            u[g] = (v * sref.multiplier(*kept[g], shapes[g])).astype(F)
    return u, kept


def deliver_ref(x, counts, segments, trims, levels, shapes, limits, n_streams, encoding, level_gains=None):
    """x [B, S] float32 -> ([bytes per stream], kept [(a, c)], limited values per segment).  limits: one per segment (None:
    off) or None.  Peaks, kept ranges and loudness are those of the unlimited audio."""
    limits = limits if limits is not None else [None] * len(segments)
    trims_ = trims if trims is not None else [tref.OFF] * len(segments)
    u, kept = unlimited(x, counts, segments, trims, levels, shapes, n_streams, level_gains)
    vals = [np.minimum(np.maximum(apply(v, lm), F(-1.0)), F(1.0)).astype(F) for v, lm in zip(u, limits)]
    out = []
    for j in range(n_streams):
        parts = []
        for g, s in enumerate(segments):
            if s.stream == j:
                parts += [SILENCE[encoding] * int(s.lead_samples), dref.encode(vals[g], encoding),
                          SILENCE[encoding] * int(trims_[g].tail_samples)]
        out.append(b"".join(parts))
    return out, kept, vals


# ---- what the definition refuses, on delivery_ref.GOOD (three segments), in the raw form (mode, ceiling, lookahead, reserved).
# name -> (limits, the volume of segment 1 or None, the segment the message names, words of the message)
_OFF = (0, 0.0, 0, 0)
_ON = (1, 0.5, 110, 0)
LIMIT_REFUSALS = {
    "mode 2": ([_OFF, (2, 0.5, 110, 0), _OFF], None, 1, ("mode 2",)),
    "mode -1": ([(-1, 0.5, 110, 0), _OFF, _OFF], None, 0, ("mode -1",)),
    "ceiling 0": ([_OFF, _OFF, (1, 0.0, 110, 0)], None, 2, ("ceiling 0",)),
    "ceiling negative": ([_ON, (1, -0.25, 110, 0), _OFF], None, 1, ("ceiling -0.25",)),
    "ceiling above 1": ([(1, 1.5, 110, 0), _OFF, _OFF], None, 0, ("ceiling 1.5",)),
    "ceiling nan": ([_OFF, (1, float("nan"), 110, 0), _OFF], None, 1, ("ceiling nan",)),
    "ceiling inf": ([_OFF, _ON, (1, float("inf"), 110, 0)], None, 2, ("ceiling inf",)),
    "lookahead 0": ([(1, 0.5, 0, 0), _OFF, _OFF], None, 0, ("lookahead 0",)),
    "lookahead 1025": ([_OFF, (1, 0.5, 1025, 0), _OFF], None, 1, ("lookahead 1025",)),
    "lookahead negative": ([_OFF, _OFF, (1, 0.5, -3, 0)], None, 2, ("lookahead -3",)),
    "reserved": ([_OFF, (0, 0.0, 0, 7), _OFF], None, 1, ("reserved 7",)),
    "volume": ([_OFF, _ON, _OFF], 1500.0, 1, ("volume 1500",)),
    "volume negative": ([_OFF, _ON, _OFF], -1024.5, 1, ("volume -1024.5",)),
}


# ---- the by-value batch of the device test: five rows of 9000, counts that make segments cross the pack's tiles in every
# encoding and the gain kernel's; tanh(0.5 * noise) * sin under a slow swell to three times the level, so that with a ceiling
# of 0.7 about a fifth of a long segment's samples are above it
B, S, CEILING = 5, 9000, 0.7
COUNTS = np.array([9000, 4097, 1, 0, 5000], np.int64)


def batch(seed=2024):
    rng = np.random.default_rng(seed)
    t = np.arange(S)
    x = np.empty((B, S), F)
    for b in range(B):
        swell = 1.0 + 2.0 * (0.5 - 0.5 * np.cos(2 * np.pi * (t + 700 * b) / 3000.0))
        x[b] = (np.tanh(0.5 * rng.standard_normal(S)) * np.sin(2 * np.pi * t / 37.0 + b) * swell).astype(F)
    return x


def over_fraction(u, ceiling):
    u = np.asarray(u, F)
    return float((np.abs(u) > F(ceiling)).mean()) if u.size else 0.0
