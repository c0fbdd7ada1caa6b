"""An independent NumPy float64 statement of the levelled delivery (include/vitsmi.h, "levelled delivery"): the K-weighting of a
rate, the sub-block energies, the gates of ITU-R BS.1770-4, the gain, the refusals, and the byte streams given the gains.
Nothing here imports the package; the sample formula and the encoders are delivery_ref's, the kept ranges trim_ref's.

A level is anything with the attributes mode, target_lufs, max_gain_db, peak_ceiling (Level below)."""
import math
from collections import namedtuple

import numpy as np

import delivery_ref as dref
import trim_ref as tref
from delivery_ref import SILENCE

Level = namedtuple("Level", "mode target_lufs max_gain_db peak_ceiling")
OFF = Level(0, -23.0, 30.0, 0.0)

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): shelf b0 b1 b2 a1 a2, high-pass a1 a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)


def hop(fs):
    return (int(fs) + 5) // 10


def coefficients(fs):
    """(b_shelf, a_shelf, b_hp, a_hp), each three float64 values"""
    G, Q, f0 = 3.999843853973347, 0.7071752369554196, 1681.974450955533
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a1 = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    Q, f0 = 0.5003270373238773, 38.13547087602444
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return b1, a1, [1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def biquad(b, a, x):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2], from rest (direct form I, Python floats = float64)"""
    x = np.asarray(x, np.float64).tolist()
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    b0, b1, b2 = b
    _, a1, a2 = a
    for n, v in enumerate(x):
        w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, v, y1, w
        y[n] = w
    return np.array(y, np.float64)


def k_weight(x, fs):
    b1, a1, b2, a2 = coefficients(fs)
    return biquad(b2, a2, biquad(b1, a1, x))


def sub_blocks(x, fs):
    """the energies e_k of the whole sub-blocks of one kept range (float64 [n_sub])"""
    h = hop(fs)
    n_sub = len(x) // h
    y = k_weight(np.asarray(x, np.float64)[:n_sub * h], fs)
    return (y * y).reshape(n_sub, h).sum(axis=1) if n_sub else np.zeros(0)


def blocks(e, fs):
    """z_j of one row's sub-block energies"""
    e = np.asarray(e, np.float64)
    if e.size < 4:
        return np.zeros(0)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * hop(fs))


def gate(rows_e, fs):
    """rows_e: the sub-block energies of one or several rows (pooled) -> (L, blocks, absolute-gated, both gates)"""
    z = np.concatenate([blocks(e, fs) for e in rows_e]) if len(rows_e) else np.zeros(0)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return -math.inf, int(z.size), 0, 0
    gamma = -0.691 + 10.0 * math.log10(z[keep].mean()) - 10.0
    both = keep & (l > gamma)
    if not both.any():
        return -math.inf, int(z.size), int(keep.sum()), 0
    return -0.691 + 10.0 * math.log10(z[both].mean()), int(z.size), int(keep.sum()), int(both.sum())


def loudness(x, fs):
    """integrated loudness of one kept range, LUFS (-inf: no block, or none that passes)"""
    return gate([sub_blocks(x, fs)], fs)[0]


def ungated(x, fs):
    z = blocks(sub_blocks(x, fs), fs)
    return -0.691 + 10.0 * math.log10(z.mean())


def gain(L, peak, level):
    """float32"""
    if L == -math.inf:
        return np.float32(1.0)
    g = 10.0 ** ((float(np.float32(level.target_lufs)) - L) / 20.0)
    g = min(g, 10.0 ** (float(np.float32(level.max_gain_db)) / 20.0))
    if level.peak_ceiling > 0 and peak > 0:
        g = min(g, float(np.float32(level.peak_ceiling)) / float(peak))
    return np.float32(g)


def level_bad(l):
    return (l.mode not in (0, 1, 2) or not np.isfinite(l.target_lufs) or not -70 <= l.target_lufs <= 0
            or not np.isfinite(l.max_gain_db) or not 0 <= l.max_gain_db <= 120
            or not np.isfinite(l.peak_ceiling) or not 0 <= l.peak_ceiling <= 1)


def check(counts, segments, trims, levels, n_streams, encoding, fs):
    """ValueError("segment g") for the first segment the definition refuses; "rate": the sample rate"""
    tref.check(counts, segments, trims, n_streams, encoding)
    if levels is None:
        return
    first = {}
    for g, (s, l) in enumerate(zip(segments, levels)):
        if level_bad(l) or (l.mode and s.normalize != 0):
            raise ValueError(f"segment {g}")
        if l.mode == 2:
            o = first.setdefault(s.stream, l)
            if (np.float32(o.target_lufs), np.float32(o.max_gain_db), np.float32(o.peak_ceiling)) != (
                    np.float32(l.target_lufs), np.float32(l.max_gain_db), np.float32(l.peak_ceiling)):
                raise ValueError(f"segment {g}")
    if any(l.mode for l in levels) and not 8000 <= fs <= 192000:
        raise ValueError("rate")


def measure(x, counts, segments, trims, levels, n_streams, fs):
    """-> (loudness float64 [G] (NaN at mode 0), gain float32 [G], kept [(a, c)]) of the plan, all in float64 from x"""
    trims = trims if trims is not None else [tref.OFF] * len(segments)
    levels = levels if levels is not None else [OFF] * len(segments)
    x = np.asarray(x, np.float32)
    kept = [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segments, trims)]
    loud = np.full(len(segments), np.nan)
    gn = np.ones(len(segments), np.float32)
    rows = [x[s.row, a:a + c] for s, (a, c) in zip(segments, kept)]
    peaks = [np.max(np.abs(v)) if v.size else np.float32(0) for v in rows]
    e = [sub_blocks(v, fs) if l.mode else None for v, l in zip(rows, levels)]
    for g, l in enumerate(levels):
        if l.mode == 1:
            loud[g] = gate([e[g]], fs)[0]
            gn[g] = gain(loud[g], peaks[g], l)
    for j in range(n_streams):
        mine = [g for g, (s, l) in enumerate(zip(segments, levels)) if s.stream == j and l.mode == 2]
        if not mine:
            continue
        L = gate([e[g] for g in mine], fs)[0]
        gj = gain(L, max(peaks[g] for g in mine), levels[mine[0]])
        for g in mine:
            loud[g], gn[g] = L, gj
    return loud, gn, kept


def postprocess(v, g, volume):
    """a levelled segment's samples: one float32 product with the gain, the volume's, the clip"""
    v = (np.asarray(v, np.float32) * np.float32(g)).astype(np.float32)
    return dref.postprocess(v, None, volume)


def deliver_ref(x, counts, segments, trims, levels, n_streams, encoding, gains):
    """The byte streams of a levelled delivery whose gains are given (float32 [G]; the device's, or measure()'s): x [B, S]
    float32 -> [bytes per stream].  Unlevelled segments: trim_ref.deliver_ref's formula."""
    trims = trims if trims is not None else [tref.OFF] * len(segments)
    levels = levels if levels is not None else [OFF] * len(segments)
    x = np.asarray(x, np.float32)
    kept = [tref.trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segments, trims)]
    rows = {s.row: x[s.row, a:a + c] for s, (a, c) in zip(segments, kept)}
    peak_row = {r: (np.max(np.abs(v)) if v.size else np.float32(0)) for r, v in rows.items()}
    out = []
    for j in range(n_streams):
        mine = [(g, s, t) for g, (s, t) in enumerate(zip(segments, trims)) if s.stream == j]
        scope2 = [peak_row[s.row] for _, s, _ in mine if s.normalize == 2]
        peak_stream = max(scope2) if scope2 else None
        parts = []
        for g, s, t in mine:
            if levels[g].mode:
                v = postprocess(rows[s.row], gains[g], s.volume)
            else:
                peak = None if s.normalize == 0 else (peak_row[s.row] if s.normalize == 1 else peak_stream)
                v = dref.postprocess(rows[s.row], peak, s.volume)
            parts += [SILENCE[encoding] * int(s.lead_samples), dref.encode(v, encoding), SILENCE[encoding] * int(t.tail_samples)]
        out.append(b"".join(parts))
    return out


def gating_signal(fs, seconds=4.0):
    """The gating signal: 0.7 sin(2 pi 220 t) + 0.3 N(0, 1) (default_rng(11)), amplitude 0.25 except 1e-5 on [0, 0.5 s) and
    0.25 * 10^(-25/20) on [2.5, 3.3 s).  37 blocks, 35 pass the absolute gate, 30 both."""
    n = int(round(seconds * fs))
    t = np.arange(n) / fs
    s = 0.7 * np.sin(2 * np.pi * 220.0 * t) + 0.3 * np.random.default_rng(11).standard_normal(n)
    amp = np.full(n, 0.25)
    amp[t < 0.5] = 1e-5
    amp[(t >= 2.5) & (t < 3.3)] = 0.25 * 10.0 ** (-25.0 / 20.0)
    return (amp * s).astype(np.float32)


def sine(fs, f=997.0, seconds=2.0, amplitude=1.0):
    return (amplitude * np.sin(2 * np.pi * f * np.arange(int(seconds * fs)) / fs)).astype(np.float32)


# ---- the levels the definition refuses, on delivery_ref.GOOD over delivery_ref.COUNTS with normalize 0 everywhere but where
# a case says otherwise.  name -> (normalize per segment, levels, rate, the segment the message names or None, a word of it)
_G = Level(1, -19.0, 30.0, 0.0)
_S = Level(2, -19.0, 30.0, 0.5)
LEVEL_REFUSALS = {
    "mode 3": ((0, 0, 0), [_G, Level(3, -19.0, 30.0, 0.0), OFF], 22050, 1, "mode 3"),
    "mode -1": ((0, 0, 0), [Level(-1, -19.0, 30.0, 0.0), OFF, OFF], 22050, 0, "mode -1"),
    "target nan": ((0, 0, 0), [OFF, OFF, Level(1, float("nan"), 30.0, 0.0)], 22050, 2, "target_lufs nan"),
    "target above 0": ((0, 0, 0), [Level(1, 0.5, 30.0, 0.0), OFF, OFF], 22050, 0, "target_lufs 0.5"),
    "target below -70": ((0, 0, 0), [OFF, Level(2, -71.0, 30.0, 0.0), OFF], 22050, 1, "target_lufs -71"),
    "max gain negative": ((0, 0, 0), [OFF, OFF, Level(1, -19.0, -1.0, 0.0)], 22050, 2, "max_gain_db -1"),
    "max gain inf": ((0, 0, 0), [Level(1, -19.0, float("inf"), 0.0), OFF, OFF], 22050, 0, "max_gain_db inf"),
    "max gain above 120": ((0, 0, 0), [OFF, Level(1, -19.0, 121.0, 0.0), OFF], 22050, 1, "max_gain_db 121"),
    "ceiling negative": ((0, 0, 0), [OFF, OFF, Level(1, -19.0, 30.0, -0.25)], 22050, 2, "peak_ceiling -0.25"),
    "ceiling above 1": ((0, 0, 0), [Level(2, -19.0, 30.0, 1.5), OFF, OFF], 22050, 0, "peak_ceiling 1.5"),
    "ceiling nan": ((0, 0, 0), [OFF, Level(1, -19.0, 30.0, float("nan")), OFF], 22050, 1, "peak_ceiling nan"),
    "levelled and normalised": ((0, 2, 0), [OFF, _G, OFF], 22050, 1, "normalize 2"),
    "stream disagrees in target": ((0, 0, 0), [OFF, _S, Level(2, -16.0, 30.0, 0.5)], 22050, 2, "-16"),
    "stream disagrees in max gain": ((0, 0, 0), [OFF, _S, Level(2, -19.0, 20.0, 0.5)], 22050, 2, "20 dB"),
    "stream disagrees in ceiling": ((0, 0, 0), [OFF, _S, Level(2, -19.0, 30.0, 0.25)], 22050, 2, "ceiling 0.25"),
    "rate below 8000": ((0, 0, 0), [_G, OFF, OFF], 7999, None, "sample_rate 7999"),
    "rate above 192000": ((0, 0, 0), [OFF, OFF, _G], 192001, None, "sample_rate 192001"),
}
