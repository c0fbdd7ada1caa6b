"""An independent NumPy statement of the trimmed encoded stream (include/vitsmi.h, "trimmed streaming"): the first active
sample f_b and the start a_b of every row from the rule over a given piece list, and the expected bytes composed from the
existing references - a row is a segment of the limited delivery with kept range [a_b, n_b), peak := ref_peak[b], no level
gain: shape_ref's multiplier, limit_ref's gains, delivery_ref's encoders.  Nothing here imports the package, and nothing here
states the sample formula a second time.

An onset is anything with mode, threshold, keep_lead (Onset below) or None (the row is not trimmed)."""
from collections import namedtuple

import numpy as np

import delivery_ref as dref
import limit_ref as lref
import shape_ref as sref
import stream_shape_ref as ssref
import trim_ref as tref
from delivery_ref import SILENCE, WIDTH

F = np.float32
INT_MAX = 2 ** 31 - 1
Onset = namedtuple("Onset", "mode threshold keep_lead")


def threshold(onset, ref_peak):
    """thr of a row: mode 1 the threshold, mode 2 one fp32 product with the row's ref_peak"""
    if onset.mode == 2:
        return F(F(onset.threshold) * F(ref_peak))
    return F(onset.threshold)


def first_active(row, n, thr):
    """f_b: the first i < n with |row[i]| > thr (strict, on the raw sample), or None"""
    idx = np.flatnonzero(np.abs(np.asarray(row, F)[:int(n)]) > F(thr))
    return int(idx[0]) if idx.size else None


def onset_start(f, keep_lead, delivered_before):
    """a_b = max(f_b - keep_lead, D_k)"""
    return max(int(f) - int(keep_lead), int(delivered_before))


def starts(x, counts, pieces, onsets, L=0, ref_peak=None):
    """(f [B], a [B]) over rendered pieces [(first, n)] that tile [0, S): None / INT_MAX for a trimmed row without an onset,
    (None, 0) for a row that is not trimmed"""
    S = np.asarray(x).shape[1]
    fs, out = [], []
    for b, o in enumerate(onsets):
        if o is None or o.mode == 0:
            fs.append(None)
            out.append(0)
            continue
        f = first_active(x[b], counts[b], threshold(o, None if ref_peak is None else ref_peak[b]))
        fs.append(f)
        if f is None:
            out.append(INT_MAX)
            continue
        first, n = next((p, m) for p, m in pieces if p <= f < p + m)
        D, _ = ssref.emit_range(first, n, first + n >= S, S, L)
        out.append(onset_start(f, o.keep_lead, D))
    return fs, out


def rows_ref(x, counts, a, encoding, ref_peak=None, volume=None, shapes=None, limits=None):
    """[bytes of every row's kept range [a_b, n_b)]: stream_shape_ref.rows_ref with the kept range's start - the multiplier
    counts its fades from a_b and reads its breakpoints at row positions (shape_ref.multiplier(a, c, .))"""
    out = []
    for b in range(len(counts)):
        n = int(counts[b])
        ab = min(int(a[b]), n)
        v = np.asarray(x[b], F)[ab:n]
        if ref_peak is not None:
            v = np.zeros_like(v) if F(ref_peak[b]) < F(1e-8) else (v / F(ref_peak[b])).astype(F)
        if volume is not None and F(volume[b]) != F(1.0):
            v = (v * F(volume[b])).astype(F)
        shape = sref.NONE if shapes is None or shapes[b] is None else shapes[b]
        u = (v * sref.multiplier(ab, n - ab, shape)).astype(F)
        v = lref.apply(u, None if limits is None else limits[b])
        out.append(dref.encode(np.minimum(np.maximum(v, F(-1.0)), F(1.0)).astype(F), encoding))
    return out


def equivalent_trims(fs, a, counts):
    """the trim under which the limited delivery keeps [a_b, n_b): {mode 1, thr, keep_lead = f_b - a_b, keep_tail >= n_b}"""
    def one(b, thr):
        return tref.Trim(1, float(thr), int(fs[b]) - int(a[b]), int(counts[b]), 0)
    return one


def skips(a, counts, ranges):
    """skip [piece][B] of the delivered ranges [(e_first, e_n)]: clamp(a_b - e_first, 0, valid[b])"""
    out = []
    for ef, en in ranges:
        valid = np.clip(np.asarray(counts, np.int64) - ef, 0, en)
        out.append(np.clip(np.asarray(a, np.int64) - ef, 0, valid).astype(np.int32))
    return out


def check_onsets(onsets, ref_peak):
    """ValueError naming the row for what the definition refuses of raw onsets (mode, threshold, keep_lead, reserved)"""
    for b, (mode, thr, lead, reserved) in enumerate(onsets):
        if mode not in (0, 1, 2):
            raise ValueError(f"row {b}: onset mode {mode}")
        if not np.isfinite(thr) or thr < 0:
            raise ValueError(f"row {b}: onset threshold")
        if lead < 0:
            raise ValueError(f"row {b}: onset keep_lead {lead}")
        if reserved != 0:
            raise ValueError(f"row {b}: onset reserved {reserved}")
        if mode == 2 and ref_peak is None:
            raise ValueError(f"row {b}: onset mode 2 needs ref_peak")


# ---- the by-value batch of the device test, at test_gpu_stream_shape.py's scale
B, S, THR = 5, 5000, 0.125
COUNTS = np.array([5000, 4097, 1, 0, 2500], np.int64)


def batch():
    """limit_ref.batch's signal at 5000 samples a row, with a quiet lead: row 0 below THR up to f = 1300 and sample 1299
    exactly THR (strictness); row 1 active at sample 0; row 2's one sample inactive; row 3 empty; row 4 with f = 2048, the
    limited kernel's tile edge.  Behind every row's end: 1.0 up to the pitch - active, and never to be found."""
    x = lref.batch()[:, :S].copy()
    rng = np.random.default_rng(77)
    for b, f in ((0, 1300), (4, 2048)):
        x[b, :f] = (rng.uniform(-1, 1, f) * THR * 0.9).astype(np.float32)
        x[b, f] = np.float32(0.5)
    x[0, 1299] = np.float32(THR)
    x[1, 0] = np.float32(-0.5)
    x[2, 0] = np.float32(THR)
    for b in range(B):
        x[b, int(COUNTS[b]):] = 1.0
    return x


__all__ = ["B", "S", "THR", "COUNTS", "batch", "Onset", "INT_MAX", "SILENCE", "WIDTH", "threshold", "first_active", "onset_start", "starts", "rows_ref", "equivalent_trims",
           "skips", "check_onsets"]
