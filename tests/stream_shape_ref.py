"""An independent NumPy statement of the shaped, limited encoded stream (include/vitsmi.h, "shaped streaming"): whole rows
through limit_ref / shape_ref / delivery_ref - a row is a segment that keeps the whole row, peak := ref_peak[b], no level
gain - and the result cut by the timeline.  Nothing here imports the package.

A shape is anything with shape_ref.Shape's fields or None; a limit anything with ceiling and lookahead, or None (the row is
not limited).  One look-ahead L holds for the call."""
import numpy as np

import delivery_ref as dref
import limit_ref as lref
import shape_ref as sref
from stream_pack_ref import Chunk, pitch_of
from delivery_ref import DTYPE, SILENCE, WIDTH

F = np.float32


def emit_range(first, n, is_last, total, L):
    """what the rendered piece [first, first + n) delivers: (e_first, e_n)"""
    e_first = max(first - L, 0)
    end = min(total if is_last else first + n - L, total)
    return e_first, max(end - e_first, 0)


def timeline(pieces, total, L):
    """the delivered ranges of rendered pieces [(first, n)] that tile [0, total)"""
    return [emit_range(f, n, f + n >= total, total, L) for f, n in pieces]


def unlimited(row, c, ref_peak, volume, shape):
    """u [c] of one row: limit_ref.unlimited's formula with peak := ref_peak (None: no normalisation), kept range [0, c)"""
    v = np.asarray(row, F)[:c]
    if ref_peak is not None:
        v = np.zeros_like(v) if F(ref_peak) < F(1e-8) else (v / F(ref_peak)).astype(F)
    if F(volume) != F(1.0):
        v = (v * F(volume)).astype(F)
    return (v * sref.multiplier(0, c, shape if shape is not None else sref.NONE)).astype(F)


def rows_ref(x, counts, encoding, ref_peak=None, volume=None, shapes=None, limits=None):
    """([bytes of every row's delivery], [its values in front of the encoder])"""
    B = len(counts)
    out, vals = [], []
    for b in range(B):
        u = unlimited(x[b], int(counts[b]), None if ref_peak is None else ref_peak[b], 1.0 if volume is None else volume[b],
                      None if shapes is None else shapes[b])
        v = lref.apply(u, None if limits is None else limits[b])
        v = np.minimum(np.maximum(v, F(-1.0)), F(1.0)).astype(F)
        vals.append(v)
        out.append(dref.encode(v, encoding))
    return out, vals


def stream_ref(x, counts, pieces, encoding, ref_peak=None, volume=None, shapes=None, limits=None, L=0):
    """the chunks of the rendered pieces [(first, n)] (they tile [0, S)): one Chunk per piece that delivers something, and the
    delivered range of every piece"""
    x = np.asarray(x, F)
    B, S = x.shape
    w = WIDTH[encoding]
    rows, _ = rows_ref(x, counts, encoding, ref_peak, volume, shapes, limits)
    chunks, ranges = [], timeline(pieces, S, L)
    for (first, n), (ef, en) in zip(pieces, ranges):
        if en == 0:
            continue
        pitch = pitch_of(en, encoding)
        valid, data, peak = np.zeros(B, np.int32), [], np.zeros(B, F)
        for b in range(B):
            valid[b] = min(max(int(counts[b]) - ef, 0), en)
            row = rows[b][w * ef:w * (ef + int(valid[b]))]
            data.append(row + SILENCE[encoding] * ((pitch - len(row)) // w))
            seen = x[b, :min(first + n, int(counts[b]))]       # the running peak sees what has been RENDERED
            peak[b] = np.max(np.abs(seen)) if seen.size else F(0)
        chunks.append(Chunk(ef, en, pitch, valid, data, peak))
    return chunks, ranges


def recut(chunks_rows, counts, ranges, encoding):
    """rows of bytes cut to the delivered ranges: [[bytes per row] per range that delivers]"""
    w = WIDTH[encoding]
    return [[chunks_rows[b][w * ef:w * min(ef + en, int(counts[b]))] for b in range(len(counts))] for ef, en in ranges if en]


__all__ = ["Chunk", "DTYPE", "SILENCE", "WIDTH", "emit_range", "timeline", "unlimited", "rows_ref", "stream_ref", "recut", "pitch_of"]
