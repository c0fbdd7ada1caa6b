"""An independent NumPy statement of the encoded-stream definition (include/vitsmi.h, "encoded streaming"): a chunk is B rows
at a 16-byte row pitch, each holding its valid encoded samples and silence behind them, with the running peaks of the rows.
The sample functions are delivery_ref's (the definition says: the delivery's sample with peak := ref_peak[b]); nothing here
imports the package."""
from collections import namedtuple

import numpy as np

from delivery_ref import DTYPE, SILENCE, WIDTH, encode, postprocess

Chunk = namedtuple("Chunk", "first n pitch valid data peak")    # data: [B] bytes objects of `pitch` bytes; peak float32 [B]


def pitch_of(n, encoding):
    return -(-WIDTH[encoding] * int(n) // 16) * 16


def check_format(encoding, ref_peak, volume, B):
    """ValueError for what the definition refuses"""
    if encoding not in WIDTH:
        raise ValueError("unknown encoding")
    for b in range(B):
        if volume is not None and not np.isfinite(volume[b]):
            raise ValueError(f"volume[{b}]")
        if ref_peak is not None and not (np.isfinite(ref_peak[b]) and ref_peak[b] >= 0):
            raise ValueError(f"ref_peak[{b}]")


def chunk_ref(x, counts, first, n, encoding, ref_peak=None, volume=None):
    """x [B, S] float32 (what lies behind counts[b] is never read), columns [first, first + n) -> Chunk"""
    x = np.asarray(x, np.float32)
    B = x.shape[0]
    check_format(encoding, ref_peak, volume, B)
    w, pitch = WIDTH[encoding], pitch_of(n, encoding)
    valid, rows, peak = np.zeros(B, np.int32), [], np.zeros(B, np.float32)
    for b in range(B):
        valid[b] = min(max(int(counts[b]) - first, 0), n)
        v = postprocess(x[b, first:first + int(valid[b])], None if ref_peak is None else np.float32(ref_peak[b]),
                        np.float32(1.0) if volume is None else np.float32(volume[b]))
        row = encode(v, encoding)
        rows.append(row + SILENCE[encoding] * ((pitch - len(row)) // w))
        assert len(rows[-1]) == pitch
        seen = x[b, :first + int(valid[b])]          # (first + valid[b] <= counts[b] wherever valid[b] > 0; else the row has ended)
        seen = seen[:int(counts[b])]
        peak[b] = np.max(np.abs(seen)) if seen.size else np.float32(0)
    return Chunk(first, n, pitch, valid, rows, peak)


def stream_ref(x, counts, ranges, encoding, ref_peak=None, volume=None):
    """the chunks of the (first, n) pairs in `ranges`"""
    return [chunk_ref(x, counts, f, n, encoding, ref_peak, volume) for f, n in ranges]


def pieces(S, piece):
    """columns [0, S) cut into pieces of `piece` samples, the last one shorter"""
    return [(f, min(piece, S - f)) for f in range(0, S, piece)]


def joined(chunks, b, encoding):
    """row b's valid bytes, joined over the chunks"""
    w = WIDTH[encoding]
    return b"".join(c.data[b][:w * int(c.valid[b])] for c in chunks)


__all__ = ["Chunk", "DTYPE", "SILENCE", "WIDTH", "chunk_ref", "stream_ref", "pieces", "joined", "pitch_of", "check_format"]
