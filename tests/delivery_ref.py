"""An independent NumPy statement of the delivery definition (include/vitsmi.h, "delivery"): the plan, the fp32
post-processing, the three integer encoders and the byte streams.  Nothing here imports the package: the encoders take
floor(log2 m) from np.frexp (exact for integers below 2^24), the package's host encoder from comparisons, the kernel from a
leading-zero count.

A segment is anything with the attributes row, stream, lead_samples, normalize, volume (Seg below)."""
from collections import namedtuple

import numpy as np

Seg = namedtuple("Seg", "row stream lead_samples normalize volume")
WIDTH = {"pcm16": 2, "ulaw": 1, "alaw": 1, "f32": 4}
SILENCE = {"pcm16": b"\x00\x00", "ulaw": b"\xff", "alaw": b"\xd5", "f32": b"\x00\x00\x00\x00"}
DTYPE = {"pcm16": "<i2", "ulaw": "u1", "alaw": "u1", "f32": "<f4"}
INT_MAX = 2 ** 31 - 1


def _ilog2(m):
    return np.frexp(m.astype(np.float64))[1].astype(np.int64) - 1


def ulaw(q):
    """int16 values -> mu-law bytes (uint8)"""
    s = np.asarray(q).astype(np.int64) >> 2
    neg = s < 0
    m = np.abs(s) + 33
    seg = np.clip(_ilog2(m) - 5, 0, 8)
    u = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
    return (u ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def alaw(q):
    """int16 values -> A-law bytes (uint8)"""
    s = np.asarray(q).astype(np.int64) >> 3
    neg = s < 0
    m = np.where(neg, -s - 1, s)
    seg = np.clip(_ilog2(np.maximum(m, 1)) - 4, 0, 7)
    a = (seg << 4) | (np.where(seg < 2, m >> 1, m >> seg) & 15)
    return (a ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def postprocess(x, peak, volume):
    """one row's valid samples -> v (float32 in [-1, 1]); peak None: no normalisation"""
    v = np.asarray(x, np.float32)
    if peak is not None:
        v = np.zeros_like(v) if np.float32(peak) < np.float32(1e-8) else (v / np.float32(peak)).astype(np.float32)
    if np.float32(volume) != np.float32(1.0):
        v = (v * np.float32(volume)).astype(np.float32)
    return np.minimum(np.maximum(v, np.float32(-1.0)), np.float32(1.0)).astype(np.float32)


def encode(v, encoding):
    """v float32 in [-1, 1] -> bytes"""
    v = np.asarray(v, np.float32)
    if encoding == "f32":
        return v.astype("<f4").tobytes()
    scaled = (v * np.float32(32767.0)).astype(np.float32)
    q = np.trunc(np.minimum(np.maximum(scaled, np.float32(-32767.0)), np.float32(32767.0))).astype(np.int16)
    if encoding == "pcm16":
        return q.astype("<i2").tobytes()
    return (ulaw(q) if encoding == "ulaw" else alaw(q)).tobytes()


def plan_ref(counts, segments, n_streams, encoding):
    """-> (stream_samples [J], stream_offsets [J + 1], total_bytes); ValueError("segment g: ...") for a plan the definition
    refuses (the index of the first offending segment; -1 for a fault of the plan as a whole)"""
    counts = [int(c) for c in counts]
    B = len(counts)
    if encoding not in WIDTH:
        raise ValueError("segment -1: unknown encoding")
    if not 1 <= n_streams <= B:
        raise ValueError("segment -1: n_streams")
    if not 0 <= len(segments) <= B:
        raise ValueError("segment -1: n_segs")
    seen = set()
    for g, s in enumerate(segments):
        bad = (not 0 <= s.row < B or s.row in seen or not 0 <= s.stream < n_streams or not 0 <= s.lead_samples <= INT_MAX
               or s.normalize not in (0, 1, 2) or not np.isfinite(s.volume))
        if bad:
            raise ValueError(f"segment {g}")
        seen.add(s.row)
    w = WIDTH[encoding]
    samples = [sum(int(s.lead_samples) + counts[s.row] for s in segments if s.stream == j) for j in range(n_streams)]
    offsets = [0]
    for n in samples:
        offsets.append(offsets[-1] + w * n)
    return np.array(samples, np.int64), np.array(offsets, np.int64), offsets[-1]


def deliver_ref(x, counts, segments, n_streams, encoding):
    """x [B, S] float32 (whatever lies behind counts[b] is never read) -> [bytes per stream]"""
    plan_ref(counts, segments, n_streams, encoding)
    x = np.asarray(x, np.float32)
    rows = {s.row: x[s.row, :int(counts[s.row])] for s in segments}
    peak_row = {r: (np.max(np.abs(v)) if v.size else np.float32(0)) for r, v in rows.items()}
    out = []
    for j in range(n_streams):
        mine = [s for s in segments if s.stream == j]
        scope2 = [peak_row[s.row] for s in mine if s.normalize == 2]
        peak_stream = max(scope2) if scope2 else None
        parts = []
        for s in mine:
            peak = None if s.normalize == 0 else (peak_row[s.row] if s.normalize == 1 else peak_stream)
            parts.append(SILENCE[encoding] * int(s.lead_samples))
            parts.append(encode(postprocess(rows[s.row], peak, s.volume), encoding))
        out.append(b"".join(parts))
    return out


# ---- the plans the definition refuses, over rows of COUNTS samples (shared by the host and the device tests)
COUNTS = np.array([5, 0, 7, 3, 11, 2], np.int64)
GOOD = [Seg(0, 0, 0, 1, 1.0), Seg(2, 1, 5, 2, 0.5), Seg(3, 1, 0, 0, 2.0)]
# name -> (segments, n_streams, encoding, the segment the message names or None, a word of the message)
REFUSALS = {
    "row below": (GOOD[:2] + [Seg(-1, 0, 0, 1, 1.0)], 2, "pcm16", 2, "row -1"),
    "row above": ([Seg(6, 0, 0, 1, 1.0)] + GOOD[1:], 2, "pcm16", 0, "row 6"),
    "row twice": (GOOD + [Seg(2, 0, 0, 1, 1.0)], 2, "pcm16", 3, "row 2"),
    "stream below": (GOOD[:1] + [Seg(2, -1, 0, 1, 1.0)], 2, "pcm16", 1, "stream -1"),
    "stream above": (GOOD[:1] + [Seg(2, 2, 0, 1, 1.0)], 2, "pcm16", 1, "stream 2"),
    "no streams": (GOOD[:1], 0, "pcm16", None, "n_streams = 0"),
    "more streams than rows": (GOOD[:1], 7, "pcm16", None, "n_streams = 7"),
    "more segments than rows": ([Seg(b % 6, 0, 0, 1, 1.0) for b in range(7)], 1, "pcm16", None, "n_segs = 7"),
    "negative lead": (GOOD[:2] + [Seg(3, 0, -1, 1, 1.0)], 2, "pcm16", 2, "lead_samples -1"),
    "lead above INT_MAX": ([Seg(3, 0, INT_MAX + 1, 1, 1.0)], 2, "pcm16", 0, f"lead_samples {INT_MAX + 1}"),
    "normalize 3": (GOOD[:1] + [Seg(3, 0, 0, 3, 1.0)], 2, "pcm16", 1, "normalize 3"),
    "normalize -1": (GOOD[:1] + [Seg(3, 0, 0, -1, 1.0)], 2, "pcm16", 1, "normalize -1"),
    "volume nan": (GOOD + [Seg(4, 0, 0, 1, float("nan"))], 2, "pcm16", 3, "volume"),
    "volume inf": ([Seg(4, 0, 0, 1, float("inf"))] + GOOD, 2, "pcm16", 0, "volume"),
}
