"""An independent NumPy statement of the trimmed delivery (include/vitsmi.h, "trimmed delivery"): the kept range of a row, the
refusals, the layout with tails - element by element, so that copies and fills can be read off it - and the byte streams.
Nothing here imports the package; the sample formula and the encoders are delivery_ref's.

A trim is anything with the attributes mode, threshold, keep_lead, keep_tail, tail_samples (Trim below)."""
from collections import namedtuple

import numpy as np

import delivery_ref as ref
from delivery_ref import INT_MAX, SILENCE, WIDTH, Seg

Trim = namedtuple("Trim", "mode threshold keep_lead keep_tail tail_samples")
OFF = Trim(0, 0.0, 0, 0, 0)


def kept_range(n, first_active, last_active, t):
    """the rule: (a, c) from the first / last active index (first > last: none active)"""
    n = int(n)
    if t.mode == 0:
        return 0, n
    if first_active > last_active:
        return 0, 0
    a = max(0, int(first_active) - int(t.keep_lead))
    e = min(n, int(last_active) + 1 + int(t.keep_tail))
    return a, e - a


def active_bounds(row, n, t):
    """(first, last) active index of row[:n] under trim t, (INT_MAX, -1) when none is (or the trim is off) - by a plain walk"""
    n = int(n)
    if t.mode == 0 or n == 0:
        return INT_MAX, -1
    v = np.abs(np.asarray(row, np.float32)[:n])
    thr = np.float32(t.threshold)
    if t.mode == 2:
        peak_all = np.float32(0)
        for s in v:
            peak_all = s if s > peak_all else peak_all
        thr = np.float32(thr * peak_all)
    first, last = INT_MAX, -1
    for i, s in enumerate(v.tolist()):
        if np.float32(s) > thr:
            first = min(first, i)
            last = i
    return first, last


def trim_range_ref(row, n, t):
    if int(n) > 4096:        # (long rows: the same rule, vectorised)
        v = np.abs(np.asarray(row, np.float32)[:int(n)])
        if t.mode == 0:
            return 0, int(n)
        thr = np.float32(t.threshold) if t.mode == 1 else np.float32(np.float32(t.threshold) * v.max())
        idx = np.nonzero(v > thr)[0]
        return kept_range(n, *((int(idx[0]), int(idx[-1])) if idx.size else (INT_MAX, -1)), t)
    return kept_range(n, *active_bounds(row, n, t), t)


def trim_bad(t):
    return (t.mode not in (0, 1, 2) or not np.isfinite(t.threshold) or t.threshold < 0 or t.keep_lead < 0 or t.keep_tail < 0
            or not 0 <= t.tail_samples <= INT_MAX)


def check(counts, segments, trims, n_streams, encoding):
    """ValueError("segment g") for the first segment the definition refuses - its own fields, then its trim's; -1: the plan"""
    B = len(counts)
    if encoding not in WIDTH or not 1 <= n_streams <= B or not 0 <= len(segments) <= B:
        raise ValueError("segment -1")
    seen = set()
    for g, s in enumerate(segments):
        bad = (not 0 <= s.row < B or s.row in seen or not 0 <= s.stream < n_streams or not 0 <= s.lead_samples <= INT_MAX
               or s.normalize not in (0, 1, 2) or not np.isfinite(s.volume))
        if bad or (trims is not None and trim_bad(trims[g])):
            raise ValueError(f"segment {g}")
        seen.add(s.row)


def element_map(kept, segments, trims, n_streams):
    """The streams, element by element: (map, stream_samples) - map[e] is -1 for silence, else the index of dst element e in the
    packed audio (the kept samples of the segments in dst order, back to back).  Small plans only."""
    trims = trims if trims is not None else [OFF] * len(segments)
    out, samples, packed = [], [], 0
    for j in range(n_streams):
        n0 = len(out)
        for s, t in zip(segments, trims):
            if s.stream != j:
                continue
            c = int(kept[s.row])
            out += [-1] * int(s.lead_samples) + list(range(packed, packed + c)) + [-1] * int(t.tail_samples)
            packed += c
        samples.append(len(out) - n0)
    return np.array(out, np.int64), samples


def runs(mask):
    """maximal runs of True in a boolean vector: [(start, length)]"""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    edges = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a), int(b - a)) for a, b in zip(edges[::2], edges[1::2])]


def plan_ref(kept, segments, trims, n_streams, encoding):
    """-> (stream_samples [J], stream_offsets [J + 1], total_bytes) over kept counts, with the tails"""
    check(kept, segments, trims, n_streams, encoding)
    trims = trims if trims is not None else [OFF] * len(segments)
    w = WIDTH[encoding]
    samples = [sum(int(s.lead_samples) + int(kept[s.row]) + int(t.tail_samples) for s, t in zip(segments, trims) if s.stream == j)
               for j in range(n_streams)]
    offsets = [0]
    for n in samples:
        offsets.append(offsets[-1] + w * n)
    return np.array(samples, np.int64), np.array(offsets, np.int64), offsets[-1]


def deliver_ref(x, counts, segments, trims, n_streams, encoding):
    """x [B, S] float32 (what lies behind counts[b] is never read) -> ([bytes per stream], kept_first [G], kept_count [G])"""
    check(counts, segments, trims, n_streams, encoding)
    trims = trims if trims is not None else [OFF] * len(segments)
    x = np.asarray(x, np.float32)
    kept = [trim_range_ref(x[s.row], counts[s.row], t) for s, t in zip(segments, trims)]
    rows = {s.row: x[s.row, a:a + c] for s, (a, c) in zip(segments, kept)}
    peak_row = {r: (np.max(np.abs(v)) if v.size else np.float32(0)) for r, v in rows.items()}
    out = []
    for j in range(n_streams):
        mine = [(s, t) for s, t in zip(segments, trims) if s.stream == j]
        scope2 = [peak_row[s.row] for s, _ in mine if s.normalize == 2]
        peak_stream = max(scope2) if scope2 else None
        parts = []
        for s, t in mine:
            peak = None if s.normalize == 0 else (peak_row[s.row] if s.normalize == 1 else peak_stream)
            parts += [SILENCE[encoding] * int(s.lead_samples), ref.encode(ref.postprocess(rows[s.row], peak, s.volume), encoding),
                      SILENCE[encoding] * int(t.tail_samples)]
        out.append(b"".join(parts))
    return out, np.array([a for a, _ in kept], np.int64), np.array([c for _, c in kept], np.int64)


# ---- the trims the definition refuses, on delivery_ref.GOOD over delivery_ref.COUNTS (host and device tests)
GOOD_TRIMS = [Trim(2, 0.5, 1, 1, 2), OFF, Trim(1, 0.01, 0, 0, 0)]
# name -> (trims, the segment the message names, a word of the message)
TRIM_REFUSALS = {
    "mode 3": ([GOOD_TRIMS[0], Trim(3, 0.1, 0, 0, 0), OFF], 1, "mode 3"),
    "mode -1": ([Trim(-1, 0.1, 0, 0, 0), OFF, OFF], 0, "mode -1"),
    "threshold negative": ([OFF, OFF, Trim(1, -0.5, 0, 0, 0)], 2, "threshold -0.5"),
    "threshold nan": ([OFF, Trim(1, float("nan"), 0, 0, 0), OFF], 1, "threshold nan"),
    "threshold inf": ([Trim(2, float("inf"), 0, 0, 0), OFF, OFF], 0, "threshold inf"),
    "keep_lead negative": ([OFF, OFF, Trim(1, 0.1, -2, 0, 0)], 2, "keep_lead -2"),
    "keep_tail negative": ([OFF, Trim(1, 0.1, 0, -7, 0), OFF], 1, "keep_tail -7"),
    "tail negative": ([Trim(0, 0.0, 0, 0, -1), OFF, OFF], 0, "tail_samples -1"),
    "tail above INT_MAX": ([OFF, OFF, Trim(0, 0.0, 0, 0, INT_MAX + 1)], 2, f"tail_samples {INT_MAX + 1}"),
}


def batch():
    """The by-value batch of the device test: 10 rows, one for each way the scan can go wrong.  -> (x, counts, segments, trims,
    n_streams).  Values are multiples of 1/8 where equality with a threshold matters (0.25 * 1.0 and 0.5 are exact)."""
    S = 70003
    x = np.zeros((10, S), np.float32)
    rng = np.random.default_rng(2024)
    counts = np.zeros(10, np.int64)

    def quiet(n):
        return rng.uniform(-0.01, 0.01, n).astype(np.float32)

    # 0: the first active sample at index 0, the last at n - 1; n = 300 (no multiple of 64 or 256); absolute threshold
    counts[0] = 300
    x[0, :300] = quiet(300)
    x[0, 0], x[0, 299] = 0.5, -0.5
    # 1: exactly one active sample, negative, in the middle; margins clipped at neither end
    counts[1] = 1000
    x[1, :1000] = quiet(1000)
    x[1, 417] = -0.75
    # 2: none active: every sample at or below thr
    counts[2] = 129
    x[2, :129] = quiet(129)
    # 3: none active: every sample EQUALS thr (0.25, with both signs)
    counts[3] = 77
    x[3, :77] = np.float32(0.25) * rng.choice([-1.0, 1.0], 77).astype(np.float32)
    # 4: n = 0
    # 5: a large value just behind n must not show; active samples only negative; relative threshold
    counts[5] = 513
    x[5, :513] = quiet(513)
    x[5, 100:400] = -np.abs(rng.uniform(0.3, 0.9, 300)).astype(np.float32)
    x[5, 250] = -1.0
    x[5, 513:520] = 100.0
    # 6: longer than 65 536 samples: the grid-stride loop runs; activity in the first and in the second sweep
    counts[6] = 70001
    x[6, :70001] = quiet(70001)
    x[6, 5000] = 0.6
    x[6, 69000] = -0.7
    # 7: mode 2 with threshold >= 1: an empty range, inside a normalize-2 stream
    counts[7] = 200
    x[7, :200] = rng.uniform(-0.9, 0.9, 200).astype(np.float32)
    # 8: margins clipped at both ends (keep_lead / keep_tail larger than what lies around the activity)
    counts[8] = 90
    x[8, :90] = quiet(90)
    x[8, 3:80] = rng.uniform(0.3, 0.8, 77).astype(np.float32)
    # 9: trim off: the whole row
    counts[9] = 65
    x[9, :65] = rng.uniform(-1.2, 1.2, 65).astype(np.float32)
    for b in range(10):
        if b != 5:
            x[b, int(counts[b]):] = np.nan
    segments = [Seg(0, 0, 0, 1, 1.0), Seg(1, 0, 5, 0, 2.5), Seg(2, 0, 0, 1, 1.0),               # stream 0: normalize 1 / 0
                Seg(5, 1, 3, 2, 0.5), Seg(7, 1, 0, 2, 0.5), Seg(6, 1, 0, 2, 0.5), Seg(3, 1, 2, 2, 0.5),   # stream 1: the stream's peak
                Seg(4, 2, 4, 1, 1.0), Seg(8, 2, 0, 1, 1.0), Seg(9, 2, 0, 0, 1.0)]
    trims = [Trim(1, 0.25, 0, 0, 0), Trim(1, 0.25, 10, 20, 7), Trim(1, 0.25, 5, 5, 3),
             Trim(2, 0.25, 2, 3, 0), Trim(2, 1.0, 4, 4, 6), Trim(2, 0.5, 100, 100, 0), Trim(1, 0.25, 9, 9, 0),
             Trim(1, 0.1, 1, 1, 2), Trim(1, 0.25, 50, 50, 0), Trim(0, 0.9, 7, 7, 4)]
    return x, counts, segments, trims, 3
