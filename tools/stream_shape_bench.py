#!/usr/bin/env python3
"""What shaping and limiting an encoded stream costs (vitsmi.h, "shaped streaming"), on bench.py's voice:
    python tools/stream_shape_bench.py [--preset medium] [--chunk-frames 64] [--warmup 3] [--iters 10] [--root DIR]
                                       [--only COLUMN] [--passes N]
One handle, host inputs, fixed seeds (every pass renders the same frames), workspaces reserved.  Two requests: B = 1 x 256 ids
("b1") and B = 32 with rows of 32 .. 256 ids ("b32_mixed"), natively as PCM16.  Per request, wall-clock medians of (a) the
time until the first chunk is in host memory and (b) the whole stream, for the columns
  plain        synthesize_stream_encoded as it was: stream_pack_kernel;
  fades        ... with fades of 5 and 10 ms on every row: stream_pack_shaped_kernel;
  limit110     ... with a limiter of 110 samples (5 ms) at a ceiling of 0.5: stream_pack_limited_kernel and the carry;
  limit1024    ... with the longest look-ahead;
  trim         ... without fades or limiter, every row trimmed at an absolute threshold of 0.01 with keep_lead 110 (vitsmi.h,
               "trimmed streaming"): stream_onset_kernel until every onset is found, stream_pack_shaped_kernel;
  trim_never   ... at a threshold nothing reaches: the scan runs in front of every chunk - its worst case;
  limit110_trim  limit110 with the trim of `trim`.
--root DIR measures the package of another tree (e.g. a checkout of the parent commit, built) with the same script: columns
that tree does not have are left out.  --only COLUMN --passes N runs N untimed passes of one column and nothing else (the
run a kernel trace is taken of).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("plain", "fades", "limit110", "limit1024", "trim", "trim_never", "limit110_trim")


def timed(fn, warmup, iters):
    """fn() -> (first_ms, total_ms, chunks); medians and minima over `iters` calls"""
    for _ in range(warmup):
        fn()
    r = np.array([fn() for _ in range(iters)])
    return {"first_ms": float(np.median(r[:, 0])), "total_ms": float(np.median(r[:, 1])), "first_min_ms": float(r[:, 0].min()),
            "total_min_ms": float(r[:, 1].min()), "chunks": int(r[0, 2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--chunk-frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--only", choices=COLUMNS)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, session
    from phoonnx_amd.synth import write_voice
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{a.preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", a.preset, seed=1234)
        os.replace(path + ".tmp", path)
    s = MiSession(path)
    shaped = hasattr(session, "stream_emit_range")
    cf, T = a.chunk_frames, 256
    rate = s.delivered_rate
    columns = {"plain": {}}
    if shaped:
        fades = session.Shape(int(rate * 0.005), int(rate * 0.010), "linear")
        columns.update({"fades": {"shapes": fades}, "limit110": {"shapes": fades, "limit": session.Limit(0.5, 110)},
                        "limit1024": {"shapes": fades, "limit": session.Limit(0.5, 1024)}})
    if hasattr(session, "Onset"):
        columns.update({"trim": {"onsets": session.Onset(1, 0.01, 110)}, "trim_never": {"onsets": session.Onset(1, 1e30, 110)},
                        "limit110_trim": {"shapes": fades, "limit": session.Limit(0.5, 110), "onsets": session.Onset(1, 0.01, 110)}})
    rng = np.random.default_rng(2024)
    requests = {"b1": np.full(1, T, np.int64), "b32_mixed": np.linspace(32, T, 32).astype(np.int64)}
    out = {"tool": "stream_shape_bench", "root": root, "preset": a.preset, "chunk_frames": cf, "warmup": a.warmup, "iters": a.iters,
           "shaped_path": shaped, "requests": {}}
    for name, lens in requests.items():
        B = len(lens)
        ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
        sid = np.zeros(B, np.int64) if s.hparam("gin") else None
        rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
        seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        list(s.synthesize_stream_encoded(ids, lens, rows, sid, chunk_frames=cf, seeds=seeds))
        frames = int(s.last_y_lengths().max())
        s.reserve(B, T, frames + 64)   # (no timed pass reallocates)
        rec = {"frames": frames, "samples_max": int(np.asarray(s.last_sample_counts()).max())}

        def stream(kw):
            def fn():
                t0 = time.perf_counter()
                first, n = None, 0
                for _ in s.synthesize_stream_encoded(ids, lens, rows, sid, chunk_frames=cf, encoding="pcm16", volume=2.0, seeds=seeds, **kw):
                    n += 1
                    if first is None:
                        first = time.perf_counter()
                return (first - t0) * 1e3, (time.perf_counter() - t0) * 1e3, n
            return fn

        if a.only:
            if a.only in columns:
                for _ in range(a.passes):
                    stream(columns[a.only])()
                rec[a.only] = {"passes": a.passes}
        else:
            for col, kw in columns.items():
                rec[col] = timed(stream(kw), a.warmup, a.iters)
        out["requests"][name] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
