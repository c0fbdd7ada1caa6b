#!/usr/bin/env python3
"""What shaping costs a delivery (vitsmi.h, "shaped delivery"), on bench.py's voice:
    python tools/shape_bench.py [--preset high] [--batch 32] [--tokens 256] [--warmup 5] [--iters 30] [--unshaped-only]
One handle, one run (fixed seeds), workspaces reserved; then the SAME run is delivered over and over as PCM16, one stream per
row, normalize 0.  Every call ends in a device synchronise of its own, so the wall clock around it is the call.  The variants
alternate inside every iteration (the machine is shared: a drift hits all of them alike):
  plain_ms        deliver(): delivery_pack_kernel and the copy
  trivial_ms      deliver(shapes=Shape()): shapes without fades and points - the same launch as plain_ms
  fades_ms        deliver(shapes=Shape(fade_in, fade_out, "smooth")): delivery_pack_shaped_kernel, no breakpoints
  envelope_ms     deliver(shapes=[per row: the token_envelope of gains that alternate from token to token]): two breakpoints
                  per token boundary, some 2 * tokens per row
The shapes are built once, outside the timed calls.  The kernels' own times come from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/shape_bench.py ...): delivery_pack_kernel is the plain and trivial calls,
delivery_pack_shaped_kernel the other two - run with --only fades or --only envelope to tell those apart.
--unshaped-only times plain_ms alone: it runs on a tree without the feature too, for the comparison with the parent commit.
Prints one JSON line (medians and minima, in ms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="high")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--unshaped-only", action="store_true")
    ap.add_argument("--only", choices=["fades", "envelope"], default=None, help="of the shaped variants, time this one alone")
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, _ffi
    from phoonnx_amd import session as ses
    from phoonnx_amd.synth import write_voice
    B, T = a.batch, a.tokens
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{a.preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", a.preset, seed=1234)
        os.replace(path + ".tmp", path)
    s = MiSession(path)
    rng = np.random.default_rng(2024)
    ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sid = np.zeros(B, np.int64) if s.hparam("gin") else None
    rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
    seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    noise = _ffi.VitsNoise()
    s._begin(ids, lens, rows, sid, noise, seeds)
    frames = int(s.last_y_lengths().max())
    s.sync()
    s.reserve(B, T, frames + 64)       # (no timed call reallocates)
    s._begin(ids, lens, rows, sid, noise, seeds)
    s.sync()
    counts = s.last_sample_counts()
    plain = [ses.Segment(b, b, 0, 0, 1.0) for b in range(B)]
    variants = {"plain_ms": lambda: s.deliver(plain, B, "pcm16")}
    out = {"tool": "shape_bench", "preset": a.preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters,
           "samples": int(counts.sum()), "samples_max": int(counts.max()), "encoding": "pcm16"}
    if not a.unshaped_only:
        rate = s.delivered_rate
        fades = ses.Shape(int(0.005 * rate), int(0.02 * rate), "smooth")
        gains = np.where(np.arange(T) % 2 == 0, 1.0, 0.5).astype(np.float32)
        dur, hop = s.last_durations(), s.hparam("hop")
        envelope = [ses.Shape(points=ses.token_envelope(ses.token_bounds(dur[b], T, hop, counts[b]), gains, int(0.01 * rate)))
                    for b in range(B)]
        out["points_per_row"] = round(float(np.mean([len(e.points) for e in envelope])), 1)
        trivial = ses.Shape()
        if a.only is None:
            variants["trivial_ms"] = lambda: s.deliver(plain, B, "pcm16", shapes=trivial)
        if a.only in (None, "fades"):
            variants["fades_ms"] = lambda: s.deliver(plain, B, "pcm16", shapes=fades)
        if a.only in (None, "envelope"):
            variants["envelope_ms"] = lambda: s.deliver(plain, B, "pcm16", shapes=envelope)
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    ts = {k: [] for k in variants}
    for _ in range(a.iters):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in ts.items():
        out[k] = round(float(np.median(v)), 4)
        out[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
    if not a.unshaped_only:
        base = s.deliver(plain, B, "pcm16")
        same = s.deliver(plain, B, "pcm16", shapes=trivial)
        out["same_bytes"] = bool(all(np.array_equal(x, y) for x, y in zip(base, same)))
        got = s.deliver(plain, B, "pcm16", shapes=fades)
        out["faded_ends_are_zero"] = bool(all(g[0] == 0 and g[-1] == 0 for g in got))
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
