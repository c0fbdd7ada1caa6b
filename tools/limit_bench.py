#!/usr/bin/env python3
"""What the limiter costs a delivery (vitsmi.h, "limited delivery"), on bench.py's voice:
    python tools/limit_bench.py [--preset high] [--batch 32] [--tokens 256] [--warmup 5] [--iters 30] [--unlimited-only]
                                [--only 110|1024|idle]
One handle, one run (fixed seeds), workspaces reserved; then the SAME run is delivered over and over as PCM16, one stream per
row, normalize 0.  Every call ends in a device synchronise of its own, so the wall clock around it is the call.  The variants
alternate inside every iteration (the machine is shared: a drift hits all of them alike):
  shaped_ms         deliver(shapes=Shape(fade_in, fade_out, "smooth")): delivery_pack_shaped_kernel
  leveled_ms        deliver(levels=Level(1, -16 LUFS)): the loudness launches, delivery_pack_kernel
  limited_110_ms    deliver(levels=..., limits=Limit(ceiling, 110)): the levelled delivery with limit_gain_kernel and
                    delivery_pack_limited_kernel in the place of its pack
  limited_1024_ms   the same with a look-ahead of 1024
  limited_idle_ms   a look-ahead of 110 under a ceiling of 1.0, which nothing reaches: the gain launch stages every piece,
                    finds nothing above the ceiling and writes 1.0f without minima and sums
--unlimited-only times the first two alone: it runs on a tree without the feature too, for the comparison with the parent
commit.  --only 110 / --only 1024 / --only idle times one limited variant alone: the kernels' own times come from a kernel trace of such a
run (rocprofv3 --kernel-trace --stats -- python tools/limit_bench.py --only 110).
The ceiling is half the levelled peak of the loudest row, so the limiter works on every row; `over` is the share of the
levelled samples above it, `bytes` what the two launches move at least: x once by each (the gain launch with its halo of
2 L a tile besides), the gain buffer written and read, the PCM16 written.
Prints one JSON line (medians and minima, in ms)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAIN_TILE = 2048       # csrc/limit.hip.hpp, kLimitTile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="high")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--unlimited-only", action="store_true")
    ap.add_argument("--only", choices=["110", "1024", "idle"], default=None, help="time this limited variant alone")
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
    rate = s.delivered_rate
    fades = ses.Shape(int(0.005 * rate), int(0.02 * rate), "smooth")
    level = ses.Level(1, -16.0, 60.0, 0.0)
    variants = {}
    if a.only is None:
        variants["shaped_ms"] = lambda: s.deliver(plain, B, "pcm16", shapes=fades)
        variants["leveled_ms"] = lambda: s.deliver(plain, B, "pcm16", levels=level)
    out = {"tool": "limit_bench", "preset": a.preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters,
           "samples": int(counts.sum()), "samples_max": int(counts.max()), "encoding": "pcm16"}
    if not a.unlimited_only:
        lev, _, gain = s.deliver(plain, B, "f32", levels=level, return_levels=True)
        ceiling = float(np.float32(min(1.0, 0.5 * max(float(np.abs(v).max()) for v in lev))))
        P = int(counts.sum())
        out["ceiling"] = ceiling
        out["over"] = round(float(sum(int((np.abs(v) > ceiling).sum()) for v in lev)) / max(P, 1), 4)
        for L in (110, 1024):
            if a.only not in (None, str(L)):
                continue
            limit = ses.Limit(ceiling, L)
            variants[f"limited_{L}_ms"] = lambda limit=limit: s.deliver(plain, B, "pcm16", levels=level, limits=limit)
            tiles = sum(-(-int(c) // GAIN_TILE) for c in counts)
            out[f"bytes_{L}"] = {"gain_read_x": 4 * (P + 2 * L * tiles), "gain_write_g": 4 * P, "pack_read_x": 4 * P, "pack_read_g": 4 * P,
                                 "pack_write": 2 * P}
        if a.only in (None, "idle") and max(float(np.abs(v).max()) for v in lev) <= 1.0:
            idle = ses.Limit(1.0, 110)
            variants["limited_idle_ms"] = lambda: s.deliver(plain, B, "pcm16", levels=level, limits=idle)
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
    if not a.unlimited_only:
        base = s.deliver(plain, B, "pcm16", levels=level)
        same = s.deliver(plain, B, "pcm16", levels=level, limits=[None] * B)
        out["same_bytes_when_off"] = bool(all(np.array_equal(x, y) for x, y in zip(base, same)))
        got = s.deliver(plain, B, "pcm16", levels=level, limits=ses.Limit(ceiling, 110))
        top = int(np.float32(ceiling) * np.float32(32767.0))
        out["under_the_ceiling"] = bool(all(np.abs(g.astype(np.int32)).max() <= top for g in got))
        out["clipped_without"] = int(sum(int((np.abs(b.astype(np.int32)) == 32767).sum()) for b in base))
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
