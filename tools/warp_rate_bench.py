#!/usr/bin/env python3
"""What pitch at an output rate costs a whole run (vitsmi.h, "pitch at an output rate"), on bench.py's voice:
    python tools/warp_rate_bench.py [--preset high] [--batch 32] [--tokens 256] [--output-rate HZ] [--kind plain|warp2|glide04|half2]
                                    [--warmup 2] [--runs 6]
One handle, fixed seeds, MiSession.synthesize_batch without the copy of the waveform to the host's caller mattering: the
figure of interest is the kernels' own time, from a run of this tool under `rocprofv3 --kernel-trace --stats`:
  no rate,  warp2     warp_kernel's launch
  a rate,   plain     resample_counts_kernel + resample_kernel
  a rate,   warp2     warp_rate_kernel's one launch in place of both
  a rate,   glide04   glide_rate_kernel's
  a rate,   half2     every other row unpitched: identity rows in warp_rate_kernel's launch, rendered by the resampler's rule
Prints one JSON line with the wall time per run and the launches of the last run."""
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
    ap.add_argument("--output-rate", type=int, default=None)
    ap.add_argument("--kind", choices=["plain", "warp2", "glide04", "half2"], default="warp2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession
    from phoonnx_amd.synth import write_voice
    B, T = a.batch, a.tokens
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{a.preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", a.preset, seed=1234)
        os.replace(path + ".tmp", path)
    s = MiSession(path, pitch_at_rate=True)
    if a.output_rate:
        s.set_output_rate(a.output_rate)
    rng = np.random.default_rng(2024)
    ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sid = np.zeros(B, np.int64) if s.hparam("gin") else None
    rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
    seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    kw = {
        "plain": dict(token_rate=np.ones((B, T), np.float32)),
        "warp2": dict(token_semitones=np.full((B, T), 2.0, np.float32), compensate=True),
        "glide04": dict(token_semitones=np.zeros((B, T), np.float32), token_semitones_end=np.full((B, T), 4.0, np.float32), compensate=True),
        "half2": dict(token_semitones=np.where(np.arange(B)[:, None] % 2 == 0, 2.0, 0.0).astype(np.float32) * np.ones((1, T), np.float32),
                      compensate=True),
    }[a.kind]
    times, r = [], None
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        r = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds, **kw)
        if i >= a.warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    out = {"tool": "warp_rate_bench", "preset": a.preset, "batch": B, "tokens": T, "output_rate": a.output_rate, "kind": a.kind,
           "ms_per_run": float(np.mean(times)), "launches": int(s.stats()["total_launches"]),
           "longest_row": int(np.max(r["sample_lengths"])), "rows_samples": int(np.sum(r["sample_lengths"]))}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
