#!/usr/bin/env python3
"""Throughput of a batch whose utterances carry their own synthesis settings and noise seeds, against the uniform batch:
    python tools/mixed_settings_bench.py [--presets high,medium] [--batch 32] [--tokens 256] [--warmup 5] [--iters 20]
                                         [--mixed-lengths]
On one handle per voice, device-resident inputs (bench.py's voices), the two runs alternate:
  uniform: bench.py's scales [0.667, LENGTH_SCALE, 0.8] through vits_run_device (the flat noise stream);
  mixed:   vits_run_device_rows with length_scale alternating 0.9x / 1.1x the bench value, noise_scale in {0.5, 0.667},
           noise_w in {0.6, 0.8} and a distinct seed per utterance.
--mixed-lengths: utterance lengths drawn from [tokens / 4, tokens] (a padded batch) instead of all `tokens` long.
Each run is timed to its device synchronisation; prints one JSON line with samples/s of both and their ratio."""
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
    ap.add_argument("--presets", default="high,medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mixed-lengths", action="store_true")
    a = ap.parse_args()
    import torch
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession
    from phoonnx_amd.synth import write_voice
    B, T = a.batch, a.tokens
    out = {"tool": "mixed_settings_bench", "batch": B, "tokens": T, "mixed_lengths": a.mixed_lengths, "warmup": a.warmup,
           "iters": a.iters}
    for preset in a.presets.split(","):
        cache = voice_cache()
        path = os.path.join(cache, f"synth_{preset}.onnx")
        if not os.path.exists(path):
            os.makedirs(cache, exist_ok=True)
            write_voice(path + ".tmp", preset, seed=1234)
            os.replace(path + ".tmp", path)
        s = MiSession(path)
        s.set_seed(1234)
        hop = s.hparam("hop")
        rng = np.random.default_rng(2024)
        ids_h = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
        lens_h = rng.integers(T // 4, T + 1, B).astype(np.int64) if a.mixed_lengths else np.full(B, T, np.int64)
        for b in range(B):
            ids_h[b, lens_h[b]:] = 0
        ids, lens = torch.from_numpy(ids_h).cuda(), torch.from_numpy(lens_h).cuda()
        torch.cuda.synchronize()
        ls = LENGTH_SCALE[preset]
        uniform = np.array([0.667, ls, 0.8], np.float32)
        b = np.arange(B)
        mixed = np.stack([np.where(b % 4 < 2, 0.5, 0.667), ls * np.where(b % 2 == 0, 0.9, 1.1),
                          np.where(b % 3 == 0, 0.6, 0.8)], 1).astype(np.float32)
        seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)

        def run(kind):
            t0 = time.perf_counter()
            if kind == "uniform":
                s.run_device(ids.data_ptr(), lens.data_ptr(), B, T, uniform)
            else:
                s.run_device(ids.data_ptr(), lens.data_ptr(), B, T, mixed, seeds=seeds)
            n = int(s.last_y_lengths().sum()) * hop
            s.sync()
            return time.perf_counter() - t0, n

        # workspaces sized once for both workloads (as a serving process would), so that no timed run reallocates
        frames = 0
        for k in ("uniform", "mixed"):
            run(k)
            frames = max(frames, int(s.last_y_lengths().max()))
        s.reserve(B, T, int(frames * 1.25) + 64)
        for _ in range(a.warmup):
            run("uniform")
            run("mixed")
        acc = {"uniform": [0.0, 0], "mixed": [0.0, 0]}
        for _ in range(a.iters):
            for k in ("uniform", "mixed"):
                dt, n = run(k)
                acc[k][0] += dt
                acc[k][1] += n
        u = acc["uniform"][1] / acc["uniform"][0]
        m = acc["mixed"][1] / acc["mixed"][0]
        out[preset] = {"uniform_samples_per_s": u, "mixed_samples_per_s": m, "ratio": m / u,
                       "uniform_samples_per_run": acc["uniform"][1] / a.iters,
                       "mixed_samples_per_run": acc["mixed"][1] / a.iters}
        s.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
