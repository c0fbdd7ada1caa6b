#!/usr/bin/env python3
"""Cost of the timing controls (vitsmi.h, vits_controls) against a free run of the same batch:
    python tools/timing_control_bench.py [--presets medium] [--batch 32] [--tokens 256] [--warmup 5] [--iters 20]
On one handle per voice (bench.py's voices), host inputs, per-utterance seeds, the three runs alternate:
  free:   vits_run_async_rows - the duration predictor decides;
  forced: vits_run_async_ctl with the free run's own durations (vits_last_durations) - the duration predictor is not
          launched, everything behind it renders the same frames from the same noise;
  rate:   vits_run_async_ctl with token_rate 1.0 everywhere - the free run with one more product per token.
All three render the same number of samples, so the ratios are time ratios.  Each run is timed from the call to its device
synchronisation (no waveform copy to the host); prints one JSON line with samples/s of each and forced / free, rate / free."""
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
    ap.add_argument("--presets", default="medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, _ffi
    from phoonnx_amd.synth import write_voice
    B, T = a.batch, a.tokens
    out = {"tool": "timing_control_bench", "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters}
    for preset in a.presets.split(","):
        cache = voice_cache()
        path = os.path.join(cache, f"synth_{preset}.onnx")
        if not os.path.exists(path):
            os.makedirs(cache, exist_ok=True)
            write_voice(path + ".tmp", preset, seed=1234)
            os.replace(path + ".tmp", path)
        s = MiSession(path)
        hop = s.hparam("hop")
        rng = np.random.default_rng(2024)
        ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
        lens = np.full(B, T, np.int64)
        sid = np.zeros(B, np.int64) if s.hparam("gin") else None
        rows = np.tile(np.array([0.667, LENGTH_SCALE[preset], 0.8], np.float32), (B, 1))
        seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        noise = _ffi.VitsNoise()
        ones = np.ones((B, T), np.float32)
        s._begin(ids, lens, rows, sid, noise, seeds)
        durations = s.last_durations()
        frames = int(s.last_y_lengths().max())
        s.sync()
        s.reserve(B, T, frames + 64)   # (no timed run reallocates)
        kinds = {"free": {}, "forced": {"durations": durations}, "rate": {"token_rate": ones}}

        def run(kind):
            t0 = time.perf_counter()
            s._begin(ids, lens, rows, sid, noise, seeds, **kinds[kind])
            n = int(s.last_y_lengths().sum()) * hop
            s.sync()
            return time.perf_counter() - t0, n

        for _ in range(a.warmup):
            for k in kinds:
                run(k)
        acc = {k: [[], 0] for k in kinds}
        for _ in range(a.iters):
            for k in kinds:
                dt, n = run(k)
                acc[k][0].append(dt)
                acc[k][1] += n
        res = {}
        for k in kinds:
            res[k + "_samples_per_s"] = acc[k][1] / sum(acc[k][0])
            res[k + "_ms_median"] = 1e3 * float(np.median(acc[k][0]))
            res[k + "_samples_per_run"] = acc[k][1] / a.iters
        res["forced_over_free"] = res["forced_samples_per_s"] / res["free_samples_per_s"]
        res["rate_over_free"] = res["rate_samples_per_s"] / res["free_samples_per_s"]
        s.set_timing(2)
        for k in ("free", "forced"):   # stage marks of one run each: where the difference sits
            run(k)
            st = s.stats()
            res[k + "_stage_ms"] = {x: round(st[x + "_ms"], 4) for x in ("enc", "dp", "flow", "dec", "total")}
            res[k + "_launches"] = st["total_launches"]
        out[preset] = res
        s.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
