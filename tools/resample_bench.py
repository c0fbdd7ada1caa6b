#!/usr/bin/env python3
"""What delivering at an output rate costs (vitsmi.h, "output rate"), on bench.py's voice and request:
    python tools/resample_bench.py [--preset high] [--batch 32] [--tokens 256] [--rates 8000,48000] [--mix 8000,0,16000,48000]
                                   [--iters 5]
One handle, host inputs, fixed seeds (every pass renders the same frames).  Per rate, natively (rate 0), and with a rate per
row (--mix: row b at mix[b % len(mix)], 0 native; "output rate per row"; empty: no such case):
  run_ms        vits_run_async + vits_sync of the request (the resampler's launches included);
  pcm_fetch_ms  vits_last_pcm16 of that run: peak, int16 conversion and the copy of [B, S_out] int16 to the host;
  hbm_floor_us  the resample kernel's bytes alone - B * S floats read, B * S_out floats written - at 6.3 TB/s.
The kernels' own time is read from a `rocprofv3 --kernel-trace --stats` pass over this program (resample_kernel: one launch per
pass of every single rate; resample_rows_kernel: the mixed case's, to be read beside resample_kernel at the mix's highest rate).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12   # achievable on an MI355X (float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="high")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rates", default="8000,48000")
    ap.add_argument("--mix", default="8000,0,16000,48000")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, _ffi
    from phoonnx_amd.synth import write_voice
    B, T = a.batch, a.tokens
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{a.preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", a.preset, seed=1234)
        os.replace(path + ".tmp", path)
    s = MiSession(path)
    hop = s.hparam("hop")
    rng = np.random.default_rng(2024)
    ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sid = np.zeros(B, np.int64) if s.hparam("gin") else None
    rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
    seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    noise = _ffi.VitsNoise()
    out = {"tool": "resample_bench", "preset": a.preset, "batch": B, "tokens": T, "iters": a.iters, "rates": {}}
    mix = [int(r) for r in a.mix.split(",") if r]
    cases = [0] + [int(r) for r in a.rates.split(",") if r] + ([[mix[b % len(mix)] for b in range(B)]] if mix else [])
    for rate in cases:
        if isinstance(rate, list):
            s.set_output_rates(rate)
        else:
            s.set_output_rate(rate or None)
        s._begin(ids, lens, rows, sid, noise, seeds)
        frames = int(s.last_y_lengths().max())
        s.sync()
        s.reserve(B, T, frames + 64)   # (no timed pass reallocates)
        run_ms, pcm_ms = [], []
        for it in range(a.iters + 1):
            t0 = time.perf_counter()
            s._begin(ids, lens, rows, sid, noise, seeds)
            counts = s.last_sample_counts()
            s.sync()
            t1 = time.perf_counter()
            pcm = s.last_pcm16(True, 1.0, shape=(B, int(counts.max())))
            t2 = time.perf_counter()
            if it:   # (the first pass warms up)
                run_ms.append((t1 - t0) * 1e3)
                pcm_ms.append((t2 - t1) * 1e3)
        S_in = int(s.last_y_lengths().max()) * hop
        rec = {"S_in": S_in, "S_out": int(pcm.shape[1]), "run_ms": float(np.median(run_ms)),
               "pcm_fetch_ms": float(np.median(pcm_ms)), "pcm_bytes": int(pcm.nbytes)}
        if isinstance(rate, list):
            rec["mix"] = mix
            rec["hbm_floor_us"] = (B * S_in + int(counts.sum())) * 4 / HBM_BYTES_PER_S * 1e6
            out["rates"]["mixed"] = rec
            continue
        if rate:
            rec["hbm_floor_us"] = (B * S_in + B * pcm.shape[1]) * 4 / HBM_BYTES_PER_S * 1e6
        out["rates"][str(rate or "native")] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
