#!/usr/bin/env python3
"""What pitch costs a stream (vitsmi.h, "streamed pitch"), on bench.py's voice:
    python tools/warp_stream_bench.py [--preset high] [--batch 32] [--tokens 256] [--chunk-frames 64] [--warmup 2]
                                      [--repeats 3] [--runs 6] [--only plain|warp2|glide04] [--output-rate HZ]
One handle, fixed seeds, fp32 chunks through MiSession.synthesize_stream; the consumer only takes the time of every chunk.
The kinds alternate inside every repeat (the machine is shared: a drift hits all of them alike):
  plain     the unwarped stream (vits_run_chunked_ctl)
  warp2     every token at +2 semitones, compensated (vits_run_chunked_glided: windowed warp_kernel launches)
  glide04   every token gliding 0 -> +4, compensated (windowed glide_kernel launches)
Per kind and repeat: the mean ms from the call to the first delivered chunk, and the mean ms per run.  --only times one kind
alone: the windowed launches' own times come from a kernel trace of such a run
(rocprofv3 --kernel-trace --stats -- python tools/warp_stream_bench.py --only warp2).
--output-rate sets the session's output rate: plain is then the resampled stream, warp2 / glide04 the folded ones (vitsmi.h,
"pitch at an output rate": windowed warp_rate_kernel / glide_rate_kernel launches, no resampler stage).
Prints one JSON line."""
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
    ap.add_argument("--chunk-frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--only", choices=["plain", "warp2", "glide04"], default=None)
    ap.add_argument("--output-rate", type=int, default=None)
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
    ones = np.ones((B, T), np.float32)
    kinds = {
        "plain": dict(token_rate=ones),
        "warp2": dict(token_semitones=np.full((B, T), 2.0, np.float32), compensate=True),
        "glide04": dict(token_semitones=np.zeros((B, T), np.float32), token_semitones_end=np.full((B, T), 4.0, np.float32), compensate=True),
    }
    if a.only:
        kinds = {a.only: kinds[a.only]}

    def run(kw):
        t0 = time.perf_counter()
        first = None
        n_chunks = samples = 0
        for _, data, total in s.synthesize_stream(ids, lens, rows, sid, chunk_frames=a.chunk_frames, seeds=seeds, **kw):
            if first is None:
                first = time.perf_counter() - t0
            n_chunks += 1
            samples = total
        return first * 1e3, (time.perf_counter() - t0) * 1e3, n_chunks, int(samples)

    out = {"tool": "warp_stream_bench", "preset": a.preset, "batch": B, "tokens": T, "chunk_frames": a.chunk_frames,
           "output_rate": a.output_rate, "runs_per_repeat": a.runs, "first_chunk_ms": {k: [] for k in kinds}, "ms_per_run": {k: [] for k in kinds},
           "chunks": {}, "total_samples": {}, "launches": {}}
    for k, kw in kinds.items():
        for _ in range(a.warmup):
            run(kw)
    for _ in range(a.repeats):
        acc = {k: [] for k in kinds}
        for _ in range(a.runs):
            for k, kw in kinds.items():
                acc[k].append(run(kw))
                out["launches"][k] = int(s.stats()["total_launches"])
        for k in kinds:
            out["first_chunk_ms"][k].append(float(np.mean([r[0] for r in acc[k]])))
            out["ms_per_run"][k].append(float(np.mean([r[1] for r in acc[k]])))
            out["chunks"][k], out["total_samples"][k] = acc[k][-1][2], acc[k][-1][3]
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
