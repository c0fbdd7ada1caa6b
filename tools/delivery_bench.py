#!/usr/bin/env python3
"""What delivering a batch costs (vitsmi.h, "delivery") against what it replaces, on bench.py's voice:
    python tools/delivery_bench.py [--preset medium] [--batch 32] [--tokens 256] [--warmup 5] [--iters 20]
One handle, host inputs, fixed seeds (every pass renders the same frames), workspaces reserved.  Two requests: every row
`tokens` ids long ("equal"), and rows of tokens/8 .. tokens ids ("mixed").  Per request, wall-clock per call (median):
  host_ms            synthesize_batch (the fp32 [B,1,1,S_max] array to the host) + per row the .copy() cut, TTSVoice._postprocess
                     and AudioChunk.audio_int16_array: what synthesize_requests does today;
  delivered_pcm16_ms synthesize_delivered(encoding="pcm16"): run, post-processing, encoding and packing on the device;
  delivered_ulaw8k_ms the same in mu-law with the output rate at 8000 Hz (host_ulaw8k_ms: the host path at that rate, with
                     audio_encoding.encode(..., "ulaw") in the place of the int16 conversion);
  run_ms             the run alone (vits_run_async + vits_sync), for scale;
and the bytes that cross the bus each way.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, _ffi, audio_encoding
    from phoonnx_amd.config import SynthesisConfig
    from phoonnx_amd.synth import write_voice
    from phoonnx_amd.voice import AudioChunk, TTSVoice
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
    sid = np.zeros(B, np.int64) if s.hparam("gin") else None
    rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
    seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    noise = _ffi.VitsNoise()
    syn = SynthesisConfig(normalize_audio=True, volume=1.0)
    requests = {"equal": np.full(B, T, np.int64), "mixed": np.linspace(T // 8, T, B).astype(np.int64)}
    out = {"tool": "delivery_bench", "preset": a.preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters,
           "requests": {}}

    def host(encoding):
        def fn():
            r = s.synthesize_batch(ids, lens, rows, sid, seeds=seeds)
            valid = r["sample_lengths"] if "sample_lengths" in r else r["y_lengths"] * hop
            res = []
            for b in range(B):
                audio = r["output"][b, 0, 0, :int(valid[b])].copy()
                v = TTSVoice._postprocess(None, audio, syn)
                res.append(AudioChunk(0, 2, 1, v).audio_int16_array if encoding == "pcm16" else audio_encoding.encode(v, encoding))
            return r, res
        return fn

    def run_only():
        s._begin(ids, lens, rows, sid, noise, seeds)
        s.sync()

    for name, lens in requests.items():
        rec = {"lens_min": int(lens.min()), "lens_max": int(lens.max())}
        for rate, enc in ((None, "pcm16"), (8000, "ulaw")):
            s.set_output_rate(rate)
            s._begin(ids, lens, rows, sid, noise, seeds)
            frames = int(s.last_y_lengths().max())
            s.sync()
            s.reserve(B, T, frames + 64)   # (no timed pass reallocates)
            tag = "pcm16" if rate is None else "ulaw8k"
            r, res = host(enc)()
            d = s.synthesize_delivered(ids, lens, rows, sid, encoding=enc, seeds=seeds)
            same = all(np.array_equal(x, y) for x, y in zip(res, d["streams"]))
            rec[f"host_{tag}_ms"], rec[f"host_{tag}_min_ms"] = timed(host(enc), a.warmup, a.iters)
            rec[f"delivered_{tag}_ms"], rec[f"delivered_{tag}_min_ms"] = timed(
                lambda: s.synthesize_delivered(ids, lens, rows, sid, encoding=enc, seeds=seeds), a.warmup, a.iters)
            rec[f"run_{tag}_ms"], _ = timed(run_only, a.warmup, a.iters)
            rec[f"host_{tag}_bytes"] = int(r["output"].nbytes)
            rec[f"delivered_{tag}_bytes"] = int(sum(x.nbytes for x in d["streams"]))
            rec[f"same_bytes_{tag}"] = bool(same)
            rec[f"samples_max_{tag}"] = int(r["output"].shape[3])
        out["requests"][name] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
