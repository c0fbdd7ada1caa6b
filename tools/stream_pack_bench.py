#!/usr/bin/env python3
"""What an encoded stream costs (vitsmi.h, "encoded streaming") against what it replaces, on bench.py's voice:
    python tools/stream_pack_bench.py [--preset medium] [--chunk-frames 64] [--warmup 5] [--iters 20] [--root DIR]
One handle, host inputs, fixed seeds (every pass renders the same frames), workspaces reserved.  Two requests: B = 1 x 256
ids ("b1") and B = 32 with rows of 32 .. 256 ids ("b32_mixed").  Per request, natively as PCM16 and at 8000 Hz as mu-law,
wall-clock medians of (a) the time until the first chunk is in host memory and (b) the whole stream, for
  stream          synthesize_stream alone (fp32 chunks [B, n]);
  stream_host     synthesize_stream + audio_encoding.encode per chunk on the host (every row of the chunk, padding included);
  stream_encoded  synthesize_stream_encoded: post-processing, encoding and masking per chunk on the device;
and the bytes each path copies to the host.  --root DIR measures the package of another tree (e.g. a checkout of the parent
commit, built) with the same script: paths that tree does not have are left out.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, warmup, iters):
    """fn() -> (first_ms, total_ms); medians and minima over `iters` calls"""
    for _ in range(warmup):
        fn()
    r = np.array([fn() for _ in range(iters)])
    return {"first_ms": float(np.median(r[:, 0])), "total_ms": float(np.median(r[:, 1])), "first_min_ms": float(r[:, 0].min()),
            "total_min_ms": float(r[:, 1].min())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--chunk-frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, audio_encoding
    from phoonnx_amd.synth import write_voice
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{a.preset}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", a.preset, seed=1234)
        os.replace(path + ".tmp", path)
    s = MiSession(path)
    has_enc = hasattr(s, "synthesize_stream_encoded")
    cf, T = a.chunk_frames, 256
    rng = np.random.default_rng(2024)
    requests = {"b1": np.full(1, T, np.int64), "b32_mixed": np.linspace(32, T, 32).astype(np.int64)}
    out = {"tool": "stream_pack_bench", "preset": a.preset, "chunk_frames": cf, "warmup": a.warmup, "iters": a.iters,
           "encoded_path": has_enc, "requests": {}}
    for name, lens in requests.items():
        B = len(lens)
        ids = rng.integers(1, s.hparam("n_vocab"), (B, T)).astype(np.int64)
        sid = np.zeros(B, np.int64) if s.hparam("gin") else None
        rows = np.tile(np.array([0.667, LENGTH_SCALE[a.preset], 0.8], np.float32), (B, 1))
        seeds = (np.arange(B, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        rec = {"lens_min": int(lens.min()), "lens_max": int(lens.max())}
        for rate, enc in ((None, "pcm16"), (8000, "ulaw")):
            tag = "pcm16" if rate is None else "ulaw8k"
            s.set_output_rate(rate)
            chunks = list(s.synthesize_stream(ids, lens, rows, sid, chunk_frames=cf, seeds=seeds))
            frames = int(s.last_y_lengths().max())
            counts = np.asarray(s.last_sample_counts(), np.int64)
            s.reserve(B, T, frames + 64)   # (no timed pass reallocates)

            def stream(encode):
                def fn():
                    t0 = time.perf_counter()
                    first = None
                    for _, x, _ in s.synthesize_stream(ids, lens, rows, sid, chunk_frames=cf, seeds=seeds):
                        if encode:
                            audio_encoding.encode(np.clip(x, -1.0, 1.0), enc)
                        if first is None:
                            first = time.perf_counter()
                    return (first - t0) * 1e3, (time.perf_counter() - t0) * 1e3
                return fn

            def encoded():
                t0 = time.perf_counter()
                first = None
                for _ in s.synthesize_stream_encoded(ids, lens, rows, sid, chunk_frames=cf, encoding=enc, seeds=seeds):
                    if first is None:
                        first = time.perf_counter()
                return (first - t0) * 1e3, (time.perf_counter() - t0) * 1e3

            r = {"chunks": len(chunks), "frames": frames, "samples_max": int(counts.max()),
                 "stream": timed(stream(False), a.warmup, a.iters), "stream_host": timed(stream(True), a.warmup, a.iters),
                 "stream_bytes": int(sum(x.nbytes for _, x, _ in chunks))}
            if has_enc:
                got = list(s.synthesize_stream_encoded(ids, lens, rows, sid, chunk_frames=cf, encoding=enc, seeds=seeds))
                w = got[0].data.dtype.itemsize
                r["stream_encoded"] = timed(encoded, a.warmup, a.iters)
                r["stream_encoded_bytes"] = int(sum(B * (-(-w * c.data.shape[1] // 16) * 16) + 4 * B for c in got))
                # the same audio: each row's valid elements are the host encoder's over the fp32 stream's valid samples
                x = np.concatenate([c for _, c, _ in chunks], axis=1)
                r["same_bytes"] = bool(all(
                    np.array_equal(np.concatenate([c.data[b, :int(c.valid[b])] for c in got]),
                                   audio_encoding.encode(np.clip(x[b, :int(counts[b])], -1.0, 1.0), enc)) for b in range(B)))
            rec[tag] = r
        out["requests"][name] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
