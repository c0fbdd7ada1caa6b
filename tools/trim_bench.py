#!/usr/bin/env python3
"""What trimming costs a delivery (vitsmi.h, "trimmed delivery"), on bench.py's voice:
    python tools/trim_bench.py [--preset high] [--batch 32] [--tokens 256] [--warmup 5] [--iters 30] [--untrimmed-only]
One handle, one run (fixed seeds), workspaces reserved; then the SAME run is delivered over and over, one stream per row,
natively as PCM16 and at 8000 Hz as mu-law.  Every call ends in a device synchronise of its own, so the wall clock around
it is the call.  The variants alternate inside every iteration (the machine is shared: a drift hits all of them alike):
  plain_ms        deliver(normalize 0): pack and copy alone
  norm_ms         deliver(normalize 1): + delivery_peak_kernel, one read of the valid samples - so norm_ms - plain_ms is one
                  pass over the waveform at the peak kernel's own rate (peak_pass_ms)
  trim_abs_ms     deliver(normalize 1, trims=absolute): + the scan, the readback of the bounds, the plan
  trim_rel_ms     deliver(normalize 1, trims=relative): + the peak launch over the untrimmed rows in front of the scan
  layout_ms       deliver_layout(trims=relative): the scan and its readback without pack and copies
The thresholds are tiny and the margins huge, so that nothing is cut (the synthetic voice renders no silence): the trimmed
calls move the same bytes as the untrimmed ones, and the difference is what the scan adds.  --untrimmed-only times
plain_ms and norm_ms alone: it runs on a tree without the feature too, for the comparison with the parent commit.
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
    ap.add_argument("--untrimmed-only", action="store_true")
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
    out = {"tool": "trim_bench", "preset": a.preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters, "rates": {}}
    for rate, enc in ((None, "pcm16"), (8000, "ulaw")):
        s.set_output_rate(rate)
        s._begin(ids, lens, rows, sid, noise, seeds)
        frames = int(s.last_y_lengths().max())
        s.sync()
        s.reserve(B, T, frames + 64)       # (no timed call reallocates)
        s._begin(ids, lens, rows, sid, noise, seeds)
        s.sync()
        counts = s.last_sample_counts()
        plain = [ses.Segment(b, b, 0, 0, 1.0) for b in range(B)]
        norm = [ses.Segment(b, b, 0, 1, 1.0) for b in range(B)]
        variants = {"plain_ms": lambda: s.deliver(plain, B, enc), "norm_ms": lambda: s.deliver(norm, B, enc)}
        if not a.untrimmed_only:
            t_abs, t_rel = ses.Trim(1, 1e-30, 2 ** 30, 2 ** 30), ses.Trim(2, 1e-30, 2 ** 30, 2 ** 30)
            variants["trim_abs_ms"] = lambda: s.deliver(norm, B, enc, trims=t_abs)
            variants["trim_rel_ms"] = lambda: s.deliver(norm, B, enc, trims=t_rel)
            variants["layout_ms"] = lambda: s.deliver_layout(norm, B, enc, trims=t_rel)
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        ts = {k: [] for k in variants}
        for _ in range(a.iters):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        rec = {"samples": int(counts.sum()), "samples_max": int(counts.max()), "encoding": enc}
        for k, v in ts.items():
            rec[k] = round(float(np.median(v)), 4)
            rec[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        rec["peak_pass_ms"] = round(rec["norm_ms"] - rec["plain_ms"], 4)
        if not a.untrimmed_only:
            base = s.deliver(norm, B, enc)
            got, first, kept = s.deliver(norm, B, enc, trims=t_rel, return_kept=True)
            rec["same_bytes"] = bool(all(np.array_equal(x, y) for x, y in zip(base, got)) and not first.any()
                                     and np.array_equal(kept, counts))
        out["rates"]["native" if rate is None else str(rate)] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
