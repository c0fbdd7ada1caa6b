#!/usr/bin/env python3
"""What levelling costs a delivery (vitsmi.h, "levelled delivery"), on bench.py's voice:
    python tools/loudness_bench.py [--preset high] [--batch 32] [--tokens 256] [--warmup 5] [--iters 30] [--unlevelled-only]
One handle, one run (fixed seeds), workspaces reserved; then the SAME run is delivered over and over, one stream per row,
natively as PCM16 and at 8000 Hz as mu-law.  Every call ends in a device synchronise of its own, so the wall clock around
it is the call.  The variants alternate inside every iteration (the machine is shared: a drift hits all of them alike):
  plain_ms        deliver(normalize 0): pack and copy alone
  norm_ms         deliver(normalize 1): + delivery_peak_kernel
  level_ms        deliver(normalize 0, levels=row): + the loudness launches, the peak launch under the scan's grid, the copy of
                  energies and peaks, gates and gains on the host
  level_stream_ms the same with one stream of all rows, levelled as a stream (against plain_stream_ms)
  measure_ms      deliver_leveled with dst = NULL: the measurement alone, nothing packed
--unlevelled-only times plain_ms and norm_ms alone: it runs on a tree without the feature too, for the comparison with the
parent commit.  Prints one JSON line (medians and minima, in ms); under a kernel trace the launches' own times show up as
loudness_state_kernel, loudness_carry_kernel, loudness_energy_kernel and loudness_fold_kernel."""
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
    ap.add_argument("--unlevelled-only", action="store_true")
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
    out = {"tool": "loudness_bench", "preset": a.preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters, "rates": {}}
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
        one = [ses.Segment(b, 0, 0, 0, 1.0) for b in range(B)]
        variants = {"plain_ms": lambda: s.deliver(plain, B, enc), "norm_ms": lambda: s.deliver(norm, B, enc)}
        if not a.unlevelled_only:
            row, stream = ses.Level(1, -19.0, 60.0, 0.0), ses.Level(2, -19.0, 60.0, 0.0)
            n, code = len(plain), _ffi.ENCODINGS[enc][0]
            arr, larr = ses._segments(plain)[0], ses._levels(row, n)
            loud, gain = np.zeros(n, np.float64), np.zeros(n, np.float32)

            def measure():
                rc = s._lib.vits_deliver_leveled(s._h, arr, None, larr, n, B, code, s.delivered_rate, None, 0, None, None, None, None,
                                                 _ffi.ptr(loud), _ffi.ptr(gain))
                assert rc == 0, s._err()

            variants["level_ms"] = lambda: s.deliver(plain, B, enc, levels=row)
            variants["plain_stream_ms"] = lambda: s.deliver(one, 1, enc)
            variants["level_stream_ms"] = lambda: s.deliver(one, 1, enc, levels=stream)
            variants["measure_ms"] = measure
        for _ in range(a.warmup):
            for fn in variants.values():
                fn()
        ts = {k: [] for k in variants}
        for _ in range(a.iters):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        rec = {"samples": int(counts.sum()), "samples_max": int(counts.max()), "encoding": enc, "rate": s.delivered_rate}
        for k, v in ts.items():
            rec[k] = round(float(np.median(v)), 4)
            rec[k.replace("_ms", "_min_ms")] = round(float(np.min(v)), 4)
        if not a.unlevelled_only:
            rec["loudness_min"], rec["loudness_max"] = round(float(loud.min()), 3), round(float(loud.max()), 3)
            twice = [s.deliver(plain, B, "f32", levels=row, return_levels=True) for _ in range(2)]
            rec["repeatable"] = bool(twice[0][2].tobytes() == twice[1][2].tobytes() and
                                     all(np.array_equal(x, y) for x, y in zip(twice[0][0], twice[1][0])))
        out["rates"]["native" if rate is None else str(rate)] = rec
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
