#!/usr/bin/env python3
"""Cost of fitted durations (vitsmi.h, "fitted durations") against a free run of the same batch:
    python tools/fit_bench.py [--preset medium] [--batch 32] [--tokens 256] [--warmup 5] [--iters 20] [--kinds free,rows,one]
On one handle (bench.py's voice), host inputs, per-utterance seeds, the runs alternate:
  free: vits_run_async_rows - the duration kernel's own result;
  rows: vits_run_async_fitted, every row a group of its own, its target the free run's frames of that row;
  one:  vits_run_async_fitted, all rows one group, its target the free run's frames of the batch.
A target equal to the free count reproduces the free durations (checked here), so all kinds render the same frames and the
ratios are time ratios; the search still runs its whole bisection.  Each run is timed from the call to its device
synchronisation (no waveform copy to the host).  Prints one JSON line: samples/s and the median of each kind, the stage marks
of one run of each (dp = duration predictor + durations + fit) and the launches.
Kernel times come from a run of this tool under `rocprofv3 --kernel-trace --stats` with one fitted kind (--kinds free,rows or
free,one): fit_duration_kernel, fit_weight_kernel and duration_kernel are the rows to read."""
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
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kinds", default="free,rows,one")
    a = ap.parse_args()
    from bench import LENGTH_SCALE, voice_cache
    from phoonnx_amd import MiSession, _ffi
    from phoonnx_amd.session import Fit, _fit
    from phoonnx_amd.synth import write_voice
    B, T, preset = a.batch, a.tokens, a.preset
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
    s._begin(ids, lens, rows, sid, noise, seeds)
    durations = s.last_durations()
    frames = int(s.last_y_lengths().max())
    s.sync()
    s.reserve(B, T, frames + 64)   # (no timed run reallocates)
    per_row = durations.sum(axis=1)
    fits = {"free": None, "rows": _fit(Fit(np.arange(B), per_row), B, hop), "one": _fit(Fit.one_group(B, int(per_row.sum())), B, hop)}
    kinds = [k for k in a.kinds.split(",") if k]
    out = {"tool": "fit_bench", "preset": preset, "batch": B, "tokens": T, "warmup": a.warmup, "iters": a.iters, "kinds": kinds,
           "frames_per_run": int(per_row.sum())}

    def run(kind):
        t0 = time.perf_counter()
        s._begin(ids, lens, rows, sid, noise, seeds, fit=fits[kind])
        n = int(s.last_y_lengths().sum()) * hop
        s.sync()
        return time.perf_counter() - t0, n

    for k in kinds:   # the identity, before anything is timed
        run(k)
        assert np.array_equal(s.last_durations(), durations), k
        if fits[k] is not None:
            scale, got, status = s.last_fit()
            assert not status.any() and got.sum() == per_row.sum() and (scale >= 1.0).all(), (k, scale, got, status)
            out[k + "_scale_range"] = [float(scale.min()), float(scale.max())]
    for _ in range(a.warmup):
        for k in kinds:
            run(k)
    acc = {k: [[], 0] for k in kinds}
    for _ in range(a.iters):
        for k in kinds:
            dt, n = run(k)
            acc[k][0].append(dt)
            acc[k][1] += n
    for k in kinds:
        out[k + "_samples_per_s"] = acc[k][1] / sum(acc[k][0])
        out[k + "_ms_median"] = 1e3 * float(np.median(acc[k][0]))
        out[k + "_ms_min_max"] = [1e3 * float(min(acc[k][0])), 1e3 * float(max(acc[k][0]))]
        out[k + "_samples_per_run"] = acc[k][1] / max(a.iters, 1)
        if k != "free" and "free" in kinds:
            out[k + "_over_free"] = out[k + "_samples_per_s"] / out["free_samples_per_s"]
    s.set_timing(2)
    for k in kinds:   # stage marks of three runs each (median): where the difference sits
        marks = []
        for _ in range(3):
            run(k)
            marks.append(s.stats())
        out[k + "_stage_ms"] = {x: round(float(np.median([m[x + "_ms"] for m in marks])), 4) for x in ("enc", "dp", "flow", "dec", "total")}
        out[k + "_launches"] = marks[0]["total_launches"]
    s.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
