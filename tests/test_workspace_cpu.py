"""A workspace is sized by the walk that carves it (csrc/slab.hpp, csrc/workspace.hpp): the byte count of a device slab is
`used` after a dry run of the same function, with the same arguments, that later hands out the buffers.  No GPU:
workspace_driver.cpp is model.cpp + onnx_reader.cpp + those headers under the host compiler.  Per row the driver checks that
the real walk ends where the dry one did, that every buffer is 256-byte aligned and none overlaps another at the extent its
kernels need (plane tensors with their pad), and that a carver one byte short reports it; here: no row left out, and sizes
that never shrink when a request grows - which is what lets a reservation for the largest request cover every smaller one."""
import glob
import os
import shutil
import subprocess
from collections import Counter

from conftest import ROOT

CSRC = os.path.join(ROOT, "phoonnx_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
VOICES = ("sx_rb1", "sx_rb2_ms", "tiny_dp", "tiny_rb1", "tiny_rb2_ms")
PRECISIONS = ("f16x3", "bf16x6", "f16")
BS, TS, FS, CHUNKS = (1, 2, 8, 32, 256), (1, 4, 37, 256, 1024), (1, 4, 63, 1000, 8000), (0, 16, 64)  # chunk 0: unchunked
PLANS = ("tokens", "frames", "vocoder", "inputs", "pcm16")


def _driver(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "workspace_driver")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-I" + CSRC, os.path.join(ROOT, "tests", "workspace_driver.cpp"),
                        os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "onnx_reader.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_every_workspace_is_the_size_its_walk_carves(tmp_path):
    files = [os.path.join(GOLDEN, v + ".onnx") for v in VOICES] + sorted(glob.glob(os.path.join(GOLDEN, "variants", "*.onnx")))
    assert len(files) >= len(VOICES) + 5, files
    env = {k: v for k, v in os.environ.items() if not k.startswith("VITSMI_")}
    r = subprocess.run([_driver(tmp_path)] + files, capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = {}
    for ln in r.stdout.splitlines():
        voice, prec, b, t, f, chunk, verdict, *rest = ln.split(" ", 7)
        key = (voice, prec, int(b), int(t), int(f), int(chunk))
        assert key not in rows, key
        rows[key] = (verdict, rest[0] if rest else "")
    # the whole grid, no row left out: every (voice, precision, size) has a verdict or the packer's refusal
    want = {(os.path.basename(v), p, b, t, f, c) for v in files for p in PRECISIONS for b in BS for t in TS for f in FS for c in CHUNKS}
    assert set(rows) == want, (len(rows), len(want), sorted(set(rows) ^ want)[:5])
    bad = {k: v for k, v in rows.items() if v[0] == "V"}
    assert not bad, sorted(bad.items())[:10]
    assert all(v[0] in "AR" for v in rows.values())
    silent = [k for k, v in rows.items() if v[0] == "R" and len(v[1].strip()) < 8]
    assert not silent, silent[:10]
    # every fixture voice is walked at every precision (a refusal is for the variant that is there to be refused)
    for v in VOICES:
        for p in PRECISIONS:
            assert rows[(v + ".onnx", p, 1, 1, 1, 0)][0] == "A", (v, p, rows[(v + ".onnx", p, 1, 1, 1, 0)])
    size = {k: dict(zip(PLANS, map(int, v[1].split()))) for k, v in rows.items() if v[0] == "A"}
    assert all(len(s) == len(PLANS) and min(s.values()) > 0 for s in size.values())
    # non-decreasing in each of B, T and F with the others fixed
    grids = (BS, TS, FS)
    for (voice, prec, b, t, f, c), s in size.items():
        at = (b, t, f)
        for axis, grid in enumerate(grids):
            i = grid.index(at[axis])
            if i + 1 == len(grid):
                continue
            nxt = list(at)
            nxt[axis] = grid[i + 1]
            s2 = size[(voice, prec, *nxt, c)]
            for plan in PLANS:
                assert s2[plan] >= s[plan], (voice, prec, plan, at, tuple(nxt), c, s[plan], s2[plan])
    # ... and a chunked run never needs more than the unchunked one of the same request
    for (voice, prec, b, t, f, c), s in size.items():
        if c:
            whole = size[(voice, prec, b, t, f, 0)]
            assert s["frames"] <= whole["frames"] and s["vocoder"] <= whole["vocoder"], (voice, prec, b, t, f, c)
    n = Counter((k[0], v[0]) for k, v in rows.items())
    print(", ".join(f"{v} {n[(v, 'A')]} walked / {n[(v, 'R')]} refused" for v in sorted({k[0] for k in rows})))
