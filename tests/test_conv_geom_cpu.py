"""Packed implies launchable (csrc/conv_geom.hpp): the packer and the launchers of both conv engines read one statement of
the tile tables, the LDS stage arithmetic and the size limits.  No GPU: conv_geom_driver.cpp is model.cpp + onnx_reader.cpp
+ that header under the host compiler."""
import os
import shutil
import subprocess
from collections import Counter

from conftest import ROOT

CSRC = os.path.join(ROOT, "phoonnx_amd", "csrc")
KS, DILS = (1, 2, 3, 5, 7, 11, 13), (1, 2, 3, 5, 9, 12, 16, 27, 32)
CINS, COUTS = (16, 32, 64, 96, 128, 512), (32, 64, 128, 192, 512)
F32 = ("f32_hint0", "f32_hint1", "f32_hint2")
SX = ("sx_bf16x3", "sx_f16x2", "sx_f16x1", "sx_f16x2_force16", "sx_f16x2_no_s16")
T_FORMATS = ("T_f32_hint0",) + tuple("T_" + f for f in SX)
T_CASES = ((16, 8), (8, 4), (4, 2), (3, 1), (7, 3))


def _driver(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "conv_geom_driver")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-pthread", "-I" + CSRC, os.path.join(ROOT, "tests", "conv_geom_driver.cpp"),
                        os.path.join(CSRC, "model.cpp"), os.path.join(CSRC, "onnx_reader.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _rows(exe, stage_cap_small):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VITSMI_")}
    if stage_cap_small is not None:
        env["VITSMI_STAGE_CAP_SMALL"] = stage_cap_small
    r = subprocess.run([exe], capture_output=True, text=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = {}
    for ln in r.stdout.splitlines():
        f, cin, cout, k, x, verdict, *msg = ln.split(" ", 6)
        key = (f, int(cin), int(cout), int(k), int(x))
        assert key not in rows, key
        rows[key] = (verdict, msg[0] if msg else "")
    return rows


def test_every_packed_conv_finds_its_stage_on_every_tile_it_may_run_on(tmp_path):
    exe = _driver(tmp_path)
    for cap in (None, "6144"):
        rows = _rows(exe, cap)
        # the whole grid, no case left out: every (format, shape) has a verdict
        want = {(f, ci, co, k, d) for f in F32 + SX for ci in CINS for co in COUTS for k in KS for d in DILS}
        want |= {(f, ci, co, k, u) for f in T_FORMATS for ci in CINS for co in COUTS for k, u in T_CASES}
        assert set(rows) == want, (len(rows), len(want), sorted(set(rows) ^ want)[:5])
        # accepted by the packer => accepted by the stage function the launcher reads, on the packed tile and on every
        # run-time substitute
        bad = {k: v for k, v in rows.items() if v[0] == "V"}
        assert not bad, (cap, sorted(bad.items())[:10])
        # every refusal says why
        assert all(v[0] in "AR" for v in rows.values())
        silent = [k for k, v in rows.items() if v[0] == "R" and len(v[1].strip()) < 8]
        assert not silent, (cap, silent[:10])
        # the grid crosses the limits of every format: it holds accepted and refused shapes
        n = Counter((k[0], v[0]) for k, v in rows.items())
        for f in F32 + SX:
            assert n[(f, "A")] > 0 and n[(f, "R")] > 0, (cap, f, n[(f, "A")], n[(f, "R")])
        # ... at the shapes the limits were read off: 13 DMA rounds against 10 on the sx engine; a 384-column halo on the f32
        # engine's widest-kernel tiles
        for ci in CINS:
            for co in COUTS:
                for f in SX:
                    assert rows[(f, ci, co, 11, 27)][0] == "R", (cap, f, ci, co)
                    if ci > 64:  # (tensors of <= 64 channels are staged raw: halo <= 128 columns)
                        assert rows[(f, ci, co, 7, 27)][0] == "A", (cap, f, ci, co)
            for f in F32:
                assert rows[(f, ci, 128, 13, 32)][0] == "R", (cap, f, ci)
        print(f"VITSMI_STAGE_CAP_SMALL={cap}: " + ", ".join(f"{f} {n[(f, 'A')]} accepted / {n[(f, 'R')]} refused" for f in F32 + SX + T_FORMATS))
