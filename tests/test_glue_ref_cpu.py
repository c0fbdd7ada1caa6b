"""The references of tests/glue_ref.py against numbers the reference project produced: every case of every committed voice
fixture (tests/golden/*.npz).  No GPU."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, case_get, golden_cases
from glue_ref import durations_ref, regulate_ref
from philox_ref import flat_noise, flat_noise64, row_noise, row_noise64

# (the voice fixtures: the G2P ones hold no durations)
_FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLDEN, "*.npz")) if any(k.endswith("/out_w_ceil") for k in np.load(f).files))
_CASES = [(os.path.basename(f)[:-4], c) for f in _FIXTURES for c in golden_cases(np.load(f))]


def test_every_voice_fixture_is_covered():
    assert {p for p, _ in _CASES} >= {"tiny_rb1", "tiny_rb2_ms", "tiny_dp", "sx_rb1", "sx_rb2_ms"} and len(_CASES) >= 25


@pytest.mark.parametrize("preset,case", _CASES)
def test_references_reproduce_the_fixtures(preset, case):
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    lens, sc, nz = (case_get(g, case, k) for k in ("lens", "scales", "noise_z"))
    logw, w_ceil, ylen = (case_get(g, case, k) for k in ("out_logw", "out_w_ceil", "out_y_lengths"))
    w, cum, yl, _ = durations_ref(logw[:, 0, :], lens, sc[1])
    assert np.array_equal(w, w_ceil)
    assert np.array_equal(yl, ylen)
    z_p = case_get(g, case, "out_z_p")
    F = z_p.shape[2]
    if nz is None:                       # (the noise-free cases: noise_scale 0 in the fixture's scales)
        assert sc[0] == 0
        nz = np.zeros_like(z_p)
    want = regulate_ref(case_get(g, case, "out_m_p"), case_get(g, case, "out_logs_p"), w_ceil.astype(np.int64), nz, sc[0], ylen, F=F)
    err = float(np.abs(want - z_p).max())
    assert err <= 1e-6, err


def test_float64_noise_is_the_float32_noise_to_rounding():
    """the float64 Box-Muller variants follow the float32 restatement the seeded-stream tests inject (same counters, same
    uniforms), and the flat stream with a 32-bit stream id is the row stream of channel 0"""
    for seed in (1, 0xFFFFFFFFFFFFFFFF, 42):
        v32 = row_noise(seed, 2, 3, 1026)
        v64, ra = row_noise64(seed, 2, 3, 1026)
        assert v64.shape == ra.shape == (3, 1026) and float(np.abs(v32 - v64).max()) < 2e-6
        assert np.array_equal(flat_noise(seed, 2, 1026), v32[0])
        f64, fra = flat_noise64(seed, 2, 1026)
        assert np.array_equal(f64, v64[0]) and np.array_equal(fra, ra[0])
    assert not np.array_equal(flat_noise(1, 2, 8), flat_noise(1, 2 | (1 << 32), 8))
