"""Whole runs on more than 256 tokens against the C oracle: a sentence of about 130 phonemes is already longer (phoneme-id
sequences carry a blank between symbols), and from token 256 on the duration scans enter their second pass, the length
regulator searches a longer `cum`, and the encoder, duration-predictor and flow kernels tile more columns than any other
test gives them.  Full-width token domain (the "medium" / "small" voices of phoonnx_amd/synth.py), the cheapest vocoder the
format allows - so the oracle stays fast (0.4 s at B = 2, T = 257 and 2.2 s at B = 3, T = 600 on a 16-thread CPU host; every
case prints its own)."""
import os
import time

import numpy as np
import pytest

from bench import voice_cache
from conftest import GOLDEN, zero_tails
from glue_ref import forced_durations_ref, regulate_ref
from philox_ref import row_noise

pytestmark = pytest.mark.gpu

CHEAP = dict(upsample_rates=(2, 2), upsample_kernel_sizes=(4, 4), upsample_initial_channel=32, resblock_kernel_sizes=(3,),
             resblock_dilation_sizes=((1, 2),))
TAPS = ("x", "m_p", "logs_p", "logw", "w_ceil", "z_p", "z")
STAGE_TOL = 2e-4          # (tests/test_gpu_parity.py's, for the committed fixtures)

# name: (preset or fixture, overrides, T, lens, seed); the seeds were chosen on the CPU so that the oracle's own logw keeps every
# valid token's duration clear of an integer (1e-5 relative)
CASES = {
    "medium_sdp_257": ("medium", {}, 257, [257, 170], 1),
    "medium_sdp_600": ("medium", {}, 600, [600, 257, 256], 1),
    "medium_dp_600": ("medium", {"use_sdp": False}, 600, [600, 400], 1),
    "medium_ms_300": ("medium", {"n_speakers": 4}, 300, [300, 280], 1),
    "small_600": ("small", {}, 600, [600, 300], 1),
    "tiny_rb1_600": ("tiny_rb1", None, 600, [600, 410], 1),
}
SCALES = np.array([0.667, 1.4, 0.8], np.float32)
_REF = {}


def _voice(preset, over):
    if over is None:
        return os.path.join(GOLDEN, preset + ".onnx")
    from phoonnx_amd.synth import write_voice
    over = dict(CHEAP, **over)
    tag = preset + "".join(f"_{k}{v}" for k, v in sorted(over.items()))
    tag = "".join(ch if ch.isalnum() or ch in "_-" else "" for ch in tag)
    cache = voice_cache()
    path = os.path.join(cache, f"synth_{tag}.onnx")
    if not os.path.exists(path):
        os.makedirs(cache, exist_ok=True)
        write_voice(path + ".tmp", preset, seed=1234, **over)
        os.replace(path + ".tmp", path)
    return path


def _clear_of_integers(logw, lens, length_scale):
    pre = np.exp(logw[:, 0, :].astype(np.float64)) * np.float64(np.float32(length_scale))
    valid = np.arange(pre.shape[1])[None, :] < np.asarray(lens)[:, None]
    near = np.rint(pre)
    return bool((np.abs(pre - near)[valid] > 1e-5 * np.maximum(near, 1.0)[valid]).all())


def _inputs(name):
    """(path, ids, lens, sid, noise_dp, noise_z) of a case, built as tests/test_gpu_fullsize.py builds them"""
    preset, over, T, lens, seed = CASES[name]
    path = _voice(preset, over)
    rng = np.random.default_rng(seed)
    lens = np.array(lens, np.int64)
    B = len(lens)
    n_vocab, inter, n_spk = _hparams(path)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, n_vocab, lens[b])
    sid = rng.integers(0, n_spk, B).astype(np.int64) if n_spk > 1 else None
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, inter, T * 8)).astype(np.float32)
    return path, ids, lens, sid, ndp, nz


def _hparams(path):
    from phoonnx_amd import MiSession
    s = MiSession(path, host_only=True)
    r = s.hparam("n_vocab"), s.hparam("inter"), s.hparam("n_speakers") if s.hparam("gin") else 1
    s.close()
    return r


def _reference(name):
    if name not in _REF:
        from vits_oracle import VitsOracle
        path, ids, lens, sid, ndp, nz = _inputs(name)
        o = VitsOracle(path)
        t0 = time.perf_counter()
        ref = o.infer(ids, lens, SCALES, sid, ndp, nz)
        print(f"{name}: VitsOracle.infer took {time.perf_counter() - t0:.2f} s")
        _REF[name] = (path, ids, lens, sid, ndp, nz, ref)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_long_run_matches_oracle(name):
    from phoonnx_amd import MiSession
    path, ids, lens, sid, ndp, nz, ref = _reference(name)
    T = ids.shape[1]
    # on the oracle alone: the frames fit the injected noise, no duration hangs on the last bit of logw, and tokens from 256 on
    # have something to say
    assert int(ref["y_lengths"].max()) <= 8 * T
    assert _clear_of_integers(ref["logw"], lens, SCALES[1])
    assert np.abs(ref["logw"][:, :, 256:]).max() > 0 and ref["w_ceil"][:, 256:].any()
    s = MiSession(path)
    got = s.synthesize_batch(ids, lens, SCALES, sid, ndp, nz, taps=TAPS)
    assert np.array_equal(got["w_ceil"], ref["w_ceil"])          # integer durations: exact
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    tol = STAGE_TOL if name.startswith("tiny") else 5e-4
    for k in ("x", "m_p", "logs_p", "logw", "z_p", "z"):
        np.testing.assert_allclose(got[k], ref[k], atol=tol, rtol=0, err_msg=k)
    assert got["output"].shape == ref["output"].shape
    want = zero_tails(ref["output"], ref["y_lengths"], s.hparam("hop"))
    err = float(np.abs(got["output"] - want).max())
    print(f"{name}: waveform max-abs error vs oracle {err:.3g}, reference peak {np.abs(ref['output']).max():.3g}")
    assert err < 1e-3, err
    assert np.abs(ref["output"]).max() > 0.02                    # the comparison is not vacuous
    s.close()


def test_forced_durations_past_256_tokens():
    """Forced durations over 600 tokens with runs of dropped tokens across index 256 and an utterance without any frame:
    the durations and frame counts come back exactly, and at noise_scale 0 z_p is the NumPy length regulator over the run's
    own m_p / logs_p, bit for bit."""
    from phoonnx_amd import MiSession
    path, ids, lens, sid, _, _ = _inputs("medium_sdp_600")
    B, T = ids.shape
    rng = np.random.default_rng(17)
    dur = rng.integers(0, 4, (B, T)).astype(np.int64)
    dur[0, 250:262] = 0
    dur[0, 590:] = 0
    dur[1, 255:257] = 0
    dur[2, :] = 0
    for b in range(B):
        dur[b, lens[b]:] = 0
    w_ref, _, y_ref = forced_durations_ref(dur, lens)
    s = MiSession(path)
    scales = np.array([0.0, 1.0, 0.8], np.float32)
    got = s.synthesize_batch(ids, lens, scales, sid, taps=("m_p", "logs_p", "w_ceil", "z_p"), durations=dur, return_durations=True)
    assert np.array_equal(got["durations"], dur) and np.array_equal(got["w_ceil"], w_ref)
    assert np.array_equal(got["y_lengths"], y_ref) and y_ref[2] == 1
    F = got["z_p"].shape[2]
    want = regulate_ref(got["m_p"], got["logs_p"], dur, np.zeros((B, got["m_p"].shape[1], F), np.float32), 0.0, y_ref, F=F)
    assert np.array_equal(got["z_p"], want)
    assert np.abs(want[0, :, int(y_ref[0]) - 1]).max() > 0 and np.isfinite(got["output"]).all()
    s.close()


def test_seeded_run_past_256_tokens():
    """The seeded streams at T = 600: the run equals the one with tests/philox_ref.py's row_noise injected (the tolerances of
    tests/test_gpu_utterance_settings.py::test_seeded_stream_is_the_documented_one)"""
    from phoonnx_amd import MiSession
    path, ids, lens, sid, _, _ = _inputs("medium_sdp_600")
    B, T = ids.shape
    rows = np.array([[0.667, 1.0, 0.8], [0.5, 1.2, 0.6], [0.667, 0.9, 0.8]], np.float32)
    seeds = np.array([1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0], np.uint64)
    s = MiSession(path)
    ndp = np.stack([row_noise(int(sd), 1, 2, T) for sd in seeds])
    seeded = s.synthesize_batch(ids, lens, rows, sid, taps=("w_ceil", "z"), seeds=seeds)
    C, F = s.hparam("inter"), int(seeded["y_lengths"].max()) + 8
    nz = np.stack([row_noise(int(sd), 2, C, F) for sd in seeds])
    inj = s.synthesize_batch(ids, lens, rows, sid, ndp, nz, taps=("logw", "w_ceil", "z"))
    # (on the injected run alone: no duration hangs on the last bits of logw, where the two runs may differ)
    for b in range(B):
        assert _clear_of_integers(inj["logw"][b:b + 1], lens[b:b + 1], rows[b, 1]), b
    assert np.array_equal(seeded["w_ceil"], inj["w_ceil"]) and np.array_equal(seeded["y_lengths"], inj["y_lengths"])
    assert seeded["w_ceil"][:, 256:].any()
    assert float(np.abs(seeded["z"] - inj["z"]).max()) < 1e-5
    assert float(np.abs(seeded["output"] - inj["output"]).max()) < 1e-5
    s.close()
