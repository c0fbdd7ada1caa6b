"""Full-size parity on the GPU box: synthetic "medium" / "high" / multi-speaker voices
(phoonnx_amd/synth.py writes .onnx files with the exporter's structure), HIP path vs the C
oracle on identical inputs and injected noise, plus size-independent properties at the
BASELINE batch size."""
import os

import numpy as np
import pytest

from bench import voice_cache
from conftest import zero_tails

pytestmark = pytest.mark.gpu

CACHE = voice_cache()   # (bench.py's voices: the same files)


_ORACLE_REF = {}


def _voice(preset, **over):
    from phoonnx_amd.synth import write_voice
    tag = preset + "".join(f"_{k}{v}" for k, v in sorted(over.items()))
    tag = "".join(ch if ch.isalnum() or ch in "_-" else "" for ch in tag)
    path = os.path.join(CACHE, f"synth_{tag}.onnx")
    if not os.path.exists(path):
        os.makedirs(CACHE, exist_ok=True)
        write_voice(path + ".tmp", preset, seed=1234, **over)
        os.replace(path + ".tmp", path)
    return path


@pytest.mark.parametrize("preset,over,B,T,precision",
                         [("medium", {}, 3, 96, None), ("high", {}, 2, 64, None),
                          ("medium", {"n_speakers": 4}, 2, 80, None),
                          # 64 -> 128 -> 64 -> 32 channels: raw-format z / conv_pre input and stages
                          ("small", {"upsample_initial_channel": 128, "upsample_rates": (8, 4),
                                     "upsample_kernel_sizes": (16, 8)}, 3, 70, None),
                          # the six-product exact arithmetic (the default is f16x3)
                          ("medium", {}, 3, 96, "bf16x6"), ("high", {}, 2, 64, "bf16x6")])
def test_fullsize_pipeline_matches_oracle(monkeypatch, preset, over, B, T, precision):
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice(preset, **over)
    if precision:
        monkeypatch.setenv("VITSMI_GEN_PRECISION", precision)
    s, o = MiSession(path), VitsOracle(path)
    assert s.hparam("gen_nprod") == (6 if precision == "bf16x6" else 2)
    rng = np.random.default_rng(99)
    lens = np.array([T] + [int(x) for x in rng.integers(T // 3, T, B - 1)], np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sid = rng.integers(0, 4, B).astype(np.int64) if over.get("n_speakers", 1) > 1 else None
    scales = np.array([0.667, 1.4, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, s.hparam("inter"), T * 8)).astype(np.float32)
    # (the two arithmetics of a voice are checked against the SAME oracle rendering: the C oracle's generator takes 25-40 s here)
    key = (path, B, T)
    if key not in _ORACLE_REF:
        _ORACLE_REF[key] = o.infer(ids, lens, scales, sid, ndp, nz)
    ref = _ORACLE_REF[key]
    got = s.synthesize_batch(ids, lens, scales, sid, ndp, nz, taps=("x", "m_p", "logs_p", "logw", "w_ceil", "z_p", "z"))
    assert np.array_equal(got["w_ceil"], ref["w_ceil"])          # integer durations: exact
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    for k in ("x", "m_p", "logs_p", "logw", "z_p", "z"):
        np.testing.assert_allclose(got[k], ref[k], atol=5e-4, rtol=0, err_msg=k)
    assert got["output"].shape == ref["output"].shape
    # default tails mode: every valid sample of the graph's padded rendering, exact zeros behind each utterance's end
    hop = s.hparam("hop")
    want = zero_tails(ref["output"], ref["y_lengths"], hop)
    err = np.abs(got["output"] - want).max()
    print(f"{preset} {precision or 'f16x3'}: waveform max-abs error vs oracle {err:.3g}")
    assert err < 1e-3, err                                        # north_star tolerance
    assert 0.02 < np.abs(ref["output"]).max() < 0.999             # the comparison is not vacuous
    # tails="reference": the whole padded output as the graph (and onnxruntime) computes it, tails included ...
    s.set_tails("reference")
    full = s.synthesize_batch(ids, lens, scales, sid, ndp, nz)
    err_full = np.abs(full["output"] - ref["output"]).max()
    assert err_full < 1e-3, err_full
    # ... and the default mode differs from it in NO valid sample, bit for bit (the samples it skips are never read)
    for b in range(B):
        n = int(ref["y_lengths"][b]) * hop
        assert np.array_equal(full["output"][b, 0, 0, :n], got["output"][b, 0, 0, :n]), b
        assert not got["output"][b, 0, 0, n:].any()
    if int(ref["y_lengths"].min()) < int(ref["y_lengths"].max()):
        assert np.abs(full["output"] - got["output"]).max() > 1e-4   # (the graph's tails are not silence)
    s.close()


def test_generator_engines_agree(monkeypatch):
    """The same voice through the split-operand generator (default f16x3 arithmetic) and (VITSMI_GEN_ENGINE=f32)
    through the f32-MFMA generator: two independent implementations of the same fp32 arithmetic must agree to
    rounding."""
    from phoonnx_amd import MiSession
    path = _voice("medium")
    rng = np.random.default_rng(5)
    B, T = 4, 128
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T, T - 17, T // 2, T - 1], np.int64)
    sc = np.array([0.667, 1.3, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    s1 = MiSession(path)
    assert s1.hparam("gen_sx") == 1
    a = s1.synthesize_batch(ids, lens, sc, None, ndp, nz)
    s1.close()
    monkeypatch.setenv("VITSMI_GEN_ENGINE", "f32")
    s2 = MiSession(path)
    assert s2.hparam("gen_sx") == 0
    b = s2.synthesize_batch(ids, lens, sc, None, ndp, nz)
    s2.close()
    assert np.array_equal(a["y_lengths"], b["y_lengths"])
    assert np.abs(a["output"]).max() > 0.02
    np.testing.assert_allclose(a["output"], b["output"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("preset", ["medium", "high"])
def test_encoder_engines_agree(monkeypatch, preset):
    """The text encoder's convs on the split-operand engine (default: f16x3 products, planar epilogue, operand planes
    written by LayerNorm / attention / the first FFN conv) against VITSMI_ENC_ENGINE=f32 (the f32-MFMA engine): the same
    fp32 arithmetic to rounding - durations equal, every tap in front of the generator within the stage tolerance."""
    from phoonnx_amd import MiSession
    path = _voice(preset)
    rng = np.random.default_rng(11)
    B, T = 5, 200
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T, T - 17, T // 2, 3, T - 1], np.int64)
    sc = np.array([0.667, 1.3, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    taps = ("x", "m_p", "logs_p", "logw", "w_ceil", "z_p", "z")
    s1 = MiSession(path)
    assert s1.hparam("enc_sx") == 1
    a = s1.synthesize_batch(ids, lens, sc, None, ndp, nz, taps=taps)
    s1.close()
    monkeypatch.setenv("VITSMI_ENC_ENGINE", "f32")
    s2 = MiSession(path)
    assert s2.hparam("enc_sx") == 0
    b = s2.synthesize_batch(ids, lens, sc, None, ndp, nz, taps=taps)
    s2.close()
    assert np.array_equal(a["w_ceil"], b["w_ceil"]) and np.array_equal(a["y_lengths"], b["y_lengths"])
    for k in ("x", "m_p", "logs_p", "logw", "z_p", "z"):
        assert np.abs(b[k]).max() > 0.05
        np.testing.assert_allclose(a[k], b[k], atol=2e-5, rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(a["output"], b["output"], atol=5e-5, rtol=0)


@pytest.mark.parametrize("preset,B,T", [("medium", 4, 128), ("high", 2, 96)])
def test_generator_f16_mode_agrees_with_exact_mode(monkeypatch, preset, B, T):
    """The default generator arithmetic (f16x3: operands as two fp16 planes, three MFMA products per fp32 product,
    weights scaled per tensor) against VITSMI_GEN_PRECISION=bf16x6 (six bf16 plane products, every product exact):
    the same waveform to fp32 rounding noise."""
    from phoonnx_amd import MiSession
    path = _voice(preset)
    rng = np.random.default_rng(6)
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T] + [int(v) for v in rng.integers(T // 2, T, B - 1)], np.int64)
    sc = np.array([0.667, 1.3, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    s1 = MiSession(path)
    assert s1.hparam("gen_nprod") == 2
    b = s1.synthesize_batch(ids, lens, sc, None, ndp, nz)
    s1.close()
    monkeypatch.setenv("VITSMI_GEN_PRECISION", "bf16x6")
    s2 = MiSession(path)
    assert s2.hparam("gen_nprod") == 6
    a = s2.synthesize_batch(ids, lens, sc, None, ndp, nz)
    s2.close()
    assert np.array_equal(a["y_lengths"], b["y_lengths"])
    assert np.abs(a["output"]).max() > 0.02
    err = float(np.abs(a["output"] - b["output"]).max())
    print(f"{preset}: f16x3 vs exact max-abs {err:.3g}")
    assert err < 2e-5, err


def _snr_db(ref, got):
    ref, got = ref.astype(np.float64), got.astype(np.float64)
    return 10 * np.log10((ref ** 2).sum() / max(((got - ref) ** 2).sum(), 1e-30))


def test_config4_multispeaker_mixed_lengths_reduced_precision_vocoder():
    """BASELINE config 4: multi-speaker voice, mixed-length padded batch, reduced-precision vocoder (gen_precision "f16":
    one fp16 plane per operand, one MFMA product per fp32 product, fp32 accumulation, generator activations stored as fp16).
    Everything up to z is computed exactly as always.  Declared bar: waveform within 1e-2
    max-abs AND >= 35 dB SNR of the fp32 oracle, per utterance."""
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice("medium", n_speakers=4)
    s, o = MiSession(path, gen_precision="f16"), VitsOracle(path)
    assert s.hparam("gen_nprod") == 1 and s.hparam("gen_sx") == 1
    rng = np.random.default_rng(4)
    B, T = 8, 72
    lens = np.array([T] + [int(v) for v in rng.integers(T // 4, T, B - 1)], np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sid = rng.integers(0, 4, B).astype(np.int64)
    scales = np.array([0.667, 1.2, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    ref = o.infer(ids, lens, scales, sid, ndp, nz)
    got = s.synthesize_batch(ids, lens, scales, sid, ndp, nz, taps=("z",))
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    np.testing.assert_allclose(got["z"], ref["z"], atol=5e-4, rtol=0)      # exact part of the pipeline
    hop = s.hparam("hop")
    errs, snrs = [], []
    for b in range(B):
        n = int(ref["y_lengths"][b]) * hop
        errs.append(float(np.abs(got["output"][b, 0, 0, :n] - ref["output"][b, 0, 0, :n]).max()))
        snrs.append(_snr_db(ref["output"][b, 0, 0, :n], got["output"][b, 0, 0, :n]))
    print(f"config 4 (B=8, 4 speakers, mixed lengths), f16 vocoder vs fp32 oracle: max-abs {max(errs):.3g}, worst SNR {min(snrs):.1f} dB")
    assert max(errs) < 1e-2 and min(snrs) > 35.0, (errs, snrs)
    st = s.stats()
    assert st["f16_saturated"] == 0 and 0 < st["f16_peak_max"] < 65504.0   # range-guarded like f16x3
    s.close()


@pytest.mark.parametrize("preset", ["high", "medium"])
def test_f16_vocoder_against_the_oracle_single_speaker(preset):
    """The same bar on the two bench voices (ResBlock1 with 128-row MFMA-bound stages / ResBlock2), B = 3."""
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice(preset)
    s, o = MiSession(path, gen_precision="f16"), VitsOracle(path)
    assert s.hparam("gen_nprod") == 1
    rng = np.random.default_rng(8)
    B, T = 3, 80
    lens = np.array([T, T - 11, T // 2], np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sc = np.array([0.667, 1.4, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    ref = o.infer(ids, lens, sc, None, ndp, nz)
    got = s.synthesize_batch(ids, lens, sc, None, ndp, nz)
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    hop = s.hparam("hop")
    errs, snrs = [], []
    for b in range(B):
        n = int(ref["y_lengths"][b]) * hop
        errs.append(float(np.abs(got["output"][b, 0, 0, :n] - ref["output"][b, 0, 0, :n]).max()))
        snrs.append(_snr_db(ref["output"][b, 0, 0, :n], got["output"][b, 0, 0, :n]))
    print(f"{preset}, f16 vocoder vs fp32 oracle: max-abs {max(errs):.3g}, worst SNR {min(snrs):.1f} dB")
    assert max(errs) < 1e-2 and min(snrs) > 35.0, (errs, snrs)
    s.close()


@pytest.mark.parametrize("preset", ["high", "medium"])
def test_baseline_config3_exact_shape_against_the_oracle(preset):
    """BASELINE config 3 exactly - B = 32 x 256 phoneme ids, full pipeline, the bench's scales, injected noise - rendered as
    ONE batch on the GPU and compared with the C oracle (OpenMP build) on eight utterances of that batch (the whole batch is
    ~50 s of host time per voice; the eight are spread over it and include the longest and the shortest rendering).  An
    utterance's samples do not depend on its batch neighbours except inside the generator's receptive field at its END (a
    shorter batch ends the tensor there, the longer one continues with masked frames: SURVEY section 8c), so the comparison
    stops gen_rf frames short of each utterance's end.  Durations exact, waveform within north_star's 1e-3."""
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice(preset)
    s = MiSession(path)
    try:
        o = VitsOracle(path, native=True)
    except Exception:  # noqa: BLE001 - no -march=native build on this host
        o = VitsOracle(path)
    rng = np.random.default_rng(1234)
    B, T = 32, 256
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sc = np.array([0.667, 1.95, 0.8], np.float32)     # bench.py LENGTH_SCALE: ~3 frames per id
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, s.hparam("inter"), T * 6)).astype(np.float32)
    got = s.synthesize_batch(ids, lens, sc, None, ndp, nz, taps=("w_ceil",))
    hop = s.hparam("hop")
    ylen = got["y_lengths"]
    assert got["output"].shape == (B, 1, 1, hop * int(ylen.max())) and int(ylen.max()) <= T * 6
    order = np.argsort(ylen)
    pick = sorted({int(order[0]), int(order[-1]), 0, 5, 13, 18, 24, 31})
    ref = o.infer(ids[pick], lens[pick], sc, None, ndp[pick], nz[pick])
    assert np.array_equal(ref["y_lengths"], ylen[pick])                     # frame counts: exact
    assert np.array_equal(ref["w_ceil"], got["w_ceil"][pick])               # every token's duration: exact
    rf = 64                                                                 # >= the generator's one-sided receptive field in frames
    worst = 0.0
    for j, b in enumerate(pick):
        n = (int(ylen[b]) - rf) * hop
        assert n > 100 * hop
        worst = max(worst, float(np.abs(got["output"][b, 0, 0, :n] - ref["output"][j, 0, 0, :n]).max()))
    print(f"config 3 ({preset}, B=32 x 256, {int(ylen.sum()) * hop} samples): max-abs vs oracle on {len(pick)} utterances {worst:.3g}")
    assert 0.02 < np.abs(ref["output"]).max() < 0.999
    assert worst < 1e-3, worst
    s.close()


@pytest.mark.parametrize("preset", ["medium", "high"])
def test_durations_do_not_depend_on_the_batch_layout(preset):
    """ceil(w) (models.py:702-704) is a discontinuity in front of everything the listener hears: one flipped duration shifts
    every later sample.  conv_sx() serves the token-domain convs of a SHORT launch with conv_sx_small_kernel (reduction split
    over four waves) and those of a long one with the engine (one accumulator chain): the same utterance's encoder sums
    differ in their last bits between B = 1, B = 8 and B = 32.  256 utterances of 16 .. 256 ids, bench scales, injected
    duration noise, each rendered alone, inside a batch of 8 and inside a batch of 32: every token's duration equal across the
    three layouts, and equal to the C oracle's on a subset.  Would a flip exist, the assertion reports how close w was to an
    integer (the margin a fix would have to respect)."""
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice(preset)
    s = MiSession(path)
    rng = np.random.default_rng(20251004)
    N, T = 256, 256
    lens = rng.integers(16, T + 1, N).astype(np.int64)
    lens[:8] = [T, 16, 255, 17, 128, 64, 200, 33]
    ids = np.zeros((N, T), np.int64)
    for b in range(N):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sc = np.array([0.667, 1.95, 0.8], np.float32)     # bench.py's scales: ~3 frames per id, duration noise ON
    ndp = rng.standard_normal((N, 2, T)).astype(np.float32)

    def render(group):
        w, lw = [], []
        for i in range(0, N, group):
            r = s.synthesize_batch(ids[i:i + group], lens[i:i + group], sc, None, ndp[i:i + group], None, taps=("w_ceil", "logw"))
            w.append(r["w_ceil"].reshape(group, -1))
            lw.append(r["logw"].reshape(group, -1))
        return np.concatenate(w), np.concatenate(lw)

    w1, lw1 = render(1)
    assert w1.shape == (N, T) and float(w1.sum()) > 2.0 * lens.sum()
    margin = None
    for group in (8, 32):
        wg, _ = render(group)
        if not np.array_equal(wg, w1):
            bad = np.argwhere(wg != w1)
            wv = np.exp(lw1.astype(np.float64)) * float(sc[1])
            margin = [float(abs(wv[b, t] - np.rint(wv[b, t]))) for b, t in bad[:16]]
        assert margin is None, (f"{len(bad)} durations differ between B = 1 and B = {group} (of {int(lens.sum())}); "
                                f"|w - nearest integer| at the flips: {margin}")
    # how much room there was: the smallest distance of any w to an integer over the sweep (a flip needs an error of that size)
    wv = np.exp(lw1.astype(np.float64)) * float(sc[1])
    valid = np.arange(T)[None, :] < lens[:, None]
    closest = float(np.abs(wv - np.rint(wv))[valid].min())
    print(f"{preset}: {int(lens.sum())} durations equal across B = 1 / 8 / 32; closest w to an integer: {closest:.3g}")
    # ... and the oracle agrees (a subset: the CPU renders the whole path)
    pick = [1, 3, 5, 7] + [int(i) for i in np.argsort(lens)[:2]]
    o = VitsOracle(path)
    F = int(w1[pick].sum(1).max())
    nz = np.zeros((len(pick), s.hparam("inter"), F), np.float32)
    ref = o.infer(ids[pick], lens[pick], np.array([0.0, sc[1], sc[2]], np.float32), None, ndp[pick], nz)
    assert np.array_equal(ref["w_ceil"].reshape(len(pick), -1), w1[pick])
    s.close()


def test_baseline_batch_properties():
    """B=32 x 256 ids (BASELINE config 3) is too slow for the CPU oracle inside a test, so check
    size-independent properties: batch-composition invariance of durations, shape law
    S = hop * max(y_len), finiteness, |audio| <= 1, and agreement of item 0 with its batch-1 run."""
    from phoonnx_amd import MiSession
    path = _voice("medium")
    s = MiSession(path)
    rng = np.random.default_rng(1234)
    B, T = 32, 256
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sc = np.array([0, 1.5, 0], np.float32)
    r = s.synthesize_batch(ids, lens, sc, taps=("w_ceil",))
    hop = s.hparam("hop")
    assert r["output"].shape == (B, 1, 1, hop * int(r["y_lengths"].max()))
    assert np.isfinite(r["output"]).all() and np.abs(r["output"]).max() <= 1.0
    assert np.array_equal(r["w_ceil"].sum(1).astype(np.int64), r["y_lengths"])
    one = s.synthesize_batch(ids[:1], lens[:1], sc, taps=("w_ceil",))
    assert np.array_equal(one["w_ceil"][0], r["w_ceil"][0])
    n = (int(one["y_lengths"][0]) - 64) * hop  # minus the generator's receptive field at the right edge
    np.testing.assert_allclose(r["output"][0, 0, 0, :n], one["output"][0, 0, 0, :n], atol=2e-5)
    s.close()


# ------------------------------------------------------------------ f16x3 range guard

def _loud_voice(tmp_path, gain):
    """A `small`-family voice on the sx engine whose generator weights are `gain` times the usual ones."""
    from phoonnx_amd.synth import PRESETS, write_voice
    path = str(tmp_path / f"loud_{gain}.onnx")
    write_voice(path, "small", seed=11, upsample_initial_channel=128, upsample_rates=(8, 4), upsample_kernel_sizes=(16, 8),
                dec_gain=PRESETS["small"]["dec_gain"] * gain)
    return path


def test_f16_range_guard_raises_or_falls_back_never_clamps(tmp_path):
    """dec.* weights x100: activations leave the fp16 planes' range.  The engine must not return clamped audio: with the
    fallback off it raises RangeError; with it on (default) the call is repeated with the bf16x6 arithmetic and matches
    the oracle to north_star's 1e-3."""
    from phoonnx_amd import MiSession, RangeError
    from vits_oracle import VitsOracle
    path = _loud_voice(tmp_path, 100.0)
    rng = np.random.default_rng(3)
    B, T = 2, 48
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T, T - 9], np.int64)
    sc = np.array([0.667, 1.2, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 64, T * 8)).astype(np.float32)
    strict = MiSession(path, range_fallback=False)
    assert strict.hparam("gen_sx") == 1 and strict.hparam("gen_nprod") == 2
    with pytest.raises(RangeError, match="65504|range"):
        strict.synthesize_batch(ids, lens, sc, None, ndp, nz)
    st = strict.stats()
    assert st["f16_saturated"] == 1 and not (st["f16_peak_max"] <= 65504.0)
    # the device-resident entry reports it at the synchronisation
    strict.close()
    s = MiSession(path)                                       # range_fallback=True
    got = s.synthesize_batch(ids, lens, sc, None, ndp, nz)
    assert s.hparam("gen_nprod") == 6                         # ... it reopened itself with the exact arithmetic
    ref = VitsOracle(path).infer(ids, lens, sc, None, ndp, nz)
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    assert np.isfinite(ref["output"]).all()
    np.testing.assert_allclose(got["output"], zero_tails(ref["output"], ref["y_lengths"], s.hparam("hop")), atol=1e-3, rtol=0)
    s.close()


def test_f16_range_guard_reports_the_dynamic_range_of_a_normal_voice():
    """On the bench voices nothing comes near either end of the fp16 planes' range: the stats say so."""
    from phoonnx_amd import MiSession
    for preset in ("medium", "high"):
        s = MiSession(_voice(preset))
        rng = np.random.default_rng(2)
        ids = rng.integers(0, 256, (2, 96)).astype(np.int64)
        s.synthesize_batch(ids, np.array([96, 80], np.int64), np.array([0.667, 1.4, 0.8], np.float32))
        st = s.stats()
        print(preset, "f16 planes: launches tracked", st["f16_tracked"], "largest |x|", st["f16_peak_max"],
              "smallest per-tensor peak", st["f16_peak_min"])
        assert st["f16_tracked"] > 20 and st["f16_saturated"] == 0
        assert 2.0 ** -12 < st["f16_peak_min"] <= st["f16_peak_max"] < 65504.0 / 8
        s.close()


def test_nonfinite_input_to_the_generator_is_reported(tmp_path):
    from phoonnx_amd import MiSession, RangeError
    s = MiSession(_voice("medium"), range_fallback=False)
    z = np.random.default_rng(0).standard_normal((1, 192, 40)).astype(np.float32)
    s.vocoder(z)                                              # fine
    z[0, 5, 17] = np.nan
    with pytest.raises(RangeError):
        s.vocoder(z)
    z[0, 5, 17] = np.inf
    with pytest.raises(RangeError):
        s.vocoder(z)
    s.close()


# ------------------------------------------------------------------ chunked / streaming vocoder

@pytest.mark.parametrize("preset,precision", [("medium", "f16x3"), ("high", "f16x3"), ("medium", "f16"), ("high", "f16"),
                                              ("medium", "bf16x6")])
def test_ragged_rendering_equals_the_padded_rendering_on_every_valid_sample(preset, precision):
    """The default tails mode does not render what lies behind an utterance's end (every generator launch ends utterance
    b's tensors gen_rf_frames behind y_len[b]; workgroups behind that exit at once).  Against the graph's padded rendering
    (tails="reference": models.py:348-368 has no mask) on six utterances of 1 .. 120 ids: every valid sample bit for bit -
    in all three arithmetics, i.e. through conv_sx_kernel, the fused pair kernels and the plane-stream generator - zeros
    behind, fewer generator FLOPs accounted, and the chunked renderer agrees with both."""
    from phoonnx_amd import MiSession
    s = MiSession(_voice(preset), gen_precision=precision, tails="reference")
    rng = np.random.default_rng(515)
    B, T = 6, 120
    lens = np.array([T, 97, 64, 33, 12, 1], np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sc = np.array([0.667, 1.8, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 10)).astype(np.float32)
    full = s.synthesize_batch(ids, lens, sc, None, ndp, nz)
    fl_full = s.stats()["dec_flops"]
    s.set_tails("zero")
    rag = s.synthesize_batch(ids, lens, sc, None, ndp, nz)
    fl_rag = s.stats()["dec_flops"]
    hop, rf = s.hparam("hop"), s.hparam("gen_rf_frames")
    ylen = full["y_lengths"]
    assert np.array_equal(ylen, rag["y_lengths"]) and full["output"].shape == rag["output"].shape
    assert int(ylen.min()) + rf < int(ylen.max())                 # (there is something to skip)
    for b in range(B):
        n = int(ylen[b]) * hop
        assert np.array_equal(full["output"][b, 0, 0, :n], rag["output"][b, 0, 0, :n]), (b, n)
        assert not rag["output"][b, 0, 0, n:].any(), b
        if n < full["output"].shape[3]:
            assert np.abs(full["output"][b, 0, 0, n:]).max() > 1e-4     # the graph's own tails are not silence
    # accounted work = the columns inside the (margin-extended) ends: conv_pre's margin is the whole receptive field, every
    # upsampling stage's what is left of it from that stage on
    hi = float(np.minimum(ylen + rf, ylen.max()).sum()) / float(B * ylen.max())
    lo = float(ylen.sum()) / float(B * ylen.max())
    assert lo < fl_rag / fl_full <= hi + 1e-9, (lo, fl_rag / fl_full, hi)
    # chunked rendering in either mode: every sample of the corresponding whole rendering
    for mode, whole in (("zero", rag), ("reference", full)):
        s.set_tails(mode)
        got = np.full(whole["output"].shape[::3], np.nan, np.float32)
        for first, samples, total in s.synthesize_stream(ids, lens, sc, None, chunk_frames=48, noise_dp=ndp, noise_z=nz):
            got[:, first:first + samples.shape[1]] = samples
        assert np.array_equal(got, whole["output"][:, 0, 0, :]), mode
    s.close()


@pytest.mark.parametrize("preset,chunk", [("medium", 32), ("high", 24), ("medium", 1000)])
def test_chunked_rendering_is_bit_identical_to_the_unchunked_run(preset, chunk):
    from phoonnx_amd import MiSession
    s = MiSession(_voice(preset))
    rng = np.random.default_rng(41)
    B, T = 3, 64
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T, 40, 55], np.int64)
    sc = np.array([0.667, 1.3, 0.8], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 192, T * 8)).astype(np.float32)
    whole = s.synthesize_batch(ids, lens, sc, None, ndp, nz)
    S = whole["output"].shape[3]
    got = np.full((B, S), np.nan, np.float32)
    firsts = []
    for first, samples, total in s.synthesize_stream(ids, lens, sc, None, chunk_frames=chunk, noise_dp=ndp, noise_z=nz):
        assert total == S and samples.shape[0] == B
        firsts.append(first)
        got[:, first:first + samples.shape[1]] = samples
    hop = s.hparam("hop")
    assert firsts == sorted(firsts) and firsts[0] == 0
    assert len(firsts) == -(-(S // hop) // chunk)
    assert np.array_equal(s.last_y_lengths(), whole["y_lengths"])
    assert np.array_equal(got, whole["output"][:, 0, 0, :])   # every sample, bit for bit: edges included
    # vocoder-only entry
    z = rng.standard_normal((2, 192, 77)).astype(np.float32)
    ref = s.vocoder(z)[:, 0, 0, :]
    parts = [c for _, c, _ in s.vocoder_stream(z, chunk_frames=chunk)]
    assert np.array_equal(np.concatenate(parts, axis=1), ref)
    s.close()


def test_chunked_rendering_on_the_f32_engine_fixture():
    from conftest import GOLDEN
    from phoonnx_amd import MiSession
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"))
    assert s.hparam("gen_sx") == 0
    rng = np.random.default_rng(4)
    z = rng.standard_normal((2, 32, 150)).astype(np.float32)
    ref = s.vocoder(z)[:, 0, 0, :]
    parts = [c for _, c, _ in s.vocoder_stream(z, chunk_frames=37)]
    assert len(parts) == 5
    assert np.array_equal(np.concatenate(parts, axis=1), ref)
    s.close()


# ------------------------------------------------------------------ corners the first round left open

def test_baseline_batch_properties_high():
    """The headline voice at the headline batch (B=32 x 256 ids), through the size-independent properties."""
    from phoonnx_amd import MiSession
    s = MiSession(_voice("high"))
    rng = np.random.default_rng(1234)
    B, T = 32, 256
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.full(B, T, np.int64)
    sc = np.array([0, 1.5, 0], np.float32)
    r = s.synthesize_batch(ids, lens, sc, taps=("w_ceil",))
    hop = s.hparam("hop")
    assert r["output"].shape == (B, 1, 1, hop * int(r["y_lengths"].max()))
    assert np.isfinite(r["output"]).all() and np.abs(r["output"]).max() <= 1.0
    assert np.array_equal(r["w_ceil"].sum(1).astype(np.int64), r["y_lengths"])
    st = s.stats()
    assert st["f16_saturated"] == 0 and st["sx_launches"] > 60
    one = s.synthesize_batch(ids[:1], lens[:1], sc, taps=("w_ceil",))
    assert np.array_equal(one["w_ceil"][0], r["w_ceil"][0])
    n = (int(one["y_lengths"][0]) - s.hparam("gen_rf_frames")) * hop   # minus the generator's receptive field
    np.testing.assert_allclose(r["output"][0, 0, 0, :n], one["output"][0, 0, 0, :n], atol=2e-5)
    s.close()


@pytest.mark.parametrize("preset,B,F", [("medium", 1, 700), ("high", 2, 300)])
def test_config2_vocoder_only_fullsize_matches_oracle(preset, B, F):
    """BASELINE config 2: the HiFi-GAN vocoder alone, z -> waveform, at the frame count of a 256-id utterance (medium)."""
    from phoonnx_amd import MiSession
    from vits_oracle import VitsOracle
    path = _voice(preset)
    s, o = MiSession(path), VitsOracle(path)
    z = np.random.default_rng(8).standard_normal((B, 192, F)).astype(np.float32)
    got, ref = s.vocoder(z), o.vocoder(z)
    assert got.shape == ref.shape == (B, 1, 1, F * s.hparam("hop"))
    err = float(np.abs(got - ref).max())
    print(f"{preset} vocoder-only B={B} F={F}: max-abs error vs oracle {err:.3g}")
    assert err < 1e-3 and np.abs(ref).max() > 0.02
    s.close()


def test_config4_batch64_properties_f16_vocoder():
    """BASELINE config 4 at its stated size: 4-speaker voice, B=64 mixed lengths with padding mask, reduced-precision
    ("f16") vocoder.  The oracle cannot render 64 utterances inside a test; properties: durations independent of the batch
    composition and of the vocoder arithmetic, shape law, finiteness, every utterance within the mode's declared bar
    (1e-2 max-abs, 35 dB SNR) of the default fp32-grade (f16x3) rendering, and an utterance's interior equal to its own B=1
    rendering."""
    from phoonnx_amd import MiSession
    path = _voice("medium", n_speakers=4)
    rng = np.random.default_rng(64)
    B, T = 64, 96
    lens = np.concatenate([[T], rng.integers(24, T, B - 1)]).astype(np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    sid = rng.integers(0, 4, B).astype(np.int64)
    sc = np.array([0, 1.3, 0], np.float32)
    full = MiSession(path)
    ref = full.synthesize_batch(ids, lens, sc, sid)
    full.close()
    s = MiSession(path, gen_precision="f16")
    assert s.hparam("gen_nprod") == 1
    r = s.synthesize_batch(ids, lens, sc, sid, taps=("w_ceil",))
    hop = s.hparam("hop")
    assert np.array_equal(r["y_lengths"], ref["y_lengths"])
    assert r["output"].shape == (B, 1, 1, hop * int(r["y_lengths"].max())) and np.isfinite(r["output"]).all()
    assert np.all(r["w_ceil"][np.arange(T)[None, :] >= lens[:, None]] == 0)          # padding mask
    worst, snr_min = 0.0, 1e9
    for b in range(B):
        n = int(r["y_lengths"][b]) * hop
        worst = max(worst, float(np.abs(r["output"][b, 0, 0, :n] - ref["output"][b, 0, 0, :n]).max()))
        snr_min = min(snr_min, _snr_db(ref["output"][b, 0, 0, :n], r["output"][b, 0, 0, :n]))
    print(f"config 4, B=64: f16 vocoder vs f16x3: max-abs {worst:.3g}, worst per-utterance SNR {snr_min:.1f} dB")
    assert worst < 1e-2 and snr_min > 35.0
    for b in (0, 17):
        one = s.synthesize_batch(ids[b:b + 1, :lens[b]].copy(), lens[b:b + 1], sc, sid[b:b + 1])
        assert one["y_lengths"][0] == r["y_lengths"][b]
        n = (int(one["y_lengths"][0]) - s.hparam("gen_rf_frames")) * hop
        # (a single utterance runs its token / frame domain on the short-launch kernel, whose fp32 sums are ordered
        # differently from the engine's: z differs in its last bits, and the fp16 activation storage of this vocoder turns
        # that into differences of its own rounding size - far inside the mode's bar, checked here at a fifth of it)
        d = float(np.abs(r["output"][b, 0, 0, :n] - one["output"][0, 0, 0, :n]).max())
        print(f"  utterance {b}: batch-64 vs batch-1 rendering max-abs {d:.3g}, SNR {_snr_db(one['output'][0, 0, 0, :n], r['output'][b, 0, 0, :n]):.1f} dB")
        assert d < 2e-3 and _snr_db(one["output"][0, 0, 0, :n], r["output"][b, 0, 0, :n]) > 45.0
    s.close()


@pytest.mark.parametrize("preset", ["medium", "high"])
def test_single_utterance_short_launch_kernels_match_the_engine(preset):
    """The reference's real call (one utterance, voice.py:350-351) runs its token- / frame-domain convs on the short-launch
    kernel (conv_sx_small.hip.hpp) and, with it switched off, on the throughput engine: same durations, same frame count,
    taps and waveform within fp32 summation-order distance."""
    from phoonnx_amd import MiSession, _ffi
    lib = _ffi.load()
    s = MiSession(_voice(preset))
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 256, (1, 200)).astype(np.int64)
    lens = np.array([200], np.int64)
    sc = np.array([0.0, 1.2, 0.0], np.float32)   # (no noise: both renderings are functions of the ids alone)
    a = s.synthesize_batch(ids, lens, sc, taps=("w_ceil", "z_p", "z"))
    assert s.stats()["sx_launches"] > 0
    prev = lib.vits_test_set_sx_small_max(0)
    try:
        b = s.synthesize_batch(ids, lens, sc, taps=("w_ceil", "z_p", "z"))
    finally:
        lib.vits_test_set_sx_small_max(prev)
    assert prev > 0
    assert np.array_equal(a["w_ceil"], b["w_ceil"]) and np.array_equal(a["y_lengths"], b["y_lengths"])
    for k in ("z_p", "z"):
        np.testing.assert_allclose(a[k], b[k], atol=2e-5, rtol=0, err_msg=k)
    d = float(np.abs(a["output"] - b["output"]).max())
    print(f"{preset}: one utterance, short-launch kernels vs engine: waveform max-abs {d:.3g}")
    assert d < 2e-5
    s.close()


def test_langid_voice_runs_and_ignores_the_language_id(tmp_path):
    """A third-party style graph that declares `langid` (voice.py:369): the feed built by TTSVoice passes through."""
    from phoonnx_amd import MiSession, SessionError
    from phoonnx_amd.synth import write_voice
    p = str(tmp_path / "lang.onnx")
    write_voice(p, "small", seed=2, extra_inputs=("langid",))
    s = MiSession(p)
    ids = np.arange(1, 31, dtype=np.int64)[None]
    feed = {"input": ids, "input_lengths": np.array([30], np.int64), "scales": np.array([0, 1, 0], np.float32),
            "langid": np.array([3], np.int64)}
    a = s.run(None, feed)[0]
    b = s.run(None, dict(feed, langid=np.array([0], np.int64)))[0]
    assert a.ndim == 4 and np.array_equal(a, b)
    with pytest.raises(SessionError):
        s.run(None, dict(feed, langid=np.zeros((1, 1), np.int64)))
    with pytest.raises(SessionError):
        s.run(None, {k: v for k, v in feed.items() if k != "langid"})   # declared inputs are required, as in onnxruntime
    s.close()


# ------------------------------------------------------------------ the N > 1 code path on one GPU

def test_open_sharded_under_rccl_world_size_1_equals_plain_open(tmp_path):
    """RCCL (backend "nccl") process group of one rank: rank 0 packs on the host, the arena goes through
    dist.broadcast on the device, its checksum is verified, the handle adopts it with a layout-only open - and renders
    exactly what a plain open renders.  In a child process (process-group state must not leak into the test session)."""
    import subprocess
    import sys
    from conftest import GOLDEN, ROOT
    code = r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29517", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
from phoonnx_amd import MiSession
from phoonnx_amd.sharding import ShardedSynthesizer, arena_checksum, open_sharded
path = sys.argv[2]
s, arena = open_sharded(path, 0, dist, force_broadcast=True)
assert arena is not None and arena.is_cuda and arena.numel() == s.arena_bytes()
plain = MiSession(path)
assert arena_checksum(arena) == arena_checksum(torch.from_numpy(np.array(plain.arena_host(), copy=True)))
rng = np.random.default_rng(0)
ids = rng.integers(0, 200, (3, 40)).astype(np.int64)
lens = np.array([40, 33, 12], np.int64)
sid = np.array([0, 3, 1], np.int64)
sc = np.array([0, 1.3, 0], np.float32)
a = s.synthesize_batch(ids, lens, sc, sid)
b = plain.synthesize_batch(ids, lens, sc, sid)
assert np.array_equal(a["y_lengths"], b["y_lengths"]) and np.array_equal(a["output"], b["output"])
s.close(); plain.close()
sh = ShardedSynthesizer(path, 0, dist, force_broadcast=True)
utts = [list(map(int, ids[i, :lens[i]])) for i in range(3)]
# (nccl backend: the shard is rendered device to device, its valid samples are packed on the GPU out of the engine's own
# output buffer, and that tensor goes into the collective - sharding.ShardedSynthesizer._gather_device)
out = sh.synthesize(utts, sc, sids=[0, 3, 1], gather=True)
assert len(out) == 3 and all(len(w) == int(b["y_lengths"][i]) * sh.hop for i, w in enumerate(out))
assert all(np.array_equal(w, b["output"][i, 0, 0, :len(w)]) for i, w in enumerate(out))      # every sample of a plain run
root = sh.synthesize(utts, sc, sids=[0, 3, 1], gather="root")
assert all(np.array_equal(w, v) for w, v in zip(out, root))
sh.close()
dist.destroy_process_group()
print("SHARDED_OK")
'''
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(GOLDEN, "sx_rb2_ms.onnx")], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0 and "SHARDED_OK" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])


def test_spline_with_16_bins_matches_oracle(tmp_path):
    """the spline-parameter buffer was sized for the reference's 10 bins (29 rows); a voice with 16 bins (47
    rows) used to run past it into the flow state.  The buffer now follows the model; durations stay exact."""
    from phoonnx_amd import MiSession
    from phoonnx_amd.synth import write_voice
    from vits_oracle import VitsOracle
    path = str(tmp_path / "bins16.onnx")
    write_voice(path, "small", seed=21, n_bins=16)
    s, o = MiSession(path), VitsOracle(path)
    rng = np.random.default_rng(16)
    B, T = 3, 50
    ids = rng.integers(0, 256, (B, T)).astype(np.int64)
    lens = np.array([T, 37, 5], np.int64)
    sc = np.array([0.5, 1.3, 0.9], np.float32)
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, 64, T * 8)).astype(np.float32)
    ref = o.infer(ids, lens, sc, None, ndp, nz)
    got = s.synthesize_batch(ids, lens, sc, None, ndp, nz, taps=("logw", "w_ceil"))
    np.testing.assert_allclose(got["logw"], ref["logw"], atol=2e-4, rtol=0)
    assert np.array_equal(got["w_ceil"], ref["w_ceil"]) and np.array_equal(got["y_lengths"], ref["y_lengths"])
    np.testing.assert_allclose(got["output"], zero_tails(ref["output"], ref["y_lengths"], s.hparam("hop")), atol=1e-3, rtol=0)
    s.close()
