"""Whole voices at production widths against a float64 rendering: the voices, the one input set, the CPU renderings and
the bound.  Shared by tests/test_fullwidth_ref_cpu.py (which checks this file's own claims) and tests/test_gpu_fullwidth.py.

The full-size tests beside this one compare the engine with the fp32 C oracle at 5e-4 (taps) and 1e-3 (waveform).  An
honest fp32 implementation sits 1e-6 .. 6e-6 from a float64 rendering of the same graph, and one conv whose weights were
rounded to fp16 - a dropped low operand plane in one launch - sits 1e-5 .. 4e-4 away: inside the old bars.  Here the
reference is `TorchVits(dtype=torch.float64)` (oracle/torch_baseline.py, pinned to the reference fixtures in that mode by
test_fullwidth_ref_cpu.py), and the bar is set by two independent honest fp32 implementations of the same graph - torch's
CPU kernels in float32 (oneDNN's blocked sums) and the C oracle (naive loops) - measured against it:

    bound(tap) = K * max(err_torch32, err_c_oracle) + 1e-7 * max|ref64|,        K = 4

with every error a max-abs over the whole tap.  Why 4: on these inputs the two witnesses differ from each other by up to
2.6x (the waveform of `high`), and test_conv_sx_f16_mode_error_is_fp32_grade allows the f16x3 arithmetic 1.5x the f32
engine's error: 2.6 * 1.5 = 3.9.  The bound is a function of the references alone; nothing in it comes from the engine.

Durations are integers behind a ceil().  `duration_margin` is evaluated on ref64 only: every valid token's
exp(logw) * length_scale lies at least GUARD (relative to the nearer integer, floor 1) from an integer, while the logw
bound is below 1e-4 - so an implementation inside its logw bound cannot move a ceil, and w_ceil / y_lengths are compared
exactly.  A voice that fails the guard gets another seed (SEEDS), never another guard."""
import os
import time

import numpy as np

from bench import voice_cache

K = 4
FLOOR = 1e-7
GUARD = 1e-3
TAPS = ("x", "m_p", "logs_p", "logw", "z_p", "z")
ENGINE_TAPS = ("x", "m_p", "logs_p", "logw", "w_ceil", "z_p", "z")

# name -> (preset of phoonnx_amd/synth.py, overrides): the files test_gpu_fullsize.py and bench.py use, where they share one
VOICES = {
    "high": ("high", {}),                                       # 192 wide, dk = 96, ResBlock1 512 -> 256 -> 128 -> 64 -> 32
    "medium_ms4": ("medium", {"n_speakers": 4}),                # every conditioning path
    "medium_dp": ("medium", {"use_sdp": False}),                # the plain duration predictor
    # the x-low shape: enc_sx = gen_sx = 1, but the flow's half = 48 is no multiple of 32 - the coupling pre / post convs
    # leave the split-operand engine while the WN layers stay on it
    "medium_w96": ("medium", {"hidden_channels": 96, "inter_channels": 96, "filter_channels": 384}),
    "small": ("small", {}),                                     # enc_sx = gen_sx = 0: the f32 engine throughout
    "small_raw": ("small", {"upsample_initial_channel": 128, "upsample_rates": (8, 4), "upsample_kernel_sizes": (16, 8)}),
}
SEEDS = {name: 99 for name in VOICES}
SEEDS["medium_dp"] = 100    # (with 99 one token of ref64 lies 9.4e-4 from an integer: inside the guard; 100 is the next seed)

B, T, LENS = 3, 24, (24, 17, 1)
SCALES = (0.667, 1.0, 0.8)                                      # noise_scale, length_scale, noise_w
VOC_B, VOC_F = 2, 48                                            # an interior beyond gen_rf_frames (12 - 15 here)

_PATHS, _MODELS, _REF = {}, {}, {}


def voice_path(name):
    """The voice's .onnx in bench.voice_cache(), written on first touch (as test_gpu_fullsize._voice does)."""
    if name not in _PATHS:
        from phoonnx_amd.synth import write_voice
        preset, over = VOICES[name]
        tag = preset + "".join(f"_{k}{v}" for k, v in sorted(over.items()))
        tag = "".join(ch if ch.isalnum() or ch in "_-" else "" for ch in tag)
        cache = voice_cache()
        path = os.path.join(cache, f"synth_{tag}.onnx")
        if not os.path.exists(path):
            os.makedirs(cache, exist_ok=True)
            write_voice(path + ".tmp", preset, seed=1234, **over)
            os.replace(path + ".tmp", path)
        _PATHS[name] = path
    return _PATHS[name]


def n_speakers(name):
    return VOICES[name][1].get("n_speakers", 1)


def inter_channels(name):
    from phoonnx_amd.synth import hparams
    preset, over = VOICES[name]
    return hparams(preset, **over)["inter_channels"]


def inputs(name):
    """The whole-path input set: B = 3, T = 24, lens 24 / 17 / 1, injected noise, one seed."""
    rng = np.random.default_rng(SEEDS[name])
    lens = np.array(LENS, np.int64)
    ids = np.zeros((B, T), np.int64)
    for b in range(B):
        ids[b, :lens[b]] = rng.integers(0, 256, lens[b])
    ndp = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, inter_channels(name), 12 * T)).astype(np.float32)
    sid = rng.integers(0, 4, B).astype(np.int64)
    return dict(ids=ids, lens=lens, scales=np.array(SCALES, np.float32), sid=sid if n_speakers(name) > 1 else None,
                noise_dp=ndp, noise_z=nz)


def vocoder_inputs(name):
    """The vocoder-only input: z standard normal [2, inter, 48], speakers 0 and 1 where the voice has speakers."""
    rng = np.random.default_rng([SEEDS[name], 1])
    z = rng.standard_normal((VOC_B, inter_channels(name), VOC_F)).astype(np.float32)
    return dict(z=z, sid=np.array([0, 1], np.int64) if n_speakers(name) > 1 else None)


def _args(inp):
    return (inp["ids"], inp["lens"], inp["scales"], inp["sid"], inp["noise_dp"], inp["noise_z"])


def torch_model(name, dtype):
    import torch
    from torch_baseline import TorchVits
    key = (name, dtype)
    if key not in _MODELS:
        _MODELS[key] = TorchVits(voice_path(name), dtype={"f64": torch.float64, "f32": torch.float32}[dtype])
    return _MODELS[key]


def torch_vocoder(m, z, sid):
    """generator(z, g) of a TorchVits in its own dtype -> [B, 1, 1, S] (the shape of VitsOracle.vocoder / MiSession.vocoder)"""
    import torch
    with torch.no_grad():
        g = None
        if m.gin:
            g = m.t["emb_g.weight"][torch.as_tensor(np.asarray(sid, np.int64))].unsqueeze(-1)
        return m.generator(torch.as_tensor(np.asarray(z, np.float32)).to(m.dtype), g).unsqueeze(1).numpy()


def renderings(name):
    """-> {"ref64", "torch32", "c"}: the whole-path renderings of inputs(name), plus "seconds" per rendering.  Rendered once
    per process and left unchanged."""
    key = (voice_path(name), "whole")
    if key not in _REF:
        from vits_oracle import VitsOracle
        inp, out, sec = inputs(name), {}, {}
        for tag, run in (("ref64", lambda: torch_model(name, "f64").infer(*_args(inp))),
                         ("torch32", lambda: torch_model(name, "f32").infer(*_args(inp))),
                         ("c", lambda: VitsOracle(voice_path(name)).infer(*_args(inp)))):
            t0 = time.perf_counter()
            out[tag] = run()
            sec[tag] = time.perf_counter() - t0
        out["seconds"] = sec
        _REF[key] = out
    return _REF[key]


def vocoder_renderings(name):
    """-> {"ref64", "torch32", "c"}: each {"output": [2, 1, 1, 48 hop]} for vocoder_inputs(name)."""
    key = (voice_path(name), "vocoder")
    if key not in _REF:
        from vits_oracle import VitsOracle
        inp = vocoder_inputs(name)
        _REF[key] = {"ref64": {"output": torch_vocoder(torch_model(name, "f64"), inp["z"], inp["sid"])},
                     "torch32": {"output": torch_vocoder(torch_model(name, "f32"), inp["z"], inp["sid"])},
                     "c": {"output": VitsOracle(voice_path(name)).vocoder(inp["z"], inp["sid"])}}
    return _REF[key]


def max_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max())


def witness_errors(r, tap):
    """(torch float32, C oracle): max-abs against ref64 over the whole tap"""
    return max_err(r["torch32"][tap], r["ref64"][tap]), max_err(r["c"][tap], r["ref64"][tap])


def bound(r, tap):
    """The bar of one tap of `r` (renderings() or vocoder_renderings()): a function of the three CPU renderings alone."""
    return K * max(witness_errors(r, tap)) + FLOOR * float(np.abs(r["ref64"][tap]).max())


def duration_margin(name):
    """The smallest distance of a valid token's exp(logw) * length_scale to an integer in ref64, relative to the nearer
    integer (floor 1)."""
    ref, inp = renderings(name)["ref64"], inputs(name)
    assert ref["logw"].dtype == np.float64
    w = np.exp(ref["logw"][:, 0, :]) * float(inp["scales"][1])
    near = np.rint(w)
    valid = np.arange(T)[None, :] < inp["lens"][:, None]
    return float((np.abs(w - near) / np.maximum(near, 1.0))[valid].min())


def fp16_weights_model(name, conv):
    """The float32 witness with one conv's weights rounded to fp16: what a dropped low operand plane in that launch gives."""
    import torch
    from torch_baseline import TorchVits
    m = TorchVits(voice_path(name))
    m.t[conv + ".weight"] = m.t[conv + ".weight"].to(torch.float16).to(torch.float32)
    return m
