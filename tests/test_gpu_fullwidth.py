"""Whole voices at production widths held to fp32 grade: the engine against a float64 rendering of the graph, inside a bar
that two honest fp32 CPU implementations set (tests/fullwidth_ref.py; the bar's own claims - the guard on the durations, and
that it catches ONE conv of fp16 grade which the 5e-4 / 1e-3 bars of test_gpu_fullsize.py pass - are checked on the CPU by
tests/test_fullwidth_ref_cpu.py).  The launch plan of a voice is what is under test: packing, flags, slopes, conditioning
rows.  Tile seams are the kernel tests' job, so the inputs are small: B = 3 x 24 tokens (lens 24 / 17 / 1), and a
vocoder-only z of 2 x 48 frames, which isolates the generator from upstream error.

Arithmetics: the default (f16x3 products on the split-operand engine where the voice opens on it), "bf16x6" (six exact
products), and "f32" (VITSMI_ENC_ENGINE=f32 with VITSMI_GEN_ENGINE=f32: the f32-MFMA engine for every conv).  The
reduced-precision "f16" vocoder declares 1e-2 and is not held to this bar."""
import numpy as np
import pytest

import fullwidth_ref as fw
from conftest import zero_tails

pytestmark = pytest.mark.gpu

CASES = [(name, "default") for name in fw.VOICES] + \
        [(name, arith) for name in ("high", "medium_ms4") for arith in ("bf16x6", "f32")]


def _open(monkeypatch, name, arith):
    from phoonnx_amd import MiSession
    if arith == "f32":
        monkeypatch.setenv("VITSMI_ENC_ENGINE", "f32")
        monkeypatch.setenv("VITSMI_GEN_ENGINE", "f32")
    s = MiSession(fw.voice_path(name), gen_precision="bf16x6" if arith == "bf16x6" else None)
    # where the case runs: the f32 engine throughout for "f32" and for `small`; otherwise the generator on the split-operand
    # engine in the arithmetic asked for, and the encoder with it in the default arithmetic only (the exact mode keeps the
    # encoder on the f32 engine: it is what a range-guard fallback falls back to)
    if arith == "f32" or name == "small":
        assert s.hparam("enc_sx") == 0 and s.hparam("gen_sx") == 0
    else:
        assert s.hparam("gen_sx") == 1 and s.hparam("gen_nprod") == (6 if arith == "bf16x6" else 2)
        if name != "small_raw":
            assert s.hparam("enc_sx") == (1 if arith == "default" else 0)
    return s


def _ran_where_it_claims(s):
    st = s.stats()
    if s.hparam("gen_sx") == 1:
        assert st["sx_launches"] > 0
    assert st["f16_saturated"] == 0 and s.range_fallbacks == 0          # (no silent reopening with another arithmetic)


@pytest.mark.parametrize("name,arith", CASES)
def test_whole_path_is_fp32_grade_against_float64(monkeypatch, name, arith):
    r, inp = fw.renderings(name), fw.inputs(name)
    ref = r["ref64"]
    s = _open(monkeypatch, name, arith)
    try:
        got = s.synthesize_batch(inp["ids"], inp["lens"], inp["scales"], inp["sid"], inp["noise_dp"], inp["noise_z"],
                                 taps=fw.ENGINE_TAPS)
        _ran_where_it_claims(s)
        hop = s.hparam("hop")
    finally:
        s.close()
    assert np.array_equal(got["w_ceil"], ref["w_ceil"])                 # integer durations: exact
    assert np.array_equal(got["y_lengths"], ref["y_lengths"])
    want = dict(ref, output=zero_tails(ref["output"], ref["y_lengths"], hop))
    errs = {k: fw.max_err(got[k], want[k]) for k in fw.TAPS + ("output",)}
    print(f"{name} {arith}: err / max(witness err): "
          + "  ".join(f"{k} {errs[k] / max(fw.witness_errors(r, k)):.2f}" for k in errs)
          + "   (bound = %d x + floor)" % fw.K)
    for k, e in errs.items():
        assert e <= fw.bound(r, k), (k, e, fw.bound(r, k), fw.witness_errors(r, k))
    for b in range(fw.B):                                               # exact zeros behind each row's end
        assert not got["output"][b, 0, 0, int(ref["y_lengths"][b]) * hop:].any(), b


@pytest.mark.parametrize("name,arith", CASES)
def test_vocoder_only_is_fp32_grade_against_float64(monkeypatch, name, arith):
    v, inp = fw.vocoder_renderings(name), fw.vocoder_inputs(name)
    s = _open(monkeypatch, name, arith)
    try:
        got = s.vocoder(inp["z"], inp["sid"])
        _ran_where_it_claims(s)
    finally:
        s.close()
    err = fw.max_err(got, v["ref64"]["output"])
    print(f"{name} {arith}: vocoder-only err / max(witness err): {err / max(fw.witness_errors(v, 'output')):.2f}"
          "   (bound = %d x + floor)" % fw.K)
    assert err <= fw.bound(v, "output"), (err, fw.bound(v, "output"), fw.witness_errors(v, "output"))
