"""tests/fullwidth_ref.py on the CPU: the float64 mode of oracle/torch_baseline.py pinned to the reference fixtures, the
duration guard on every voice, and a control that shows the bound telling fp32 grade from fp16 grade in ONE conv of a whole
voice - which the 5e-4 / 1e-3 bars of the full-size tests cannot."""
import os

import numpy as np
import pytest

import fullwidth_ref as fw
from conftest import ALL_PRESETS, GOLDEN, case_get, golden_cases

ALL_TAPS = fw.TAPS + ("output",)


@pytest.mark.parametrize("preset", ALL_PRESETS)
def test_float64_mode_matches_reference_goldens_and_the_float32_mode(preset):
    import torch
    from torch_baseline import TorchVits
    path = os.path.join(GOLDEN, preset + ".onnx")
    m64, m32 = TorchVits(path, dtype=torch.float64), TorchVits(path)
    assert all(v.dtype == torch.float64 for v in m64.t.values()) and all(v.dtype == torch.float32 for v in m32.t.values())
    assert torch.get_default_dtype() == torch.float32                   # (the mode is the object's, not the process's)
    g = np.load(os.path.join(GOLDEN, preset + ".npz"))
    for c in golden_cases(g):
        args = [case_get(g, c, k) for k in ("ids", "lens", "scales", "sid", "noise_dp", "noise_z")]
        r, r32 = m64.infer(*args), m32.infer(*args)
        assert np.array_equal(r["w_ceil"], case_get(g, c, "out_w_ceil")), (preset, c)
        assert np.array_equal(r["y_lengths"], case_get(g, c, "out_y_lengths")), (preset, c)
        assert r["y_lengths"].dtype == np.int64
        for k in ALL_TAPS + ("w_ceil",):
            assert r[k].dtype == np.float64 and r32[k].dtype == np.float32, k     # the default mode returns float32 as before
            assert r[k].shape == r32[k].shape
        # the tolerances of test_torch_baseline_matches_reference_goldens ...
        for k in fw.TAPS:
            np.testing.assert_allclose(r[k], case_get(g, c, "out_" + k), atol=1e-4, rtol=0, err_msg=f"{preset}/{c}/{k}")
        np.testing.assert_allclose(r["output"], case_get(g, c, "out_output"), atol=1e-5, rtol=0)
        # ... and the two modes of one restatement
        for k in ALL_TAPS:
            np.testing.assert_allclose(r[k], r32[k], atol=1e-5, rtol=0, err_msg=f"{preset}/{c}/{k} f64 vs f32")


@pytest.mark.parametrize("name", list(fw.VOICES))
def test_guard_holds_and_witnesses_give_the_reference_durations(name):
    r = fw.renderings(name)
    ref = r["ref64"]
    for k in ALL_TAPS + ("w_ceil",):
        assert ref[k].dtype == np.float64, k
    margin = fw.duration_margin(name)
    errs = {k: fw.witness_errors(r, k) for k in ALL_TAPS}
    print(f"{name}: frames {ref['y_lengths'].tolist()}, duration margin {margin:.3g}, seconds "
          + ", ".join(f"{k} {v:.2f}" for k, v in r["seconds"].items()))
    for k in ALL_TAPS:
        print(f"  {k:7s} torch32 {errs[k][0]:.3g}  c {errs[k][1]:.3g}  bound {fw.bound(r, k):.3g}  max|ref64| {np.abs(ref[k]).max():.3g}")
    assert margin >= fw.GUARD, margin
    assert fw.bound(r, "logw") < 1e-4                                   # (what the guard's argument rests on)
    for w in ("torch32", "c"):
        assert np.array_equal(r[w]["w_ceil"], ref["w_ceil"]), w
        assert np.array_equal(r[w]["y_lengths"], ref["y_lengths"]), w
    inp = fw.inputs(name)
    assert np.array_equal(ref["w_ceil"].sum(1).clip(1), ref["y_lengths"]) and not ref["w_ceil"][2, 1:].any()
    assert int(ref["y_lengths"].max()) <= inp["noise_z"].shape[2]
    # the comparison is not vacuous
    assert 0.02 < np.abs(ref["output"]).max() < 0.999
    for k in fw.TAPS:
        assert np.abs(ref[k]).max() > 0.05, k
    v = fw.vocoder_renderings(name)
    assert v["ref64"]["output"].dtype == np.float64
    assert v["ref64"]["output"].shape == v["c"]["output"].shape == v["torch32"]["output"].shape
    e = fw.witness_errors(v, "output")
    print(f"  vocoder-only: torch32 {e[0]:.3g}  c {e[1]:.3g}  bound {fw.bound(v, 'output'):.3g}")
    assert 0.02 < np.abs(v["ref64"]["output"]).max() < 0.999


def test_the_voices_open_on_the_engines_the_cases_are_named_for():
    from phoonnx_amd import MiSession
    want = {"high": (1, 1), "medium_ms4": (1, 1), "medium_dp": (1, 1), "medium_w96": (1, 1), "small": (0, 0)}
    for name, engines in want.items():
        s = MiSession(fw.voice_path(name), host_only=True)
        assert (s.hparam("enc_sx"), s.hparam("gen_sx")) == engines, name
        assert s.hparam("inter") == fw.inter_channels(name)
        assert fw.VOC_F > s.hparam("gen_rf_frames") * 2, name           # (the vocoder-only input has an interior)
        s.close()
    s = MiSession(fw.voice_path("small_raw"), host_only=True)
    assert s.hparam("gen_sx") == 1
    s.close()


# one conv of `high` with its weights rounded to fp16 in the float32 witness: the tap it shows at
WHOLE_PATH_CONTROLS = [("enc_p.encoder.ffn_layers.3.conv_1", "z"), ("flow.flows.2.enc.in_layers.1", "z"),
                       ("dec.ups.0", "output"), ("dec.resblocks.4.convs2.1", "output")]


@pytest.mark.parametrize("conv,tap", WHOLE_PATH_CONTROLS)
def test_bound_catches_one_fp16_grade_conv_that_the_old_tolerances_pass(conv, tap):
    r, inp = fw.renderings("high"), fw.inputs("high")
    got = fw.fp16_weights_model("high", conv).infer(*fw._args(inp))
    assert np.array_equal(got["w_ceil"], r["ref64"]["w_ceil"]) and np.array_equal(got["y_lengths"], r["ref64"]["y_lengths"])
    errs = {k: fw.max_err(got[k], r["ref64"][k]) for k in ALL_TAPS}
    print(f"{conv}: {tap} error {errs[tap]:.3g} = {errs[tap] / max(fw.witness_errors(r, tap)):.1f} x witness, "
          f"bound {fw.bound(r, tap):.3g}")
    assert errs[tap] > fw.bound(r, tap), (errs[tap], fw.bound(r, tap))  # the new bar sees it ...
    for k in fw.TAPS:
        assert errs[k] < 5e-4, k                                        # ... where test_fullsize_pipeline_matches_oracle's
    assert errs["output"] < 1e-3                                        #     tolerances do not
    # (and an honest witness stays inside: the bar does not fire on fp32 grade)
    for k in ALL_TAPS:
        assert max(fw.witness_errors(r, k)) < fw.bound(r, k)


def test_vocoder_bound_catches_an_fp16_grade_conv_of_the_last_stage():
    """dec.resblocks.11.convs1.2 (32 channels, the last stage): 1.5x over the whole-path waveform bound only, so it is held
    against the vocoder-only bound, where nothing upstream widens the witnesses' error."""
    conv = "dec.resblocks.11.convs1.2"
    v, inp = fw.vocoder_renderings("high"), fw.vocoder_inputs("high")
    got = fw.torch_vocoder(fw.fp16_weights_model("high", conv), inp["z"], inp["sid"])
    err = fw.max_err(got, v["ref64"]["output"])
    print(f"{conv}: vocoder-only error {err:.3g} = {err / max(fw.witness_errors(v, 'output')):.1f} x witness, "
          f"bound {fw.bound(v, 'output'):.3g}")
    assert fw.bound(v, "output") < err < 1e-3
