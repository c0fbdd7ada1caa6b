"""The output-rate resampler without a GPU: the plan and table of vits_resample_plan against a NumPy float64 evaluation of
the definition in include/vitsmi.h ("output rate"), its refusals, the sample counts, alignments with a rate ratio, and the
Python objects that refuse a session with a rate set."""
import math
import os

import numpy as np
import pytest

import resample_ref as ref
from conftest import GOLDEN

PAIRS = [(22050, 8000), (22050, 16000), (22050, 24000), (22050, 44100), (22050, 48000), (22050, 11025), (16000, 8000),
         (24000, 22050)]


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_plan_and_table_match_the_definition(fi, fo):
    from phoonnx_amd.session import resample_plan
    L, M, K, s, _ = ref.plan(fi, fo)
    assert resample_plan(fi, fo) == (L, M, K)
    gl, gm, gk, h = resample_plan(fi, fo, table=True)
    assert (gl, gm, gk) == (L, M, K) and h.shape == (L, K) and h.dtype == np.float32
    err = float(np.abs(h.astype(np.float64) - ref.table64(fi, fo)).max())
    print(f"{fi}->{fo}: L={L} M={M} K={K} max|h - h64|={err:.3e} (bound {2.0 ** -23 * s:.3e})")
    assert err <= 2.0 ** -23 * s      # one fp32 ulp of the largest entry, k(0) = s


def test_known_plans():
    from phoonnx_amd.session import resample_plan
    assert resample_plan(22050, 8000) == (160, 441, 104)
    assert resample_plan(22050, 48000)[0] == 320
    assert resample_plan(22050, 44100)[0] == 2
    assert resample_plan(16000, 8000)[0] == 1
    assert max(L * K for L, _, K in (resample_plan(22050, fo) for fo in (8000, 16000, 24000, 44100, 48000))) == 16640


@pytest.mark.parametrize("fi,fo,word", [(22050, 0, "0"), (0, 8000, "0"), (22050, -8000, "-8000"), (-1, 8000, "-1"),
                                        (22050, 400000, "400000"), (400000, 22050, "400000")])
def test_rates_outside_the_limits_are_refused(fi, fo, word):
    from phoonnx_amd.session import SessionError, resample_plan
    with pytest.raises(SessionError, match=word):
        resample_plan(fi, fo)


def test_a_table_beyond_the_limit_is_refused_with_its_entry_count():
    from phoonnx_amd.session import SessionError, resample_plan
    L, _, K, _, _ = ref.plan(22050, 22051)
    assert L * K > 1 << 18
    with pytest.raises(SessionError, match=str(L * K)):
        resample_plan(22050, 22051)


def test_sample_counts_and_host_only_handles():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import SessionError, output_sample_counts
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True, output_rate=8000)   # the plan, no table on a device
    hop = s.hparam("hop")
    fi = int(s.meta("sample_rate") or 22050)
    assert s.resampling and s.output_rate == 8000
    assert s.last_sample_counts().shape == (0,)        # (no run on a host-only handle: counts come from the helper)
    for fo in (8000, 16000, 48000):
        s.set_output_rate(fo)
        L, M = ref.plan(fi, fo)[:2]
        n = np.array([0, 1, hop, 7 * hop], np.int64)
        want = np.array([math.ceil(int(v) * L / M) for v in n], np.int64)
        assert np.array_equal(output_sample_counts(n, fi, fo), want)
        assert np.array_equal(ref.count(n, fi, fo), want)
    with pytest.raises(SessionError, match=str(22051 * 38)):
        s.set_output_rate(22051, input_rate=22050)
    assert s.output_rate == 48000                      # a refused rate leaves the setting alone
    s.set_output_rate(fi)
    assert not s.resampling                            # the voice's own rate: the native path
    s.set_output_rate(None)
    assert s.output_rate is None and not s.resampling
    for bad in (0, -8000, 8000.0):
        with pytest.raises(SessionError, match="positive integer"):
            s.set_output_rate(bad)
    s.close()
    layout = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), layout_only=True, output_rate=16000)
    assert layout.resampling
    layout.close()


def test_alignments_with_a_rate_ratio():
    from phoonnx_amd.voice import build_alignments
    groups = [("^", [1]), ("a", [4, 0]), ("b", [5, 0]), ("c", [6]), ("$", [2])]
    dur = [2, 3, 0, 0, 0, 1, 4]
    hop = 256
    for fi, fo in ((22050, 8000), (22050, 48000), (22050, 16000)):
        L, M = ref.plan(fi, fo)[:2]
        native = build_alignments(groups, dur, hop)
        al = build_alignments(groups, dur, hop, ratio=(L, M))
        N = math.ceil(sum(dur) * hop * L / M)
        assert sum(a.num_samples for a in al) == N
        assert al[2].num_samples == 0                                  # "b": zero frames, zero samples
        pos = 0
        for a, n in zip(al, native):
            assert a.start_sample == pos == min(N, math.ceil(n.start_sample * L / M))
            assert (a.phoneme, a.phoneme_ids) == (n.phoneme, n.phoneme_ids)
            pos += a.num_samples
        # an utterance whose durations are all zero is one frame of audio, which goes to the last entry
        zero = build_alignments(groups, [0] * 7, hop, total_frames=1, ratio=(L, M))
        assert [a.num_samples for a in zero] == [0, 0, 0, 0, math.ceil(hop * L / M)]
        assert all(a.start_sample == 0 for a in zero)
    assert [vars(a) for a in build_alignments(groups, dur, hop, ratio=None)] == [vars(a) for a in build_alignments(groups, dur, hop)]


def test_pipelined_and_sharded_sessions_refuse_a_session_with_a_rate():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession, SessionError
    from phoonnx_amd.sharding import ShardedSynthesizer
    path = os.path.join(GOLDEN, "tiny_rb1.onnx")
    s = MiSession(path, host_only=True, output_rate=8000)
    with pytest.raises(SessionError, match="output rate"):
        PipelinedSession(s, parts=2)
    with pytest.raises(SessionError, match="output rate"):
        ShardedSynthesizer(path, 0, session=s)
    s.close()


def test_voice_load_refuses_an_output_rate_on_a_session_that_cannot_resample():
    from phoonnx_amd.voice import TTSVoice

    class OrtLike:
        def get_inputs(self):
            return []

        def run(self, names, feed):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="set_output_rate"):
        TTSVoice.load(os.path.join(GOLDEN, "tiny_rb1.onnx"), output_sample_rate=8000, session=OrtLike())
