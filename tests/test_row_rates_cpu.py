"""A rate per row (include/vitsmi.h, "output rate per row") without a GPU: the three entries are declared and exported, a
host-only handle validates and keeps the rows' plans, the refusals name the row and leave the previous setting alone, the
per-row sample counts, and the sessions and voices that cannot carry row rates say so."""
import math
import os
import re

import numpy as np
import pytest

import resample_ref as ref
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(GOLDEN, "tiny_rb1.onnx")


def _host():
    from phoonnx_amd import MiSession
    return MiSession(PATH, host_only=True)


def test_the_entries_are_declared_and_exported():
    from phoonnx_amd import _ffi
    lib = _ffi.load()
    header = open(os.path.join(ROOT, "include", "vitsmi.h")).read()
    for name in ("vits_set_output_rates", "vits_last_sample_rates", "vits_test_resample_rows"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    assert re.search(r"#define VITS_MAX_ROW_RATES 8\b", header)


def test_a_host_only_handle_keeps_the_rows_and_validates():
    s = _host()
    fi = int(s.meta("sample_rate") or 22050)
    assert s.output_rates is None
    s.set_output_rates([8000, None, 48000, 0, fi, 8000])
    assert s.output_rates == (8000, 0, 48000, 0, fi, 8000) and s.output_rate is None
    assert s.last_sample_rates().shape == (0,)                 # (no run on a host-only handle)
    # eight distinct resampling rates are admitted - native rows and repeats do not count
    eight = [8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000]
    s.set_output_rates(eight + [0, fi, 8000])
    assert s.output_rates == tuple(eight + [0, fi, 8000])
    s.set_output_rates(None)
    assert s.output_rates is None
    s.close()
    from phoonnx_amd import MiSession
    layout = MiSession(PATH, layout_only=True)
    layout.set_output_rates([16000, 0])
    assert layout.output_rates == (16000, 0)
    layout.close()


@pytest.mark.parametrize("rates,row,word", [
    ([8000, 11025, 12000, 16000, 24000, 32000, 44100, 48000, 0, 96000], 9, "96000"),    # the ninth distinct rate
    ([8000, 0, 400000], 2, "400000"),
    ([0, 22051], 1, str(22051 * 38)),                                                    # 22050 -> 22051: the table's entries
])
def test_refusals_name_the_row_and_leave_the_previous_setting(rates, row, word):
    from phoonnx_amd.session import SessionError
    s = _host()
    s.set_output_rates([16000, 0, 8000])
    with pytest.raises(SessionError, match=rf"row {row}\b.*{word}"):
        s.set_output_rates(rates, input_rate=22050)
    assert s.output_rates == (16000, 0, 8000)                  # a refused call leaves the setting alone
    # ... in the engine too: the handle still holds the three rows (a host-only handle cannot run; clearing and setting work)
    s.set_output_rates([16000, 0, 8000])
    s.close()


def test_a_refusal_leaves_a_handle_rate_in_place():
    from phoonnx_amd.session import SessionError
    s = _host()
    s.set_output_rate(8000)
    with pytest.raises(SessionError, match=r"row 0\b.*400000"):
        s.set_output_rates([400000])
    assert s.output_rate == 8000 and s.output_rates is None and s.resampling
    s.close()


def test_python_side_refusals():
    from phoonnx_amd.session import SessionError
    s = _host()
    for bad in ([], [8000.0], [-1], ["8000"]):
        with pytest.raises(SessionError):
            s.set_output_rates(bad)
    assert s.output_rates is None
    s.close()


def test_a_handle_rate_clears_the_row_rates_and_the_reverse():
    s = _host()
    s.set_output_rates([8000, 0])
    s.set_output_rate(16000)
    assert s.output_rates is None and s.output_rate == 16000 and s.resampling
    s.set_output_rates([0, 48000])
    assert s.output_rate is None and not s.resampling and s.output_rates == (0, 48000)
    s.set_output_rate(None)
    assert s.output_rates is None and s.output_rate is None
    s.close()


def test_the_c_entries_directly():
    """the handle's own state, not the session's mirror of it: clearing, a NULL array, a negative rate and a negative count"""
    from phoonnx_amd import _ffi
    s = _host()
    lib, h = s._lib, s._h
    rates = np.array([8000, 0, -5], np.int32)
    assert lib.vits_set_output_rates(h, 0, _ffi.ptr(rates), 3) != 0 and "row 2" in s._err() and "-5" in s._err()
    assert lib.vits_set_output_rates(h, 0, _ffi.ptr(rates), -1) != 0
    assert lib.vits_set_output_rates(h, 0, _ffi.ptr(rates), 2) == 0
    assert lib.vits_set_output_rates(h, 0, None, 2) == 0           # a NULL array clears
    assert lib.vits_set_output_rates(h, 0, _ffi.ptr(rates), 0) == 0
    buf = np.zeros(4, np.int32)
    assert lib.vits_last_sample_rates(h, _ffi.ptr(buf), 4) == 0    # no run: no rows
    assert lib.vits_last_sample_rates(None, _ffi.ptr(buf), 4) != 0
    s.close()


def test_sample_counts_per_row():
    from phoonnx_amd.session import output_sample_counts
    s = _host()
    hop, fi = s.hparam("hop"), int(s.meta("sample_rate") or 22050)
    s.close()
    n = np.array([0, 1, hop, 7 * hop], np.int64)
    for rates in ([8000, 16000, 48000, 8000], [None, 0, fi, 44100], [48000] * 4):
        want = []
        for v, r in zip(n, rates):
            L, M = (1, 1) if r in (None, 0, fi) else ref.plan(fi, r)[:2]
            want.append(math.ceil(int(v) * L / M))
        got = output_sample_counts(n, fi, rates)
        assert got.dtype == np.int64 and np.array_equal(got, want), (rates, got, want)
    assert np.array_equal(output_sample_counts(n, fi, [8000] * 4), output_sample_counts(n, fi, 8000))
    from phoonnx_amd.session import SessionError
    with pytest.raises(SessionError, match="rates"):
        output_sample_counts(n, fi, [8000, 16000])


def test_pipelined_and_sharded_sessions_refuse_a_session_with_row_rates():
    from phoonnx_amd.session import PipelinedSession, SessionError
    from phoonnx_amd.sharding import ShardedSynthesizer
    s = _host()
    s.set_output_rates([8000, 0])
    with pytest.raises(SessionError, match="per-row output rates"):
        PipelinedSession(s, parts=2)
    with pytest.raises(SessionError, match="per-row output rates"):
        ShardedSynthesizer(PATH, 0, session=s)
    s.close()


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def _voice(session):
    from phoonnx_amd.config import PhonemeType, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    cfg = VoiceConfig(num_symbols=64, num_speakers=1, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={c: [1 + i] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


class _OrtLike:
    """a session that neither delivers nor resamples"""

    def get_inputs(self):
        return []

    def run(self, names, feed):
        raise AssertionError("not reached")


class _DeliversOnly(_OrtLike):
    def synthesize_delivered(self, *a, **kw):
        raise AssertionError("not reached")


@pytest.mark.parametrize("session", [_OrtLike(), _DeliversOnly()])
@pytest.mark.parametrize("kw", [{"output_sample_rates": [8000]}, {"encodings": ["ulaw"]}])
def test_a_voice_on_a_session_without_row_rates_raises(session, kw):
    voice = _voice(session)
    with pytest.raises(ValueError, match="set_output_rates"):
        voice.synthesize_requests_encoded([("ab", None)], **kw)


def test_a_voice_checks_one_value_per_request():
    s = _host()                            # (has both methods: the checks in front of the first run are what is tested)
    voice = _voice(s)
    with pytest.raises(ValueError, match="one value per request"):
        voice.synthesize_requests_encoded([("ab", None)], output_sample_rates=[8000, 16000])
    with pytest.raises(ValueError, match="positive integers"):
        voice.synthesize_requests_encoded([("ab", None)], output_sample_rates=[-8000])
    with pytest.raises(ValueError):
        voice.synthesize_requests_encoded([("ab", None)], encodings=["mp3"])
    s.close()
