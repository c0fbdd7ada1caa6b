"""Timing control without a GPU: phonemes_to_id_groups against the reference-generated grid of phonemes_to_ids, the pure
alignment builder, and the Python-side validation of `durations` / `token_rate` (raised before anything reaches a handle)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

from phoonnx_amd import MiSession, SessionError
from phoonnx_amd.phoneme_ids import BlankBetween, phonemes_to_id_groups, phonemes_to_ids
from phoonnx_amd.voice import AudioChunk, PhonemeAlignment, build_alignments


@pytest.fixture(scope="module")
def G():
    with open(os.path.join(GOLDEN, "frontend.json"), encoding="utf-8") as f:
        return json.load(f)


def _flat(groups):
    return [i for _, ids in groups for i in ids]


# ------------------------------------------------------------------ phonemes_to_id_groups

def test_groups_flatten_to_the_reference_ids(G):
    n = 0
    for case in G["phonemes_to_ids"]:
        id_map = None if case["map"] == "default" else G["id_maps"][case["map"]]
        kw = dict(case["kw"])
        kw["blank_between"] = BlankBetween(kw["blank_between"])
        if case["error"]:
            with pytest.raises(Exception) as ei:
                phonemes_to_id_groups(list(case["phonemes"]), id_map=id_map, **kw)
            assert type(ei.value).__name__ == case["error"], case
        else:
            groups = phonemes_to_id_groups(list(case["phonemes"]), id_map=id_map, **kw)
            assert _flat(groups) == case["ids"], case
            assert all(isinstance(ids, list) for _, ids in groups)
        n += 1
    assert n == len(G["phonemes_to_ids"]) > 2000


MAP = {"_": [0], "^": [1], "$": [2], " ": [3], "a": [10], "b": [11], "c": [12], "ai": [20, 21], "#": [4]}


def test_groups_bos_eos_and_blanks_behind_their_token():
    g = phonemes_to_id_groups(list("ab"), MAP)
    # bos takes the leading blank, every phoneme the blank behind it (the last one: the blank at the end), eos stands alone
    assert g == [("^", [1, 0]), ("a", [10, 0]), ("b", [11, 0]), ("$", [2])]
    assert _flat(g) == phonemes_to_ids(list("ab"), MAP)


def test_groups_leading_blank_without_bos_is_its_own_entry():
    g = phonemes_to_id_groups(list("ab"), MAP, bos_token=None, eos_token=None)
    assert g == [("_", [0]), ("a", [10, 0]), ("b", [11, 0])]
    assert _flat(g) == phonemes_to_ids(list("ab"), MAP, bos_token=None, eos_token=None)
    # no blank at the start either: the first entry is the first phoneme
    g = phonemes_to_id_groups(list("ab"), MAP, bos_token=None, eos_token=None, blank_at_start=False)
    assert g == [("a", [10, 0]), ("b", [11, 0])]


def test_groups_word_separator_without_whitespace():
    kw = dict(include_whitespace=False, word_sep_token="#")
    g = phonemes_to_id_groups(list("a b"), MAP, **kw)
    # the space becomes the word separator (token: the separator's own string), and one more closes the utterance
    assert g == [("^", [1, 0]), ("a", [10, 0]), ("#", [4, 0]), ("b", [11, 0]), ("#", [4, 0]), ("$", [2])]
    assert _flat(g) == phonemes_to_ids(list("a b"), MAP, **kw)


def test_groups_multi_character_key():
    g = phonemes_to_id_groups(list("bai"), MAP)
    assert g == [("^", [1, 0]), ("b", [11, 0]), ("ai", [20, 21, 0]), ("$", [2])]
    assert _flat(g) == phonemes_to_ids(list("bai"), MAP)


def test_groups_missing_phoneme_has_no_entry():
    g = phonemes_to_id_groups(list("azb"), MAP)
    assert [t for t, _ in g] == ["^", "a", "b", "$"]
    assert _flat(g) == phonemes_to_ids(list("azb"), MAP)
    assert phonemes_to_id_groups([], MAP) == []


# ------------------------------------------------------------------ build_alignments

def test_alignments_are_cumulative_and_sum_to_the_audio():
    groups = [("^", [1, 0]), ("a", [10, 0]), ("b", [11]), ("$", [2])]
    dur = [1, 0, 3, 2, 0, 4, 9, 9]   # (one per id; a padded row may be longer)
    hop = 256
    al = build_alignments(groups, dur, hop)
    assert [a.phoneme for a in al] == ["^", "a", "b", "$"]
    assert [a.phoneme_ids for a in al] == [[1, 0], [10, 0], [11], [2]]
    assert [a.num_samples for a in al] == [1 * hop, 5 * hop, 0, 4 * hop]       # a zero-duration token: 0 samples
    assert [a.start_sample for a in al] == [0, 1 * hop, 6 * hop, 6 * hop]
    assert sum(a.num_samples for a in al) == sum(dur[:6]) * hop
    assert all(isinstance(a, PhonemeAlignment) for a in al)
    # all durations zero: the engine still renders max(1, sum) = 1 frame, which goes to the last entry
    al = build_alignments(groups, [0] * 6, hop, total_frames=1)
    assert sum(a.num_samples for a in al) == hop and al[-1].num_samples == hop
    assert build_alignments(groups, np.array(dur), hop, total_frames=10) == build_alignments(groups, dur, hop)


def test_audio_chunk_field_defaults_to_none():
    c = AudioChunk(sample_rate=22050, sample_width=2, sample_channels=1, audio_float_array=np.zeros(4, np.float32))
    assert c.phoneme_alignments is None


class _OrtLike:
    """the onnxruntime duck type: get_inputs() / run() only"""

    def get_inputs(self):
        from phoonnx_amd.session import NodeArg
        return [NodeArg(n, "", []) for n in ("input", "input_lengths", "scales")]

    def run(self, names, feed):
        return [np.full((1, 1, 1, 256 * feed["input"].shape[1]), 0.25, np.float32)]


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(x.strip()) for x in text.split(".") if x.strip()]


def test_alignments_are_ignored_by_a_session_that_reports_no_durations():
    from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
    from phoonnx_amd.voice import TTSVoice
    cfg = VoiceConfig(num_symbols=32, num_speakers=1, num_langs=1, sample_rate=22050, lang_code="en",
                      phoneme_id_map={k: v for k, v in MAP.items() if len(k) == 1}, phoneme_type=PhonemeType.RAW,
                      alphabet=None, phonemizer_model=None)
    voice = TTSVoice(session=_OrtLike(), config=cfg, phonemizer=_Phon(), dedupe_sentences=True)
    plain = list(voice.synthesize("ab. ca"))
    asked = list(voice.synthesize("ab. ca", alignments=True))
    assert len(plain) == len(asked) == 2
    for p, a in zip(plain, asked):
        assert a.phoneme_alignments is None and np.array_equal(p.audio_float_array, a.audio_float_array)
    req = voice.synthesize_requests([("ab. ca", None)], alignments=True)
    assert [c.phoneme_alignments for c in req[0]] == [None, None]
    # the grouped front end is the flat one
    groups = voice._sentence_groups("ab. ca", SynthesisConfig())
    assert [_flat(g) for g in groups] == voice._sentence_ids("ab. ca", SynthesisConfig())


# ------------------------------------------------------------------ validation in front of the handle

@pytest.fixture(scope="module")
def host_session():
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    yield s
    s.close()


IDS = np.ones((2, 6), np.int64)
LENS = np.array([6, 4], np.int64)
SC = np.array([0.667, 1.0, 0.8], np.float32)


def _bad_calls():
    ok_d = np.ones((2, 6), np.int64)
    ok_r = np.ones((2, 6), np.float32)
    neg = ok_d.copy()
    neg[1, 2] = -1
    nan = ok_r.copy()
    nan[0, 3] = np.nan
    negr = ok_r.copy()
    negr[1, 1] = -0.5
    return [
        ("durations", dict(durations=np.ones((2, 5), np.int64))),
        ("durations", dict(durations=np.ones((6,), np.int64))),
        ("durations", dict(durations=np.ones((2, 6), np.float32))),
        ("durations[1,2]", dict(durations=neg)),
        ("token_rate[0,3]", dict(token_rate=nan)),
        ("token_rate[1,1]", dict(token_rate=negr)),
        ("token_rate", dict(token_rate=np.ones((3, 6), np.float32))),
        ("token_rate", dict(token_rate=np.ones((2, 6), np.int64))),
        ("'durations' and 'token_rate'", dict(durations=ok_d, token_rate=ok_r)),
    ]


@pytest.mark.parametrize("names,kw", _bad_calls())
def test_bad_timing_arguments_are_named_before_the_handle_is_touched(host_session, names, kw):
    from phoonnx_amd.session import PipelinedSession
    calls = [lambda: host_session.synthesize_batch(IDS, LENS, SC, **kw),
             lambda: host_session.synthesize_stream(IDS, LENS, SC, **kw)]
    for call in calls:
        with pytest.raises(SessionError) as ei:
            call()
        assert names in str(ei.value) and "host-only" not in str(ei.value), str(ei.value)
    # PipelinedSession.synthesize_batch checks the same before it deals rows to its parts
    p = PipelinedSession.__new__(PipelinedSession)
    with pytest.raises(SessionError) as ei:
        p.synthesize_batch(IDS, LENS, SC, **kw)
    assert names in str(ei.value)


def test_valid_timing_arguments_reach_the_handle(host_session):
    """... and only then does a host-only handle refuse to run: the checks above are not what stopped the call.  Values
    behind lens[b] are ignored, integer dtypes of any width are durations."""
    d = np.ones((2, 6), np.int32)
    d[1, 5] = -7          # behind lens[1] = 4
    r = np.ones((2, 6), np.float64)
    r[1, 4] = np.nan      # behind lens[1]
    for kw in (dict(durations=d), dict(token_rate=r), dict(token_rate=np.zeros((2, 6), np.float32))):
        with pytest.raises(SessionError) as ei:
            host_session.synthesize_batch(IDS, LENS, SC, **kw)
        assert "host-only" in str(ei.value), str(ei.value)


def test_stream_closure_owns_the_arrays_its_structs_point_into(host_session, monkeypatch):
    """synthesize_stream's C call runs on a worker thread after synthesize_stream has returned, and the vits_controls /
    vits_noise structs hold bare addresses: the closure handed to _stream must own the converted copies they point into
    ([3] scales -> rows, list seeds, int32 durations / float64 rates, float64 noise)."""
    import gc
    captured = []
    monkeypatch.setattr(host_session, "_stream", captured.append)
    for kw in (dict(durations=np.ones((2, 6), np.int32)), dict(token_rate=np.ones((2, 6), np.float64))):
        del captured[:]
        host_session.synthesize_stream(IDS, LENS, SC, seeds=[1, 2], noise_dp=np.zeros((2, 2, 6)),
                                       noise_z=np.zeros((2, host_session.hparam("inter"), 9)), **kw)
        gc.collect()
        junk = [np.full(n, 0x7F, np.uint8) for n in (36, 16, 48, 96) * 16]   # (what a freed block would be reused for)
        start, = captured
        cells = dict(zip(start.__code__.co_freevars, (c.cell_contents for c in start.__closure__)))
        ctl, noise = cells["ctl"], cells["noise"]
        rows, seeds, durations, token_rate = ctl._keep
        assert rows.dtype == np.float32 and rows.shape == (2, 3) and np.array_equal(rows, np.tile(SC, (2, 1)))
        assert seeds.dtype == np.uint64 and seeds.tolist() == [1, 2]
        assert ctl.scales_rows == rows.ctypes.data and ctl.seeds == seeds.ctypes.data
        if "durations" in kw:
            assert durations.dtype == np.int64 and np.array_equal(durations, np.ones((2, 6))) and token_rate is None
            assert ctl.durations == durations.ctypes.data and not ctl.token_rate
        else:
            assert token_rate.dtype == np.float32 and np.array_equal(token_rate, np.ones((2, 6))) and durations is None
            assert ctl.token_rate == token_rate.ctypes.data and not ctl.durations
        ndp, nz = noise._keep
        assert ndp.dtype == nz.dtype == np.float32 and not ndp.any() and not nz.any()
        assert noise.noise_dp == ndp.ctypes.data and noise.noise_z == nz.ctypes.data and noise.noise_z_stride == 9
        del junk


def test_grouping_warns_about_unmapped_phonemes_like_the_flat_function(caplog):
    import logging
    with caplog.at_level(logging.WARNING, logger="phoonnx_amd.phoneme_ids"):
        phonemes_to_ids(list("azb"), MAP)
        flat = [r.getMessage() for r in caplog.records]
        caplog.clear()
        phonemes_to_id_groups(list("azb"), MAP)
        assert [r.getMessage() for r in caplog.records] == flat == ["Missing phoneme from id map: z"]


def test_last_durations_without_a_run(host_session):
    with pytest.raises(SessionError) as ei:
        host_session.last_durations()
    assert "no completed run" in str(ei.value)
