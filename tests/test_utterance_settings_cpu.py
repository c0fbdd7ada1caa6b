"""Per-utterance synthesis settings and noise seeds, the parts that need no GPU: TTSVoice.synthesize_requests on a recording
stub session (rows, settings, derived seeds, sorting, the max_batch cut, regrouping, fallback, speaker check), the
validation of [B, 3] scales and seeds before any engine call, and ShardedSynthesizer over two gloo ranks."""
import os
import socket
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from phoonnx_amd.config import PhonemeType, SynthesisConfig, VoiceConfig
from phoonnx_amd.voice import TTSVoice, sentence_seed, splitmix64

M64 = (1 << 64) - 1


class _Phon:
    def add_diacritics(self, text, lang):
        return text

    def phonemize(self, text, lang):
        return [list(s.strip()) for s in text.split(".") if s.strip()]


class _BatchStub:
    """A batch session that records every call; frame count = id count, waveform of row b = a ramp scaled by its length
    scale plus 100 * its speaker (distinct per row, so regrouping is visible)."""
    HOP = 3

    def __init__(self, names=("input", "input_lengths", "scales", "sid"), n_speakers=4):
        self.names, self.n_speakers, self.calls = list(names), n_speakers, []

    def get_inputs(self):
        return [types.SimpleNamespace(name=n) for n in self.names]

    def hparam(self, key):
        return {"hop": self.HOP, "n_speakers": self.n_speakers}[key]

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None):
        self.calls.append(dict(ids=ids.copy(), lens=lens.copy(), scales=np.array(scales), sid=None if sid is None else sid.copy(),
                               seeds=None if seeds is None else np.array(seeds)))
        B = ids.shape[0]
        S = int(lens.max()) * self.HOP + 5
        out = np.full((B, 1, 1, S), 9.0, np.float32)   # (9.0 behind each row's end: must be trimmed away)
        for b in range(B):
            n = int(lens[b]) * self.HOP
            out[b, 0, 0, :n] = self.row_audio(ids[b, :lens[b]], scales[b], 0 if sid is None else sid[b])
        return {"output": out, "y_lengths": lens.astype(np.int64)}

    def row_audio(self, ids, sc, spk):
        n = len(ids) * self.HOP
        return (np.arange(n, dtype=np.float32) / 1000.0 + float(ids[0]) / 100.0) * float(sc[1]) + 0.1 * float(spk)


def _voice(session, n_speakers=4):
    cfg = VoiceConfig(num_symbols=64, num_speakers=n_speakers, num_langs=1, sample_rate=16000, lang_code="en",
                      phoneme_id_map={c: [i + 1] for i, c in enumerate("abcdefghijklmnopqrstuvwxyz ")},
                      phoneme_type=PhonemeType.RAW, alphabet=None, phonemizer_model=None)
    return TTSVoice(session=session, config=cfg, phonemizer=_Phon(), dedupe_sentences=True)


def test_splitmix64_and_sentence_seeds():
    # splitmix64 generator started at 1234567: its first outputs (the published reference sequence)
    assert splitmix64((1234567 + 0x9E3779B97F4A7C15) & M64) == 6457827717110365317
    assert splitmix64((1234567 + 2 * 0x9E3779B97F4A7C15) & M64) == 3203168211198807973
    assert sentence_seed(1234567, 0) == 6457827717110365317 and sentence_seed(1234567, 1) == 3203168211198807973
    assert sentence_seed(-1, 0) == sentence_seed(M64, 0)      # (taken mod 2^64)


def test_requests_rows_settings_seeds_sorting_and_regrouping():
    st = _BatchStub()
    v = _voice(st)
    reqs = [("abcdef. ab.", SynthesisConfig(speaker_id=2, length_scale=1.5, noise_scale=0.5, noise_w_scale=0.6)),
            ("", None),                                                    # empty request: no rows, no chunks
            ("abc. abcdefgh. a.", SynthesisConfig(speaker_id=1, volume=0.5, normalize_audio=False)),
            ("abcd.", None)]
    seeds = [11, 22, 33, (1 << 64) - 5]
    res = v.synthesize_requests(reqs, seeds=seeds, max_batch=4)
    # rows sorted by id count, runs of at most 4
    assert [c["ids"].shape[0] for c in st.calls] == [4, 2]
    lens = np.concatenate([c["lens"] for c in st.calls])
    assert np.all(np.diff(lens) >= 0)
    # every row carries its request's settings, speaker and derived seed
    want = {}
    for r, (text, cfg) in enumerate(reqs):
        cfg = cfg or SynthesisConfig()
        for k, ids in enumerate(v._sentence_ids(text, cfg)):
            want[tuple(ids)] = (v._scales(cfg), cfg.speaker_id or 0, sentence_seed(seeds[r], k))
    seen = 0
    for c in st.calls:
        assert c["scales"].shape == (c["ids"].shape[0], 3) and c["scales"].dtype == np.float32
        assert c["seeds"].dtype == np.uint64 and c["sid"].dtype == np.int64
        for b in range(c["ids"].shape[0]):
            sc, spk, sd = want[tuple(c["ids"][b, :c["lens"][b]].tolist())]
            assert np.array_equal(c["scales"][b], sc) and int(c["sid"][b]) == spk and int(c["seeds"][b]) == sd
            seen += 1
    assert seen == len(want) == 6
    # regrouped in request and sentence order, trimmed to y_len * hop and post-processed per request
    assert [len(x) for x in res] == [2, 0, 3, 1]
    for r, (text, cfg) in enumerate(reqs):
        cfg = cfg or SynthesisConfig()
        for k, ids in enumerate(v._sentence_ids(text, cfg)):
            raw = st.row_audio(np.asarray(ids), v._scales(cfg), cfg.speaker_id or 0)
            ch = res[r][k]
            assert ch.sample_rate == 16000 and ch.sample_width == 2 and ch.sample_channels == 1
            assert np.array_equal(ch.audio_float_array, v._postprocess(raw, cfg))
    # without seeds: no seeds argument reaches the session; max_batch larger than the rows: one run
    st.calls.clear()
    res2 = v.synthesize_requests(reqs, max_batch=32)
    assert len(st.calls) == 1 and st.calls[0]["seeds"] is None and st.calls[0]["ids"].shape[0] == 6
    for a, b in zip(res, res2):
        assert [np.array_equal(x.audio_float_array, y.audio_float_array) for x, y in zip(a, b)] == [True] * len(a)
    assert v.synthesize_requests([]) == [] and v.synthesize_requests([("", None)]) == [[]]
    with pytest.raises(ValueError):
        v.synthesize_requests(reqs, max_batch=0)
    with pytest.raises(ValueError):
        v.synthesize_requests(reqs, seeds=[1, 2])


def test_requests_speaker_check_and_graph_without_sid():
    st = _BatchStub()
    v = _voice(st)
    with pytest.raises(ValueError, match="request 1"):
        v.synthesize_requests([("ab.", None), ("ab.", SynthesisConfig(speaker_id=4))])
    with pytest.raises(ValueError, match="request 0"):
        v.synthesize_requests([("ab.", SynthesisConfig(speaker_id=-1))])
    assert st.calls == []                                                   # nothing ran
    # a graph without "sid": no speaker rows (and no check)
    st2 = _BatchStub(names=("input", "input_lengths", "scales"))
    _voice(st2).synthesize_requests([("ab.", SynthesisConfig(speaker_id=7))])
    assert st2.calls[0]["sid"] is None


def test_requests_fall_back_to_synthesize_without_synthesize_batch():
    class _Ort:  # the onnxruntime duck type: get_inputs() + run()
        def __init__(self):
            self.feeds = []

        def get_inputs(self):
            return [types.SimpleNamespace(name=n) for n in ("input", "input_lengths", "scales", "sid")]

        def run(self, _none, feed):
            self.feeds.append(feed)
            return [np.full((1, 1, 1, 4 * feed["input"].shape[1]), 0.25, np.float32)]

    ort = _Ort()
    v = _voice(ort, n_speakers=3)
    reqs = [("ab. abc.", SynthesisConfig(speaker_id=1, length_scale=0.8, normalize_audio=False)), ("abcd.", None)]
    got = v.synthesize_requests(reqs, seeds=[1, 2])
    want = [list(v.synthesize(t, c)) for t, c in reqs]
    assert [len(x) for x in got] == [2, 1]
    for a, b in zip(got, want):
        assert all(np.array_equal(x.audio_float_array, y.audio_float_array) for x, y in zip(a, b))
    assert [f["sid"].tolist() for f in ort.feeds[:3]] == [[1], [1], [0]]
    assert np.allclose(ort.feeds[0]["scales"], v._scales(reqs[0][1]))
    with pytest.raises(ValueError, match="request 0"):   # (speaker bound from the voice config without hparam)
        v.synthesize_requests([("ab.", SynthesisConfig(speaker_id=3))])


class _Recording:
    """Forwards to the real library and records every run entry point called through it."""

    def __init__(self, lib):
        self._lib, self.runs = lib, []

    def __getattr__(self, name):
        if name.startswith("vits_run"):
            self.runs.append(name)
        return getattr(self._lib, name)


def test_rows_validation_before_any_engine_call():
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession, SessionError
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    rec = _Recording(s._lib)
    s._lib = rec
    ids, lens = np.ones((2, 5), np.int64), np.array([5, 3], np.int64)
    good = np.array([[0.5, 1.0, 0.8], [0.6, 1.1, 0.7]], np.float32)
    bad = [dict(scales=np.ones((3, 3), np.float32)),                     # rows != B
           dict(scales=np.ones((2, 3), np.float64)),                     # dtype
           dict(scales=np.ones((2, 4), np.float32)),                     # shape
           dict(scales=np.array([[0.5, 1.0, 0.8], [0.6, np.inf, 0.7]], np.float32)),   # non-finite
           dict(scales=np.array([[0.5, 1.0, 0.8], [np.nan, 1.0, 0.7]], np.float32)),
           dict(scales=good, seeds=[1]),                                 # seeds: shape
           dict(scales=good, seeds=[1.5, 2.0]),                          # dtype
           dict(scales=good, seeds=[1, -2]),                             # range
           dict(scales=good, seeds=[1, 1 << 64])]
    for kw in bad:
        with pytest.raises(SessionError) as ei:
            s.synthesize_batch(ids, lens, kw["scales"], None, seeds=kw.get("seeds"))
        if not np.isfinite(kw["scales"]).all():
            assert "row 1" in str(ei.value)
        if kw["scales"].dtype != np.float32:
            continue   # (synthesize_stream and run_device convert scales to float32, as they always have)
        with pytest.raises(SessionError):
            list(s.synthesize_stream(ids, lens, kw["scales"], None, seeds=kw.get("seeds")))
        with pytest.raises(SessionError):
            s.run_device(0, 0, 2, 5, kw["scales"], seeds=kw.get("seeds"))
    p = PipelinedSession.__new__(PipelinedSession)   # (validation happens before any part is touched)
    for kw in bad:
        with pytest.raises(SessionError):
            p.synthesize_batch(ids, lens, kw["scales"], None, seeds=kw.get("seeds"))
    assert rec.runs == []
    # valid rows reach the row twin (which refuses a host-only handle), [3] without seeds the base entry point
    with pytest.raises(SessionError):
        s.synthesize_batch(ids, lens, good, None, seeds=np.array([3, 4], np.uint64))
    with pytest.raises(SessionError):
        s.synthesize_batch(ids, lens, good[0], None)
    assert rec.runs == ["vits_run_async_rows", "vits_run_async"]
    s._lib = rec._lib
    s.close()


class _StubSession:
    """ShardedSynthesizer's session contract; records what reached it.  Waveform = a ramp scaled by the row's length scale
    plus its seed's low bits, so the gathered result shows whose settings each utterance was rendered with."""
    HOP = 4

    def __init__(self):
        self.calls = []

    def hparam(self, key):
        assert key == "hop"
        return self.HOP

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None):
        self.calls.append((np.array(scales).tolist(), None if seeds is None else [int(x) for x in seeds]))
        B = ids.shape[0]
        sc = np.broadcast_to(np.asarray(scales, np.float32), (B, 3))
        out = np.zeros((B, 1, 1, int(lens.max()) * self.HOP), np.float32)
        for b in range(B):
            n = int(lens[b]) * self.HOP
            out[b, 0, 0, :n] = np.arange(n) * sc[b, 1] + (0 if seeds is None else int(seeds[b]) % 1000)
        return {"output": out, "y_lengths": lens.astype(np.int64)}

    def close(self):
        pass


class _OldStub(_StubSession):
    """A session with the four-argument synthesize_batch of earlier releases."""

    def synthesize_batch(self, ids, lens, scales, sid):
        return super().synthesize_batch(ids, lens, scales, sid)


def _utts(n=13, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 50, size=int(k)).tolist() for k in rng.integers(1, 30, size=n)]


def _settings_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from phoonnx_amd.sharding import ShardedSynthesizer, partition
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        utts = _utts()
        n = len(utts)
        scales = np.stack([np.array([0.5, 1.0 + 0.1 * i, 0.8], np.float32) for i in range(n)])
        seeds = [1000 * i + 7 for i in range(n)]
        st = _StubSession()
        sh = ShardedSynthesizer("unused.onnx", 0, dist, session=st)
        got = sh.synthesize(utts, scales, None, gather=True, seeds=seeds)
        mine = partition([len(u) for u in utts], world)[0][rank]
        want_rows = (scales[mine].tolist(), [seeds[i] for i in mine])
        local = sh.synthesize(utts, scales, None, gather=False)          # rows, no seeds
        old = ShardedSynthesizer("unused.onnx", 0, dist, session=_OldStub())
        legacy = old.synthesize(utts, np.array([0.5, 1.0, 0.8], np.float32), None, gather=True)
        q.put((rank, st.calls, want_rows, [w.tolist() for w in got], [(i, w.tolist()) for i, w in local],
               [w.tolist() for w in legacy]))
    finally:
        dist.destroy_process_group()


def test_sharded_rows_follow_their_utterances_two_ranks_gloo():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_settings_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=180) for _ in procs], key=lambda g: g[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    utts = _utts()
    n = len(utts)
    scales = np.stack([np.array([0.5, 1.0 + 0.1 * i, 0.8], np.float32) for i in range(n)])
    seeds = [1000 * i + 7 for i in range(n)]
    for rank, calls, want_rows, gathered, local, legacy in got:
        assert calls[0] == want_rows                                      # exactly its utterances' rows and seeds
        assert calls[1][1] is None and calls[1][0] == want_rows[0]
        for i in range(n):                                                # gathered in the original order
            m = len(utts[i]) * _StubSession.HOP
            w = np.arange(m) * scales[i, 1] + seeds[i] % 1000
            assert np.allclose(gathered[i], w, atol=1e-4), (rank, i)
            assert np.allclose(legacy[i], np.arange(m) * np.float32(1.0))
        for i, w in local:
            assert np.allclose(w, np.arange(len(utts[i]) * 4) * scales[i, 1], atol=1e-4)
    # one process, no group: the same argument checks
    from phoonnx_amd.sharding import ShardedSynthesizer
    solo = ShardedSynthesizer("unused.onnx", 0, None, session=_StubSession())
    with pytest.raises(ValueError):
        solo.synthesize(utts, scales[:3])
    with pytest.raises(ValueError):
        solo.synthesize(utts, scales, seeds=[1, 2])
    r = solo.synthesize(utts, scales, seeds=seeds)
    assert sorted(i for i, _ in r) == list(range(n))


def _bad_seed_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from phoonnx_amd.sharding import ShardedSynthesizer, partition
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        utts = _utts()
        n = len(utts)
        scales = np.tile(np.array([0.5, 1.0, 0.8], np.float32), (n, 1))
        owner = int(partition([len(u) for u in utts], world)[0][1][0])   # an utterance rank 1 renders
        errors = []
        sh = ShardedSynthesizer("unused.onnx", 0, dist, session=_StubSession())
        for bad in (-1, 1 << 64, 2.5):
            seeds = list(range(n))
            seeds[owner] = bad
            try:
                sh.synthesize(utts, scales, None, gather=True, seeds=seeds)
                errors.append(None)
            except ValueError as e:
                errors.append(str(e))
        # the group is still usable: nobody was left inside a collective
        after = sh.synthesize(utts, scales, None, gather=True, seeds=list(range(n)))
        q.put((rank, owner, errors, len(after)))
    finally:
        dist.destroy_process_group()


def test_sharded_bad_seed_fails_on_every_rank_gloo():
    """A seed outside [0, 2^64) of an utterance one rank renders: every rank raises (the whole request is checked before it
    is dealt), none is left waiting in the gather."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_bad_seed_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=180) for _ in procs], key=lambda g: g[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = len(_utts())
    for rank, owner, errors, n_after in got:
        assert len(errors) == 3 and all(e is not None and f"seeds[{owner}]" in e for e in errors), (rank, errors)
        assert n_after == n


def test_run_keeps_the_graphs_scales_shape_and_run_device_rows_are_checked():
    """session.run() is the onnxruntime stand-in: scales stay [3], as get_inputs() declares them; the device-pointer entry
    points (MiSession / PipelinedSession.run_device, run_device_steps) check [B, 3] rows and seeds before any engine call."""
    from phoonnx_amd import MiSession
    from phoonnx_amd.session import PipelinedSession, SessionError
    s = MiSession(os.path.join(GOLDEN, "tiny_rb1.onnx"), host_only=True)
    rec = _Recording(s._lib)
    s._lib = rec
    ids, lens = np.ones((2, 5), np.int64), np.array([5, 3], np.int64)
    assert [i.shape for i in s.get_inputs() if i.name == "scales"] == [[3]]
    feed = {"input": ids, "input_lengths": lens, "scales": np.tile(np.array([0.667, 1.0, 0.8], np.float32), (2, 1))}
    feed = {k: v for k, v in feed.items() if k in s._input_names}
    with pytest.raises(SessionError, match=r"shape \[3\]"):
        s.run(None, feed)
    bad = [dict(scales=np.array([[0.5, 1.0, 0.8], [0.5, np.inf, 0.8]], np.float32)),
           dict(scales=np.ones((3, 3), np.float32)), dict(scales=np.ones((2, 3), np.float32), seeds=[1, -1])]
    p = PipelinedSession.__new__(PipelinedSession)   # (checked before any part is touched)
    p.parts = []
    for kw in bad:
        with pytest.raises(SessionError):
            s.run_device(0, 0, 2, 5, kw["scales"], seeds=kw.get("seeds"))
        with pytest.raises(SessionError):
            p.run_device(0, 0, 2, 5, kw["scales"], seeds=kw.get("seeds"))
        with pytest.raises(SessionError):
            p.run_device_steps(0, 0, 2, 5, kw["scales"], 1, seeds=kw.get("seeds"))
    assert rec.runs == []
    s._lib = rec._lib
    s.close()


def test_pipelined_run_device_gives_each_part_its_rows():
    from phoonnx_amd.session import PipelinedSession

    class _Part:
        def __init__(self):
            self.calls = []

        def run_device(self, ids_ptr, lens_ptr, B, T, scales, sid_ptr=None, seeds=None):
            self.calls.append((ids_ptr, B, np.array(scales).tolist(), None if seeds is None else [int(x) for x in seeds]))
            return {}

        def last_y_lengths(self):
            return np.ones(self.calls[-1][1], np.int64)

        def sync(self):
            pass

    p = PipelinedSession.__new__(PipelinedSession)
    p.parts = [_Part(), _Part()]
    rows = np.arange(15, dtype=np.float32).reshape(5, 3)
    seeds = np.arange(10, 15, dtype=np.uint64)
    p.run_device(1000, 2000, 5, 4, rows, seeds=seeds)
    assert [c[1:] for c in p.parts[0].calls] == [(2, rows[:2].tolist(), [10, 11])]
    assert [c[1:] for c in p.parts[1].calls] == [(3, rows[2:].tolist(), [12, 13, 14])]
    assert p.parts[1].calls[0][0] == 1000 + 2 * 4 * 8
    for part in p.parts:
        part.calls.clear()
    p.run_device_steps(1000, 2000, 5, 4, rows, 2, seeds=seeds)
    assert [c[1:] for c in p.parts[1].calls] == [(3, rows[2:].tolist(), [12, 13, 14])] * 2
    for part in p.parts:
        part.calls.clear()
    p.run_device_steps(1000, 2000, 5, 4, rows, 2, alternate=True, seeds=seeds)
    assert [c[1:] for c in p.parts[0].calls] == [(5, rows.tolist(), list(range(10, 15)))]
    # a [3] vector without seeds: every part gets it as it is, and no seeds
    for part in p.parts:
        part.calls.clear()
    p.run_device(1000, 2000, 5, 4, np.array([0.5, 1.0, 0.8], np.float32))
    assert [c[2:] for c in p.parts[0].calls] == [(np.array([0.5, 1.0, 0.8], np.float32).tolist(), None)]
