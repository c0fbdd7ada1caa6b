"""SURVEY §8 f4 (ByT5 G2P): the NumPy restatement of the T5 graph (oracle/t5_oracle.py) against outputs of the Hugging Face
transformers model the fixture was exported from (oracle/gen_g2p_golden.py), and the text <-> id mirror against the outputs
of the reference's own `_encode_text` / `_decode_phones` (mul.py:135-170)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "byt5_tiny.npz"))


def test_relative_position_buckets_are_exact(G):
    from t5_oracle import relative_position_bucket
    assert np.array_equal(relative_position_bucket(G["bucket/rel"], True), G["bucket/enc"])
    assert np.array_equal(relative_position_bucket(G["bucket/rel"], False), G["bucket/dec"])


def test_t5_oracle_matches_transformers(G):
    from t5_oracle import T5Oracle
    o = T5Oracle(os.path.join(GOLDEN, "byt5_tiny.onnx"))
    hp = json.load(open(os.path.join(GOLDEN, "byt5_tiny.hparams.json")))
    assert (o.d_model, o.heads, o.d_kv, o.n_enc, o.n_dec, o.num_buckets) == (
        hp["d_model"], hp["num_heads"], hp["d_kv"], hp["num_layers"], hp["num_decoder_layers"],
        hp["relative_attention_num_buckets"])
    assert not o.tied
    for c in range(4):
        ids = G[f"c{c}/input_ids"][0]
        enc = o.encode(ids)
        np.testing.assert_allclose(enc, G[f"c{c}/encoder_out"][0], atol=2e-5, rtol=0)
        lg = o.logits(ids, G[f"c{c}/decoder_input_ids"][0])
        np.testing.assert_allclose(lg, G[f"c{c}/logits"], atol=2e-4, rtol=0)
        want = G[f"c{c}/greedy"].tolist()
        assert o.greedy(ids, max_length=len(want)) == want     # integer work: exact (mul.py:192-230)


T5_FAMILIES = {   # feed_forward_proj, tied -> what the C++ reader must report: (gated, act, scale_out)
    "gated-gelu": (dict(feed_forward_proj="gated-gelu", tied=False), (1, 0, 0)),
    "relu-tied": (dict(feed_forward_proj="relu", tied=True), (0, 1, 1)),
    "gelu-erf": (dict(feed_forward_proj="gelu", tied=False), (0, 2, 0)),
}


@pytest.mark.parametrize("family", sorted(T5_FAMILIES))
def test_written_t5_models_are_the_transformers_model_of_the_same_config(family, tmp_path):
    """phoonnx_amd.synth.write_t5 gives the GPU tests their full-width models, so it is pinned here, not trusted: a small
    model of each graph family the engine implements (gated tanh-GELU untied, ReLU tied, erf-GELU untied) is written, read by
    the oracle and by the C++ reader, and compared with the transformers model of the same T5Config holding the written
    weights.  Bounds: encoder output and logits in float32 as test_t5_oracle_matches_transformers holds the fixture to (2e-5 /
    2e-4: two float32 implementations of a graph with logits O(10), smaller than the fixture's); in float64 - oracle
    dtype=np.float64 against the model in double - 1e-9 absolute: there only the graph itself can differ."""
    transformers = pytest.importorskip("transformers")
    import torch
    from phoonnx_amd.g2p import MiG2PSession
    from phoonnx_amd.synth import write_t5
    from t5_oracle import T5Oracle
    opts, (gated, act, scale_out) = T5_FAMILIES[family]
    geo = dict(d_model=64, d_kv=16, num_heads=4, d_ff=128, num_layers=2, num_decoder_layers=2, vocab_size=384, **opts)
    path = str(tmp_path / "t5.onnx")
    hp = write_t5(path, seed=21, **geo)
    assert hp["d_model"] == 64 and hp["feed_forward_proj"] == opts["feed_forward_proj"]
    # the C++ reader's description of the graph
    s = MiG2PSession(path, host_only=True)
    got = {k: s.hparam(k) for k in ("vocab", "d_model", "heads", "d_kv", "d_ff", "n_enc", "n_dec", "num_buckets", "gated", "act",
                                    "scale_out")}
    s.close()
    assert got == dict(vocab=384, d_model=64, heads=4, d_kv=16, d_ff=128, n_enc=2, n_dec=2, num_buckets=32, gated=gated, act=act,
                       scale_out=scale_out), got
    o = T5Oracle(path)
    o64 = T5Oracle(path, dtype=np.float64)
    assert (o.d_model, o.heads, o.d_kv, o.n_enc, o.n_dec, o.num_buckets, o.tied) == (64, 4, 16, 2, 2, 32, opts["tied"])
    assert o.act == {"gated-gelu": "gelu_new", "relu": "relu", "gelu": "gelu"}[opts["feed_forward_proj"]]
    assert all(v.dtype == np.float64 for v in o64.w.values()) and all(v.dtype == np.float32 for v in o.w.values())
    # the transformers model of the same configuration, holding the written weights
    cfg = transformers.T5Config(vocab_size=384, d_model=64, d_kv=16, d_ff=128, num_layers=2, num_decoder_layers=2, num_heads=4,
                                relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0,
                                feed_forward_proj=opts["feed_forward_proj"], tie_word_embeddings=opts["tied"],
                                decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, layer_norm_epsilon=1e-6)
    def hf_model():
        mm = transformers.T5ForConditionalGeneration(cfg).eval()
        if not opts["tied"]:   # (transformers 5 shares lm_head with the embedding whatever the config says - the flag only
            # switches the output scale; a head of its own, as T5 v1.1 / ByT5 checkpoints have, is a Parameter of its own)
            mm.lm_head.weight = torch.nn.Parameter(torch.zeros_like(mm.shared.weight))
        return mm
    m = hf_model()
    sd = {}
    for k, v in o.w.items():
        parts = k.split(".")
        if k == "shared":
            sd["shared.weight"] = v
        elif k == "lm_head":
            sd["lm_head.weight"] = v.T
        elif parts[1] == "final_layer_norm":
            sd[k + ".weight"] = v
        else:
            name = f"{parts[0]}.block.{parts[1]}.layer.{parts[2]}." + ".".join(parts[3:]) + ".weight"
            sd[name] = v if v.ndim == 1 or parts[-1] == "relative_attention_bias" else v.T
    if opts["tied"]:
        assert np.array_equal(o.w["lm_head"], o.w["shared"].T)
    own = dict(m.state_dict())
    alias = {"encoder.embed_tokens.weight", "decoder.embed_tokens.weight"}     # (views of shared.weight)
    assert set(own) - alias == set(sd), set(own) ^ set(sd)                     # every parameter of the model was written
    for k, v in sd.items():
        assert tuple(own[k].shape) == v.shape, k
    full = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    full.update({k: full["shared.weight"] for k in alias})
    m.load_state_dict(full, strict=True)
    assert (m.lm_head.weight.data_ptr() == m.shared.weight.data_ptr()) == opts["tied"]
    assert all(torch.equal(v, full[k]) for k, v in m.state_dict().items())
    m64 = hf_model().double()
    # (T5LayerNorm casts to float32 for its variance whatever the model's dtype: in the double model that one step is
    # replaced by the same formula without the cast, or the comparison below would measure float32 rounding again)
    import types
    from transformers.models.t5.modeling_t5 import T5LayerNorm
    n_ln = 0
    for mod in m64.modules():
        if isinstance(mod, T5LayerNorm):
            mod.forward = types.MethodType(
                lambda self, x: self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)), mod)
            n_ln += 1
    assert n_ln == 2 * 2 + 3 * 2 + 2
    m64.load_state_dict({k: v.double() for k, v in full.items()}, strict=True)
    rng = np.random.default_rng(3)
    for S, T in ((1, 1), (9, 5), (150, 20)):      # (150: relative positions beyond max_distance)
        ids = rng.integers(3, 259, S).astype(np.int64)
        dec = np.concatenate(([0], rng.integers(3, 259, T - 1))).astype(np.int64)
        with torch.no_grad():
            tid, td = torch.from_numpy(ids)[None], torch.from_numpy(dec)[None]
            mask = torch.ones_like(tid)
            enc_t = m.encoder(input_ids=tid, attention_mask=mask).last_hidden_state[0].numpy()
            lg_t = m(input_ids=tid, attention_mask=mask, decoder_input_ids=td).logits.numpy()
            enc_t64 = m64.encoder(input_ids=tid, attention_mask=mask).last_hidden_state[0].numpy()
            lg_t64 = m64(input_ids=tid, attention_mask=mask, decoder_input_ids=td).logits.numpy()
        assert float(np.abs(lg_t).max()) > 1
        np.testing.assert_allclose(o.encode(ids), enc_t, atol=2e-5, rtol=0)
        np.testing.assert_allclose(o.logits(ids, dec), lg_t, atol=2e-4, rtol=0)
        lg64 = o64.logits(ids, dec)
        assert lg64.dtype == np.float64
        np.testing.assert_allclose(o64.encode(ids), enc_t64, atol=1e-9, rtol=0)
        np.testing.assert_allclose(lg64, lg_t64, atol=1e-9, rtol=0)
    ids = rng.integers(3, 259, 30).astype(np.int64)
    with torch.no_grad():
        gen = [0]
        for _ in range(16):                       # the greedy loop of mul.py:192-230 on the transformers model
            lg = m(input_ids=torch.from_numpy(ids)[None], decoder_input_ids=torch.tensor([gen])).logits
            gen.append(int(lg[0, -1].argmax()))
    assert o.greedy(ids, max_length=16, eos=-1) == gen[1:]


def test_text_mirror_matches_reference_functions():
    from phoonnx_amd.g2p import decode_phones, encode_text
    F = json.load(open(os.path.join(GOLDEN, "byt5_frontend.json"), encoding="utf-8"))
    for c in F["encode"]:
        got = encode_text(c["text"], c["lang"])
        assert got.dtype == np.int64 and got.shape == (1, len(c["ids"])) and got[0].tolist() == c["ids"]
    tokens = F["tokenizer_config"]["added_tokens_decoder"]
    for c in F["decode"]:
        assert decode_phones(c["ids"], tokens) == c["text"]


def test_g2p_abi_surface_and_model_description(G):
    """CPU side of the product: g2pmi.h symbols exported, the C++ reader derives the T5 geometry from the .onnx, and its
    relative-position buckets (integers) equal the transformers function's over the whole supported range."""
    import re
    from conftest import ROOT
    from phoonnx_amd import _ffi
    from phoonnx_amd.g2p import MiG2PSession
    from phoonnx_amd.session import SessionError
    hdr = open(os.path.join(ROOT, "include", "g2pmi.h")).read()
    declared = set(re.findall(r"\b(g2p_[a-z0-9_]+)\s*\(", hdr))
    lib = _ffi.load()
    assert declared == set(_ffi.G2P_EXPORTS), declared ^ set(_ffi.G2P_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    s = MiG2PSession(os.path.join(GOLDEN, "byt5_tiny.onnx"), host_only=True)
    hp = json.load(open(os.path.join(GOLDEN, "byt5_tiny.hparams.json")))
    assert s.hparam("vocab") == hp["vocab_size"] and s.hparam("d_model") == hp["d_model"]
    assert s.hparam("heads") == hp["num_heads"] and s.hparam("d_kv") == hp["d_kv"] and s.hparam("d_ff") == hp["d_ff"]
    assert s.hparam("n_enc") == hp["num_layers"] and s.hparam("n_dec") == hp["num_decoder_layers"]
    assert s.hparam("num_buckets") == hp["relative_attention_num_buckets"]
    assert s.hparam("gated") == 1 and s.hparam("act") == 0 and s.hparam("scale_out") == 0    # gated-gelu (tanh form), untied
    assert [o.name for o in s.get_outputs()] == ["logits"]
    rel = G["bucket/rel"]
    assert [s.bucket(int(r)) for r in rel] == G["bucket/enc"].tolist()
    assert [s.bucket(int(r), decoder=True) for r in rel] == G["bucket/dec"].tolist()
    with pytest.raises(SessionError):   # host-only handles cannot run
        s.run(None, {"input_ids": np.array([[5, 6]], np.int64), "decoder_input_ids": np.array([[0]], np.int64)})
    s.close()
    with pytest.raises(SessionError):   # a VITS graph is not a T5 graph
        MiG2PSession(os.path.join(GOLDEN, "tiny_dp.onnx"), host_only=True)


def test_language_tags_resolve_like_the_reference_match_lang():
    """TTSVoice hands BCP-47 tags (config.lang_code) to the phonemizer; the reference resolves them to the
    phonemizer's own list through langcodes (phonemizers/base.py:86-122).  Expected values = langcodes' answers for the
    reference's lists (mul.py:31-33, 248-256)."""
    from phoonnx_amd.g2p import ByT5Phonemizer as B, CharsiuPhonemizer as Ch
    byt5 = {"en-US": "en-US", "en": "en-US", "en-GB": "en-GB", "en-AU": "en-GB", "pt": "pt-BR", "pt-PT": "pt-PT",
            "de": "de-DE", "de-AT": "de-DE", "zh": "zh-CN", "no": "nb-NO", "yue": "yue-CN", "fr-CA": "fr-FR"}
    charsiu = {"en-US": "eng-us", "en": "eng-us", "en-GB": "eng-uk", "pt-BR": "por-bz", "pt": "por-bz", "pt-PT": "por-po",
               "de": "ger", "de-DE": "ger", "nl-NL": "dut", "cs": "cze", "el-GR": "gre", "zh-TW": "zho-t", "zh-CN": "zho-s",
               "es-MX": "spa-me", "es-AR": "spa-latin", "es": "spa", "fr-CA": "fra-qu", "fr": "fra", "eng-us": "eng-us",
               "fa-IR": "fas", "is": "ice", "cy": "wel-nw", "vi": "vie-n"}
    for t, want in byt5.items():
        assert B.get_lang(t) == want, (t, B.get_lang(t), want)
    for t, want in charsiu.items():
        assert Ch.get_lang(t) == want, (t, Ch.get_lang(t), want)
    for bad in ("xx-YY", "tlh", ""):
        for cls in (B, Ch):
            with pytest.raises(ValueError):
                cls.get_lang(bad)
