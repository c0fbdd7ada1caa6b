"""TTSVoice — the user-facing object of phoonnx with the MI355X engine behind it.

Counterpart of `phoonnx/voice.py:61-379`: `TTSVoice.load()`, `synthesize()`,
`synthesize_wav()`, `phoneme_ids_to_audio()`, `AudioChunk` keep the reference's names,
arguments and observable behaviour; the one difference is the object stored in
`self.session`: a `MiSession` (C ABI -> HIP kernels) instead of an onnxruntime session.
Behaviour around the hot call is pinned to the reference's own outputs
(tests/golden/frontend.json): feed construction, post-processing, int16 conversion, WAV
framing — including the reference's sentence-list duplication (voice.py:203-206), which is
reproduced by default and can be switched off with `dedupe_sentences=True`.

Extensions: `synthesize(..., batch_sentences=True)` renders all
sentences of a text in ONE batched engine call; `synthesize_requests()` renders the sentences
of many requests, each with its own SynthesisConfig (and optionally its own noise seed), in
shared batches; `synthesize(..., alignments=True)` / `synthesize_requests(..., alignments=True)` attach per-phoneme
timing (`AudioChunk.phoneme_alignments`) from the durations the engine reports (MiSession.last_durations);
`synthesize_encoded()` / `synthesize_requests_encoded()` return a text's or a request's audio as one encoded stream (16-bit
PCM, G.711 mu-law / A-law, float32) with a pause in front of every sentence - post-processed, encoded and packed on the
device by sessions that deliver (MiSession.synthesize_delivered), by audio_encoding on the host otherwise.
"""
import dataclasses
import json
import logging
import re
import wave
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .config import PhonemeType, SynthesisConfig, VoiceConfig
from .phoneme_ids import BlankBetween, phonemes_to_id_groups, phonemes_to_ids
from .phonemizers import get_phonemizer

LOG = logging.getLogger(__name__)

_PHONEME_BLOCK = re.compile(r"(\[\[.*?\]\])")
_MAX_WAV_VALUE = 32767.0
_GAIN_RAMP = 0.01   # seconds a change of per-phoneme volume takes (synthesize_encoded, phoneme_gain_db)
_MASK64 = (1 << 64) - 1
_GOLDEN64 = 0x9E3779B97F4A7C15


def splitmix64(x: int) -> int:
    """The splitmix64 output function of a 64-bit state (the generator's state after its increment)."""
    z = x & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def sentence_seed(request_seed: int, k: int) -> int:
    """Noise seed of sentence k (0-based) of a request seeded with `request_seed`: output k + 1 of a splitmix64
    generator started at request_seed, i.e. splitmix64(request_seed + (k + 1) * 0x9E3779B97F4A7C15 mod 2^64)."""
    return splitmix64((int(request_seed) + (k + 1) * _GOLDEN64) & _MASK64)


def config_from_metadata(meta: dict) -> dict:
    """Voice-config dict from the `.onnx` metadata_props (keys of export_onnx.py:335-345).
    Raises ValueError when the file carries no usable metadata."""
    if not meta or "phoneme_id_map" not in meta:
        raise ValueError("no voice config JSON and the .onnx has no phoonnx metadata_props to rebuild it from")
    try:
        id_map = json.loads(meta["phoneme_id_map"])
    except json.JSONDecodeError as exc:
        raise ValueError("metadata_props['phoneme_id_map'] is not valid JSON") from exc
    return {
        "phoneme_type": meta.get("phoneme_type") or "raw",
        "alphabet": meta.get("alphabet") or None,
        "phonemizer_model": meta.get("phonemizer_model") or None,
        "lang_code": meta.get("lang_code") or "und",
        "audio": {"sample_rate": int(meta.get("sample_rate", 22050))},
        "num_symbols": int(meta.get("n_vocab", 256)),
        "num_speakers": int(meta.get("n_speakers", 1)),
        "phoneme_id_map": id_map,
    }


def check_consistency(config_dict: dict, meta: dict, graph_speakers: int, graph_vocab: int) -> None:
    """Extension: the three places that describe a voice must agree - the voice JSON, the
    metadata_props export_onnx.py:335-350 wrote into the .onnx, and the graph itself (embedding table sizes).  The
    reference never compares them (config.py:335-358 just reads the JSON) and a mismatch surfaces later as wrong-rate
    audio or an out-of-range Gather inside onnxruntime.  Only values a side actually STATES are compared; raises
    ValueError naming both sides."""
    def as_int(v):
        try:
            return int(v)
        except (TypeError, ValueError):
            return None

    problems = []
    pairs = (("num_speakers", config_dict.get("num_speakers"), "n_speakers"),
             ("audio.sample_rate", (config_dict.get("audio") or {}).get("sample_rate"), "sample_rate"),
             ("num_symbols", config_dict.get("num_symbols"), "n_vocab"))
    for cfg_key, cfg_val, meta_key in pairs:
        c, m = as_int(cfg_val), as_int((meta or {}).get(meta_key))
        if c is not None and m is not None and c != m:
            problems.append(f"config {cfg_key}={c} but the .onnx metadata says {meta_key}={m}")
    c = as_int(config_dict.get("num_speakers"))
    if c is not None and c != graph_speakers and not (c <= 1 and graph_speakers <= 1):
        problems.append(f"config num_speakers={c} but the graph's speaker table has {graph_speakers} rows")
    m = as_int((meta or {}).get("n_speakers"))
    if m is not None and m != graph_speakers and not (m <= 1 and graph_speakers <= 1):
        problems.append(f".onnx metadata n_speakers={m} but the graph's speaker table has {graph_speakers} rows")
    id_map = config_dict.get("phoneme_id_map") or {}
    top = -1
    for v in id_map.values():
        for i in (v if isinstance(v, (list, tuple)) else [v]):
            top = max(top, as_int(i) if as_int(i) is not None else -1)
    if top >= graph_vocab:
        problems.append(f"phoneme_id_map uses id {top} but the graph's embedding table has {graph_vocab} rows")
    if problems:
        raise ValueError("inconsistent voice: " + "; ".join(problems))


@dataclass
class PhonemeAlignment:
    """Where one phoneme (with the ids it produced, inserted blanks included) sits in its chunk's audio:
    samples [start_sample, start_sample + num_samples)."""
    phoneme: str
    phoneme_ids: List[int]
    start_sample: int
    num_samples: int


def build_alignments(groups: Sequence[Tuple[str, Sequence[int]]], durations: Sequence[int], hop: int,
                     total_frames: Optional[int] = None, ratio: Optional[Tuple[int, int]] = None) -> List[PhonemeAlignment]:
    """(token, [ids]) groups (phonemes_to_id_groups) + the frames each id occupies (`durations`, one per id in group order;
    longer, e.g. a padded batch row, is fine) + the samples per frame -> one PhonemeAlignment per group: cumulative
    starts, num_samples = the group's frames * hop, so that they sum to sum(durations) * hop; a token of zero frames gets
    0 samples.  total_frames: the utterance's frame count where it is known - the engine renders max(1, sum) frames, so
    an utterance whose durations are all 0 still has one frame of audio, which then goes to the last entry.
    ratio: (L, M) of an output rate (out / in, reduced; MiSession.set_output_rate) - the chunk's audio then has
    N = ceil(samples * L / M) samples and a boundary at input sample e lies at output sample min(N, ceil(e * L / M)), so
    that num_samples still sum to the chunk's length and a token of zero frames still gets 0 samples."""
    out: List[PhonemeAlignment] = []
    pos = frames = 0
    for token, ids in groups:
        n = int(sum(int(d) for d in durations[pos:pos + len(ids)]))
        out.append(PhonemeAlignment(phoneme=token, phoneme_ids=[int(i) for i in ids], start_sample=frames * hop,
                                    num_samples=n * hop))
        pos += len(ids)
        frames += n
    if out and total_frames is not None and total_frames > frames:
        out[-1].num_samples += (int(total_frames) - frames) * hop
    if ratio is not None:
        L, M = (int(v) for v in ratio)
        n_total = -(-sum(a.num_samples for a in out) * L // M)
        for a in out:
            lo, hi = (min(n_total, -(-e * L // M)) for e in (a.start_sample, a.start_sample + a.num_samples))
            a.start_sample, a.num_samples = lo, hi - lo
    return out


def build_span_alignments(groups: Sequence[Tuple[str, Sequence[int]]], spans: Sequence[int], total: int) -> List[PhonemeAlignment]:
    """build_alignments for a sentence whose phonemes were raised or lowered (phoneme_pitch): its audio went through the time
    warp, so a phoneme's samples are the warp's own token spans (MiSession.last_token_spans: output samples per id, in group
    order; a padded row is fine), not durations * hop.  total: the sentence's valid samples - what the spans sum to; where
    they do not (every token dropped: the one frame the engine still renders) the rest goes to the last entry."""
    out: List[PhonemeAlignment] = []
    pos = at = 0
    for token, ids in groups:
        n = int(sum(int(k) for k in spans[pos:pos + len(ids)]))
        out.append(PhonemeAlignment(phoneme=token, phoneme_ids=[int(i) for i in ids], start_sample=at, num_samples=n))
        pos += len(ids)
        at += n
    if out and int(total) > at:
        out[-1].num_samples += int(total) - at
    return out


@dataclass
class AudioChunk:
    """A chunk of raw audio: float samples in [-1, 1] plus their PCM16 rendering."""
    sample_rate: int
    sample_width: int
    sample_channels: int
    audio_float_array: np.ndarray
    _audio_int16_array: Optional[np.ndarray] = None
    _audio_int16_bytes: Optional[bytes] = None
    _MAX_WAV_VALUE: float = _MAX_WAV_VALUE
    # synthesize(..., alignments=True): per-phoneme timing of this chunk; num_samples sum to len(audio_float_array)
    phoneme_alignments: Optional[List[PhonemeAlignment]] = None

    @property
    def audio_int16_array(self) -> np.ndarray:
        if self._audio_int16_array is None:
            scaled = self.audio_float_array * self._MAX_WAV_VALUE
            self._audio_int16_array = np.clip(scaled, -self._MAX_WAV_VALUE, self._MAX_WAV_VALUE).astype(np.int16)
        return self._audio_int16_array

    @property
    def audio_int16_bytes(self) -> bytes:
        return self.audio_int16_array.tobytes()


@dataclass
class TTSVoice:
    session: Any  # MiSession (or anything with get_inputs()/run(): the onnxruntime duck type)
    config: VoiceConfig
    phonetic_spellings: Optional[Any] = None
    phonemizer: Optional[Any] = None
    dedupe_sentences: bool = False  # False = reference behaviour (every sentence list is doubled)
    # extension: deliver audio at this rate instead of config.sample_rate, resampled on the device by the session
    output_sample_rate: Optional[int] = None
    # extension: phoneme_pitch / pitch_contour together with an output rate - the session folds the rate into the warp on the
    # device (MiSession.set_pitch_at_rate).  False: they are refused with an output rate set, as they always were.
    pitch_at_rate: bool = False

    def __post_init__(self):
        if self.pitch_at_rate:
            if not hasattr(self.session, "set_pitch_at_rate"):
                raise ValueError("pitch_at_rate needs a session that folds an output rate into the warp on the device "
                                 f"(MiSession.set_pitch_at_rate); {type(self.session).__name__} has none")
            self.session.set_pitch_at_rate(True)
        if self.output_sample_rate is not None:
            if not hasattr(self.session, "set_output_rate"):
                raise ValueError("output_sample_rate needs a session that resamples on the device (MiSession.set_output_rate); "
                                 f"{type(self.session).__name__} has none")
            self.session.set_output_rate(int(self.output_sample_rate), int(self.config.sample_rate))
        if self.phonemizer is None:
            self.phonemizer = get_phonemizer(self.config.phoneme_type, self.config.alphabet,
                                             self.config.phonemizer_model)

    # ------------------------------------------------------------------ construction
    @staticmethod
    def load(model_path: Union[str, Path], config_path: Optional[Union[str, Path]] = None,
             phonemes_txt: Optional[str] = None, phoneme_map: Optional[str] = None, lang_code: Optional[str] = None,
             phoneme_type_str: Optional[str] = None, use_cuda: bool = False, device_id: int = 0,
             phonemizer: Optional[Any] = None, strict: bool = True, output_sample_rate: Optional[int] = None,
             session: Optional[Any] = None, pitch_at_rate: bool = False) -> "TTSVoice":
        """Load a voice: `<model>.onnx` + `<model>.onnx.json` (voice.py:125-172).  `use_cuda` is
        accepted for signature compatibility; the engine always runs on the MI355X `device_id`.
        strict (extension): raise ValueError when JSON, .onnx metadata and graph disagree (check_consistency).
        output_sample_rate (extension): deliver every chunk, WAV header included, at this rate: the session resamples on the
        device from config.sample_rate (MiSession.set_output_rate); ValueError with a session that cannot.
        session (extension): an already opened session to use instead of opening `model_path`.
        pitch_at_rate (extension): phoneme_pitch / pitch_contour take an output rate (MiSession.set_pitch_at_rate)."""
        import os
        from .session import MiSession
        if config_path is None:
            config_path = f"{model_path}.json"
            LOG.debug("Guessing voice config path: %s", config_path)
        if output_sample_rate is not None and session is not None and not hasattr(session, "set_output_rate"):
            raise ValueError("output_sample_rate needs a session that resamples on the device (MiSession.set_output_rate); "
                             f"{type(session).__name__} has none")
        if session is None:
            session = MiSession(str(model_path), sess_options=None, providers=["MI355XExecutionProvider"],
                                device_id=device_id)
        if os.path.exists(config_path):
            with open(config_path, "r", encoding="utf-8") as fh:
                config_dict = json.load(fh)
        else:
            # extension: no JSON next to the model -> rebuild the config from the
            # metadata_props export_onnx.py:335-350 wrote into the .onnx itself
            config_dict = config_from_metadata(session.get_modelmeta().custom_metadata_map)
        if strict and hasattr(session, "hparam"):
            try:
                check_consistency(config_dict, session.get_modelmeta().custom_metadata_map,
                                  session.hparam("n_speakers"), session.hparam("n_vocab"))
            except ValueError:
                session.close()
                raise
        config = VoiceConfig.from_dict(config_dict, phonemes_txt=phonemes_txt, lang_code=lang_code,
                                       phoneme_type_str=phoneme_type_str)
        return TTSVoice(session=session, config=config, phonemizer=phonemizer, output_sample_rate=output_sample_rate,
                        pitch_at_rate=pitch_at_rate)

    @property
    def sample_rate(self) -> int:
        """The rate of the audio this voice hands out: output_sample_rate, or the voice's own."""
        return int(self.output_sample_rate) if self.output_sample_rate is not None else self.config.sample_rate

    def _ratio(self, rate: Optional[int] = None) -> Optional[Tuple[int, int]]:
        """(L, M) = output rate / voice rate, reduced; None when the audio is not resampled.  rate: a request's own output
        rate where that is not this voice's."""
        import math
        fi, fo = int(self.config.sample_rate), self.sample_rate if rate is None else int(rate)
        if fi == fo:
            return None
        g = math.gcd(fi, fo)
        return fo // g, fi // g

    @staticmethod
    def _valid_samples(out, hop) -> np.ndarray:
        """Valid samples per row of a synthesize_batch result: "sample_lengths" (an output rate is set), else frames * hop."""
        return np.asarray(out["sample_lengths"] if "sample_lengths" in out else np.asarray(out["y_lengths"]) * hop, np.int64)

    # ------------------------------------------------------------------ text -> phonemes -> ids
    def phonemize(self, text: str) -> List[List[str]]:
        """Text to phonemes grouped by sentence; `[[ ... ]]` blocks carry literal phonemes."""
        sentences: List[List[str]] = []
        parts = _PHONEME_BLOCK.split(text)
        for i, part in enumerate(parts):
            if part.startswith("[["):
                if not sentences:
                    sentences.append([])
                if i > 0 and parts[i - 1].endswith(" "):
                    sentences[-1].append(" ")
                sentences[-1].extend(list(part[2:-2].strip()))
                if i < len(parts) - 1 and parts[i + 1].startswith(" "):
                    sentences[-1].append(" ")
                continue
            result = self.phonemizer.phonemize(part, self.config.lang_code)
            if self.dedupe_sentences:
                sentences.extend(result)
            else:
                # voice.py:203-206 replaces the accumulator by this part's result and extends it with itself
                sentences = result
                sentences.extend(sentences)
        if sentences and not sentences[-1]:
            sentences.pop()
        return sentences

    def phonemes_to_ids(self, phonemes: List[str]) -> List[int]:
        if self.config.phoneme_id_map is None:
            raise ValueError("self.config.phoneme_id_map is None")
        c = self.config
        return phonemes_to_ids(phonemes, c.phoneme_id_map, blank_token=c.blank_token, bos_token=c.bos_token,
                               eos_token=c.eos_token, word_sep_token=c.word_sep_token,
                               include_whitespace=c.include_whitespace, blank_at_start=c.blank_at_start,
                               blank_at_end=c.blank_at_end,
                               blank_between=BlankBetween.TOKENS_AND_WORDS)  # voice.py:231 ignores config.blank_between

    def phonemes_to_id_groups(self, phonemes: List[str]) -> List[Tuple[str, List[int]]]:
        """phonemes_to_ids with the ids grouped by the phoneme they came from (phoneme_ids.phonemes_to_id_groups)."""
        if self.config.phoneme_id_map is None:
            raise ValueError("self.config.phoneme_id_map is None")
        c = self.config
        return phonemes_to_id_groups(phonemes, c.phoneme_id_map, blank_token=c.blank_token, bos_token=c.bos_token,
                                     eos_token=c.eos_token, word_sep_token=c.word_sep_token,
                                     include_whitespace=c.include_whitespace, blank_at_start=c.blank_at_start,
                                     blank_at_end=c.blank_at_end, blank_between=BlankBetween.TOKENS_AND_WORDS)

    # ------------------------------------------------------------------ synthesis
    def _postprocess(self, audio: np.ndarray, syn_config: SynthesisConfig) -> np.ndarray:
        """voice.py:271-282: peak-normalise, volume, clip, float32."""
        if syn_config.normalize_audio:
            peak = np.max(np.abs(audio))
            audio = np.zeros_like(audio) if peak < 1e-8 else audio / peak
        if syn_config.volume != 1.0:
            audio = audio * syn_config.volume
        return np.clip(audio, -1.0, 1.0).astype(np.float32)

    def synthesize(self, text: str, syn_config: Optional[SynthesisConfig] = None,
                   batch_sentences: bool = False, alignments: bool = False) -> Iterable[AudioChunk]:
        """One AudioChunk per sentence.  `batch_sentences=True` (extension) renders all sentences in a
        single padded batch on the GPU instead of one engine call per sentence.  `alignments=True` (extension) fills
        AudioChunk.phoneme_alignments from the durations the engine reports; with a session that reports none (the
        onnxruntime duck type) the field stays None."""
        if syn_config is None:
            syn_config = SynthesisConfig()
        if alignments and hasattr(self.session, "last_durations") and hasattr(self.session, "synthesize_batch"):
            yield from self._synthesize_aligned(text, syn_config, batch_sentences)
            return
        all_ids = self._sentence_ids(text, syn_config)
        if batch_sentences and len(all_ids) > 1 and hasattr(self.session, "synthesize_batch"):
            audios = self.phoneme_ids_batch_to_audio(all_ids, syn_config)
        else:
            audios = (self.phoneme_ids_to_audio(ids, syn_config) for ids in all_ids)
        for audio in audios:
            yield AudioChunk(sample_rate=self.sample_rate, sample_width=2, sample_channels=1,
                             audio_float_array=self._postprocess(audio, syn_config))

    def _synthesize_aligned(self, text: str, syn_config: SynthesisConfig, batch_sentences: bool) -> Iterable[AudioChunk]:
        """synthesize() with per-phoneme timing: the same engine calls, asked for their durations as well."""
        all_groups = self._sentence_groups(text, syn_config)
        all_ids = [[i for _, ids in g for i in ids] for g in all_groups]
        hop = self.session.hparam("hop")
        if batch_sentences and len(all_ids) > 1:
            rows = zip(*self.phoneme_ids_batch_to_audio(all_ids, syn_config, return_durations=True))
        else:
            # (a batch of one is what session.run issues, voice.py:374; the durations come back with the same call)
            rows = ((a[0], d[0]) for a, d in (self.phoneme_ids_batch_to_audio([ids], syn_config, return_durations=True)
                                              for ids in all_ids))
        ratio = self._ratio()
        for groups, (audio, dur) in zip(all_groups, rows):
            # (the engine renders max(1, sum of durations) frames; natively that is the chunk's length in frames)
            frames = len(audio) // hop if ratio is None else max(1, int(np.sum(dur)))
            yield AudioChunk(sample_rate=self.sample_rate, sample_width=2, sample_channels=1,
                             audio_float_array=self._postprocess(audio, syn_config),
                             phoneme_alignments=build_alignments(groups, dur, hop, total_frames=frames, ratio=ratio))

    def _sentence_phonemes(self, text: str, syn_config: SynthesisConfig) -> List[List[str]]:
        """synthesize()'s front end up to the phonemes: phonetic spellings, diacritics, phonemize."""
        LOG.debug("text=%s", text)
        if self.phonetic_spellings and syn_config.enable_phonetic_spellings:
            text = self.phonetic_spellings.apply(text)
        if syn_config.add_diacritics:
            text = self.phonemizer.add_diacritics(text, self.config.lang_code)
        sentence_phonemes = self.phonemize(text)
        LOG.debug("phonemes=%s", sentence_phonemes)
        return sentence_phonemes

    def _sentence_ids(self, text: str, syn_config: SynthesisConfig) -> List[List[int]]:
        """synthesize()'s front end: phonetic spellings, diacritics, phonemize, ids - one non-empty id list per sentence."""
        all_ids = [self.phonemes_to_ids(p) for p in self._sentence_phonemes(text, syn_config) if p]
        return [ids for ids in all_ids if ids]

    def _sentence_groups(self, text: str, syn_config: SynthesisConfig) -> List[List[Tuple[str, List[int]]]]:
        """_sentence_ids with every sentence's ids grouped by phoneme (flattened: exactly _sentence_ids' lists)."""
        all_groups = [self.phonemes_to_id_groups(p) for p in self._sentence_phonemes(text, syn_config) if p]
        return [g for g in all_groups if any(ids for _, ids in g)]

    def synthesize_requests(self, requests: Sequence[Tuple[str, Optional[SynthesisConfig]]],
                            seeds: Optional[Sequence[int]] = None, max_batch: int = 32,
                            alignments: bool = False, postprocess: bool = True,
                            _durations: Optional[dict] = None) -> List[List[AudioChunk]]:
        """Extension: many independent requests (text, SynthesisConfig or None) rendered together.  Every sentence of
        every request becomes one row of a batch with its request's own speaker, length / noise scales and (with `seeds`,
        one integer per request) its own noise seed - sentence k of request r: sentence_seed(seeds[r], k); rows are sorted
        by length and rendered max_batch at a time.  Returns, per request, what list(synthesize(text, cfg)) returns: one
        AudioChunk per sentence, post-processed with that request's normalize_audio / volume.  With seeds, a request's
        durations do not depend on which other requests share its batches (vitsmi.h, vits_run_async_rows).  A session
        without synthesize_batch (the onnxruntime duck type) renders the requests one by one through synthesize().
        alignments=True fills every chunk's phoneme_alignments as synthesize(text, cfg, alignments=True) does.
        postprocess=False (what synthesize_requests_encoded's trimmed fallback asks for: the cut comes before the peak) returns
        the rows as rendered - no normalisation, volume or clipping; everything else, alignments included, as with True (a
        session without synthesize_batch reports no durations either way, so its chunks carry no alignments).
        _durations (internal: synthesize_requests_encoded's shaped fallback): a dict that receives the frames per phoneme id
        of sentence k of request r under (r, k); needs a session with synthesize_batch."""
        if max_batch < 1:
            raise ValueError(f"max_batch must be >= 1 (got {max_batch})")
        if seeds is not None and len(seeds) != len(requests):
            raise ValueError(f"seeds must hold one seed per request ({len(requests)}), got {len(seeds)}")
        cfgs = [cfg if cfg is not None else SynthesisConfig() for _, cfg in requests]
        expected = [i.name for i in self.session.get_inputs()]
        if "sid" in expected:  # every request's speaker is checked before anything runs
            n_spk = int(self.session.hparam("n_speakers")) if hasattr(self.session, "hparam") else self.config.num_speakers
            for r, cfg in enumerate(cfgs):
                spk = cfg.speaker_id or 0
                if not 0 <= spk < max(n_spk, 1):
                    raise ValueError(f"request {r}: speaker_id {spk} is out of range [0, {max(n_spk, 1)})")
        if not hasattr(self.session, "synthesize_batch"):
            if _durations is not None:
                raise ValueError("phoneme_gain_db needs a session that reports durations (synthesize_batch)")
            if not postprocess:
                return [[AudioChunk(sample_rate=self.sample_rate, sample_width=2, sample_channels=1,
                                    audio_float_array=np.atleast_1d(self.phoneme_ids_to_audio(ids, cfg)))
                         for ids in self._sentence_ids(text, cfg)] for (text, _), cfg in zip(requests, cfgs)]
            return [list(self.synthesize(text, cfg, alignments=alignments)) for (text, _), cfg in zip(requests, cfgs)]
        from .sharding import pad_batch
        want_dur = alignments and hasattr(self.session, "last_durations")
        rows = []  # (request, sentence, ids)
        groups = {}
        for r, ((text, _), cfg) in enumerate(zip(requests, cfgs)):
            if want_dur:
                for k, g in enumerate(self._sentence_groups(text, cfg)):
                    groups[r, k] = g
                    rows.append((r, k, [i for _, ids in g for i in ids]))
            else:
                rows.extend((r, k, ids) for k, ids in enumerate(self._sentence_ids(text, cfg)))
        audio = {}
        aligned = {}
        more = {"return_durations": True} if want_dur or _durations is not None else {}
        hop = self.session.hparam("hop")
        order = sorted(range(len(rows)), key=lambda i: len(rows[i][2]))  # (stable: equal lengths keep request order)
        for c0 in range(0, len(order), max_batch):
            run = [rows[i] for i in order[c0:c0 + max_batch]]
            ids, lens = pad_batch([ids for _, _, ids in run])
            scales = np.stack([self._scales(cfgs[r]) for r, _, _ in run])
            sid = np.asarray([cfgs[r].speaker_id or 0 for r, _, _ in run], np.int64) if "sid" in expected else None
            if seeds is None:
                out = self.session.synthesize_batch(ids, lens, scales, sid, **more)
            else:
                row_seeds = np.asarray([sentence_seed(seeds[r], k) for r, k, _ in run], np.uint64)
                out = self.session.synthesize_batch(ids, lens, scales, sid, seeds=row_seeds, **more)
            valid = self._valid_samples(out, hop)
            for b, (r, k, ids_b) in enumerate(run):
                audio[r, k] = out["output"][b, 0, 0, :int(valid[b])].copy()
                if _durations is not None:
                    _durations[r, k] = np.asarray(out["durations"][b, :len(ids_b)], np.int64).copy()
                if want_dur:
                    aligned[r, k] = build_alignments(groups[r, k], out["durations"][b], hop,
                                                     total_frames=int(out["y_lengths"][b]), ratio=self._ratio())
        result = [[] for _ in requests]
        for r, k, _ in rows:  # (rows are in request, then sentence order)
            result[r].append(AudioChunk(sample_rate=self.sample_rate, sample_width=2, sample_channels=1,
                                        audio_float_array=self._postprocess(audio[r, k], cfgs[r]) if postprocess else audio[r, k],
                                        phoneme_alignments=aligned.get((r, k))))
        return result

    # ------------------------------------------------------------------ encoded delivery (extension)
    def _lead_samples(self, sentence_silence: float, rate: Optional[int] = None) -> int:
        """Samples of silence in front of every sentence: the reference's framing (voice.py:307-326 writes
        int(sample_rate * sentence_silence * 2) bytes of 16-bit silence) wherever that byte count is even.  rate: the rate the
        audio is delivered at where that is not this voice's (a request's own: synthesize_requests_encoded)."""
        if not sentence_silence >= 0.0:
            raise ValueError(f"sentence_silence must be >= 0 (got {sentence_silence})")
        return int((self.sample_rate if rate is None else rate) * sentence_silence * 2) // 2

    @staticmethod
    def _scaled(audio: np.ndarray, peak, volume: float) -> np.ndarray:
        """_postprocess with the peak given (None: no normalisation): the same float32 operations in the same order."""
        from . import audio_encoding as ae
        return ae.scaled(audio, peak, volume)

    def _trim(self, trim_silence, trailing_silence: float, rate: Optional[int] = None):
        """trim_silence / trailing_silence of the encoded entries -> a session.Trim in samples at the delivered rate, or None
        when both are left at their defaults.  A float is a threshold relative to the sentence's peak; a Trim is taken with
        keep_lead / keep_tail in SECONDS, converted like the pause (_lead_samples); trailing_silence, in seconds, is added to
        its tail_samples."""
        from .session import Trim
        if not trailing_silence >= 0.0:
            raise ValueError(f"trailing_silence must be >= 0 (got {trailing_silence})")
        tail = self._lead_samples(trailing_silence, rate)
        if trim_silence is None:
            return Trim(0, 0.0, 0, 0, tail) if tail else None
        if isinstance(trim_silence, Trim):
            t = trim_silence
            if not (t.keep_lead >= 0 and t.keep_tail >= 0):
                raise ValueError(f"trim_silence: keep_lead / keep_tail must be >= 0 seconds (got {t.keep_lead}, {t.keep_tail})")
            return Trim(int(t.mode), float(t.threshold), self._lead_samples(t.keep_lead, rate), self._lead_samples(t.keep_tail, rate),
                        int(t.tail_samples) + tail)
        thr = float(trim_silence)
        if not (thr >= 0.0 and np.isfinite(thr)):
            raise ValueError(f"trim_silence must be a finite threshold >= 0 (got {trim_silence})")
        return Trim(2, thr, 0, 0, tail)

    @staticmethod
    def _level(loudness, loudness_scope: str, peak_ceiling: float, max_gain_db: float, configs):
        """loudness / loudness_scope / peak_ceiling / max_gain_db of the encoded entries -> a session.Level, or None when
        loudness is None.  Levelling replaces peak normalisation: a config with normalize_audio=True is refused."""
        from .session import Level
        if loudness_scope not in ("sentence", "text"):
            raise ValueError(f"loudness_scope must be 'sentence' or 'text' (got {loudness_scope!r})")
        if loudness is None:
            return None
        target = float(loudness)
        if not (np.isfinite(target) and -70.0 <= target <= 0.0):
            raise ValueError(f"loudness must be a target in LUFS within [-70, 0] (got {loudness})")
        if not (np.isfinite(max_gain_db) and 0.0 <= max_gain_db <= 120.0):
            raise ValueError(f"max_gain_db must be within [0, 120] (got {max_gain_db})")
        if not (np.isfinite(peak_ceiling) and 0.0 <= peak_ceiling <= 1.0):
            raise ValueError(f"peak_ceiling must be within [0, 1], 0 for none (got {peak_ceiling})")
        if any(c.normalize_audio for c in configs):
            raise ValueError("loudness levelling replaces peak normalisation: pass a SynthesisConfig with normalize_audio=False")
        return Level(1 if loudness_scope == "sentence" else 2, target, float(max_gain_db), float(peak_ceiling))

    def _shape(self, fade_in: float, fade_out: float, fade_curve: str, rate: Optional[int] = None):
        """fade_in / fade_out (seconds) and fade_curve of the encoded entries -> a session.Shape in samples at the delivered
        rate (int(sample_rate * seconds)), or None when neither fades."""
        from .session import Shape
        for name, v in (("fade_in", fade_in), ("fade_out", fade_out)):
            if not (v >= 0.0 and np.isfinite(v)):
                raise ValueError(f"{name} must be a finite number of seconds >= 0 (got {v})")
        if fade_curve not in ("linear", "smooth"):
            raise ValueError(f"fade_curve must be 'linear' or 'smooth' (got {fade_curve!r})")
        rate = self.sample_rate if rate is None else rate
        fi, fo = int(rate * fade_in), int(rate * fade_out)
        return Shape(fi, fo, fade_curve) if fi or fo else None

    def _limit(self, limit_ceiling: float, limit_lookahead: float, rate: Optional[int] = None):
        """limit_ceiling / limit_lookahead (seconds) of the encoded entries -> a session.Limit with the look-ahead in samples
        at the delivered rate (round(limit_lookahead * sample_rate)), or None when limit_ceiling is 0."""
        from .session import Limit
        if not (np.isfinite(limit_ceiling) and 0.0 <= limit_ceiling <= 1.0):
            raise ValueError(f"limit_ceiling must be within (0, 1], 0 for no limiter (got {limit_ceiling})")
        if limit_ceiling == 0.0:
            return None
        if not (np.isfinite(limit_lookahead) and limit_lookahead >= 0.0):
            raise ValueError(f"limit_lookahead must be a finite number of seconds >= 0 (got {limit_lookahead})")
        rate = self.sample_rate if rate is None else rate
        L = int(round(limit_lookahead * rate))
        if not 1 <= L <= 1024:
            raise ValueError(f"limit_lookahead {limit_lookahead} s is {L} samples at {rate} Hz: outside [1, 1024]")
        return Limit(float(limit_ceiling), L)

    @staticmethod
    def _group_db(phoneme_gain_db, k: int, groups) -> List[float]:
        """phoneme_gain_db(k, [the tokens of sentence k's groups]) -> one dB value per phoneme id: all ids of a group, its
        blanks included, take the group's value"""
        vals = list(phoneme_gain_db(k, [token for token, _ in groups]))
        if len(vals) != len(groups):
            raise ValueError(f"phoneme_gain_db returned {len(vals)} values for the {len(groups)} groups of sentence {k}")
        return [float(v) for v, (_, ids) in zip(vals, groups) for _ in ids]

    @staticmethod
    def _group_semitones(phoneme_pitch, k: int, groups) -> List[float]:
        """phoneme_pitch -> one value in semitones per phoneme id of sentence k, expanded over the id groups as _group_db
        expands a volume: a float is the whole sentence's; a callable (sentence_index, [the groups' tokens]) or a sequence
        indexed by the sentence gives one value per group, which all ids of the group, its blanks included, take"""
        if callable(phoneme_pitch):
            vals = list(phoneme_pitch(k, [token for token, _ in groups]))
        elif isinstance(phoneme_pitch, (int, float, np.integer, np.floating)):
            vals = [float(phoneme_pitch)] * len(groups)
        else:
            vals = list(phoneme_pitch[k])
        if len(vals) != len(groups):
            raise ValueError(f"phoneme_pitch gives {len(vals)} values for the {len(groups)} groups of sentence {k}")
        vals = [float(v) for v in vals]
        for v in vals:
            if not (np.isfinite(v) and abs(v) <= 12.0):
                raise ValueError(f"phoneme_pitch: {v} semitones in sentence {k} is not a finite value within [-12, 12]")
        return [v for v, (_, ids) in zip(vals, groups) for _ in ids]

    @staticmethod
    def _group_contour(pitch_contour, k: int, groups):
        """pitch_contour -> (start, end) values in semitones per phoneme id of sentence k.  The contour is a sequence of
        (position in [0, 1], semitones) points, positions non-decreasing, or a callable (sentence_index, [the groups'
        tokens]) -> such a sequence.  Positions are fractions of the sentence's PHONEME COUNT: with n groups, boundary i lies
        at i / n, and its value is interpolated linearly in semitones between the points on either side of it - the first
        point's value in front of it, the last one's behind it, the later one's where two points share a position.
        Group i glides from value(i / n) to value((i + 1) / n).  THE id-level rule: a group of m ids splits its glide
        into m equal parts in semitones - id q starts at v0 + (v1 - v0) * q / m and ends where id q + 1 starts, the last
        at v1 itself - so the value is continuous across the ids of a group, its blanks included."""
        pts = pitch_contour(k, [token for token, _ in groups]) if callable(pitch_contour) else pitch_contour
        try:
            pts = [(float(p), float(v)) for p, v in pts]
        except (TypeError, ValueError):
            raise ValueError(f"pitch_contour of sentence {k} must be a sequence of (position, semitones) points") from None
        if not pts:
            raise ValueError(f"pitch_contour of sentence {k} has no point")
        for i, (p, v) in enumerate(pts):
            if not (np.isfinite(p) and 0.0 <= p <= 1.0) or (i and p < pts[i - 1][0]):
                raise ValueError(f"pitch_contour: position {p} in sentence {k} is not within [0, 1] in non-decreasing order")
            if not (np.isfinite(v) and abs(v) <= 12.0):
                raise ValueError(f"pitch_contour: {v} semitones in sentence {k} is not a finite value within [-12, 12]")

        def value(x):
            j = max((i for i, (p, _) in enumerate(pts) if p <= x), default=-1)
            if j < 0:
                return pts[0][1]
            if j == len(pts) - 1:
                return pts[j][1]
            (p0, v0), (p1, v1) = pts[j], pts[j + 1]
            return v0 + (v1 - v0) * (x - p0) / (p1 - p0)

        n = len(groups)
        st0, st1 = [], []
        for i, (_, ids) in enumerate(groups):
            v0, v1 = value(i / n), value((i + 1) / n)
            m = len(ids)
            cuts = [v0] + [v0 + (v1 - v0) * q / m for q in range(1, m)] + [v1]
            st0 += cuts[:m]
            st1 += cuts[1:m + 1]
        return st0, st1

    @classmethod
    def _sentence_semitones(cls, phoneme_pitch, pitch_contour, k: int, groups):
        """(start values, end values or None) per phoneme id of sentence k: phoneme_pitch alone is _group_semitones' constant
        tokens; a pitch_contour glides, with phoneme_pitch - if given too - added to both ends"""
        base = None if phoneme_pitch is None else cls._group_semitones(phoneme_pitch, k, groups)
        if pitch_contour is None:
            return base, None
        st0, st1 = cls._group_contour(pitch_contour, k, groups)
        if base is not None:
            st0, st1 = [a + c for a, c in zip(st0, base)], [b + c for b, c in zip(st1, base)]
            for v in st0 + st1:
                if not abs(v) <= 12.0:
                    raise ValueError(f"pitch_contour + phoneme_pitch: {v} semitones in sentence {k} is not within [-12, 12]")
        return st0, st1

    def _contour_check(self, pitch_contour, rates=None) -> None:
        """pitch_contour needs a session whose delivery takes end values, and audio at the voice's own rate - or a voice with
        pitch_at_rate: the output rate is then folded into the glide on the device (vitsmi.h, "pitch at an output rate"; the
        engine refuses a rate outside a quarter .. four times the voice's own)"""
        import inspect
        if pitch_contour is None:
            return
        fn = getattr(self.session, "synthesize_delivered", None)
        if fn is None or "token_semitones_end" not in inspect.signature(fn).parameters:
            raise ValueError("pitch_contour needs a session that glides on the device (synthesize_delivered(token_semitones_end=))")
        if not self.pitch_at_rate and (self._ratio() is not None or any(self._ratio(r) is not None for r in rates or ())):
            raise ValueError("pitch_contour is not covered with an output rate set")
        if self.pitch_at_rate:
            self._rate_admitted("pitch_contour", rates)

    def _rate_admitted(self, what: str, rates=None) -> None:
        """with pitch_at_rate: the rates pitch can be folded into lie within a quarter .. four times the voice's own"""
        for r in [None] + list(rates or ()):
            lm = self._ratio(r)
            if lm is not None and (lm[1] > 4 * lm[0] or lm[0] > 4 * lm[1]):
                raise ValueError(f"{what} is not covered at {self.sample_rate if r is None else int(r)} Hz: the ratio to the voice's "
                                 f"{int(self.config.sample_rate)} Hz lies outside [1/4, 4]")

    def _pitch_check(self, phoneme_pitch, rates=None) -> None:
        """phoneme_pitch needs a session whose delivery takes semitones, and audio at the voice's own rate - or a voice with
        pitch_at_rate, as for pitch_contour"""
        import inspect
        if phoneme_pitch is None:
            return
        fn = getattr(self.session, "synthesize_delivered", None)
        if fn is None or "token_semitones" not in inspect.signature(fn).parameters:
            raise ValueError("phoneme_pitch needs a session that warps on the device (synthesize_delivered(token_semitones=))")
        if not self.pitch_at_rate and (self._ratio() is not None or any(self._ratio(r) is not None for r in rates or ())):
            raise ValueError("phoneme_pitch is not covered with an output rate set")
        if self.pitch_at_rate:
            self._rate_admitted("phoneme_pitch", rates)

    def _duration_fit(self, duration, duration_mode: str, n_sentences: int, pauses: int, entry: str, pitched: bool):
        """duration= / duration_mode= of the encoded entries -> a session.Fit with all sentences in one group, or None.
        `pauses`: the samples of silence the call itself adds, at the delivered rate.  The target is
        round((duration * delivered_rate - pauses) * native_rate / (delivered_rate * hop)) frames."""
        import inspect
        import math
        if duration is None:
            return None
        from .session import FIT_MODES, Fit
        if duration_mode not in FIT_MODES:
            raise ValueError(f"duration_mode must be 'exact' or 'at_most' (got {duration_mode!r})")
        if not (isinstance(duration, (int, float, np.integer, np.floating)) and np.isfinite(duration) and duration > 0):
            raise ValueError(f"duration must be a finite number of seconds > 0 (got {duration!r})")
        if pitched:
            raise ValueError("duration together with phoneme_pitch / pitch_contour is not covered: the warped length is not the "
                             "native frame count")
        fn = getattr(self.session, entry, None)
        if fn is None or "fit" not in inspect.signature(fn).parameters:
            raise ValueError(f"duration needs a session that fits durations on the device ({entry}(fit=))")
        rate, native, hop = self.sample_rate, int(self.config.sample_rate), int(self.session.hparam("hop"))
        frames = int(math.floor((float(duration) * rate - pauses) * native / (rate * hop) + 0.5))
        if frames < 1:
            raise ValueError(f"duration {duration} s leaves {frames} frames for the speech behind {pauses} samples of pauses: "
                             "below 1 frame")
        return Fit.one_group(n_sentences, frames, duration_mode)

    @staticmethod
    def _padded_db(token_db) -> np.ndarray:
        """per-row dB lists -> [B, T], 0 dB behind each row's end (tokens of no frames: they never show)"""
        db = np.zeros((len(token_db), max(len(q) for q in token_db)), np.float64)
        for b, q in enumerate(token_db):
            db[b, :len(q)] = q
        return db

    def _row_shapes(self, shape, token_db, durs, counts, rates=None, spans=None):
        """The host fallback's shapes, one per row: `shape` (or none), with the points of each row's token gains - what
        MiSession.synthesize_delivered(token_gain_db=) computes between run and delivery, from the same durations.
        rates: None, or the rate each row is delivered at (`shape` is then one Shape, or none, per row).  spans: None, or the
        token spans of warped rows (phoneme_pitch): the boundaries are then theirs."""
        from .session import Segment, Shape, token_bounds, token_gain_shapes, token_gains, token_span_bounds
        n = len(counts)
        if rates is None:
            shapes = [shape if shape is not None else Shape()] * n
        else:
            shapes = [sh if sh is not None else Shape() for sh in shape]
        if token_db is None:
            return shapes
        db = self._padded_db(token_db)
        hop = self.session.hparam("hop")
        ratios = [self._ratio()] * n if rates is None else [self._ratio(r) for r in rates]
        if spans is not None:
            bounds = [token_span_bounds(spans[b], counts[b]) for b in range(n)]
        else:
            bounds = [token_bounds(durs[b], len(token_db[b]), hop, counts[b], ratios[b]) for b in range(n)]
        ramp = int(self.sample_rate * _GAIN_RAMP) if rates is None else [int(int(r) * _GAIN_RAMP) for r in rates]
        return token_gain_shapes([Segment(b) for b in range(n)], shapes, token_gains(db, *db.shape), bounds, ramp)

    @staticmethod
    def _cut_alignments(al, a: int, c: int):
        """A sentence's alignments after its audio was cut to [a, a + c): every phoneme's [start, start + num) shifted by -a
        and clamped to [0, c] - num_samples still sum to c, a phoneme that was trimmed away keeps 0 samples."""
        for p in al:
            lo = min(max(p.start_sample - a, 0), c)
            hi = min(max(p.start_sample + p.num_samples - a, 0), c)
            p.start_sample, p.num_samples = lo, hi - lo
        return al

    def synthesize_encoded(self, text: str, syn_config: Optional[SynthesisConfig] = None, encoding: str = "pcm16",
                           sentence_silence: float = 0.0, normalize_scope: str = "sentence",
                           alignments: bool = False, trim_silence=None, trailing_silence: float = 0.0, loudness=None,
                           loudness_scope: str = "sentence", peak_ceiling: float = 0.0, max_gain_db: float = 30.0,
                           fade_in: float = 0.0, fade_out: float = 0.0, fade_curve: str = "linear", phoneme_gain_db=None,
                           limit_ceiling: float = 0.0, limit_lookahead: float = 0.005, phoneme_pitch=None, pitch_contour=None,
                           duration: Optional[float] = None, duration_mode: str = "exact"):
        """Extension: the whole text as ONE stream of encoded audio ("pcm16", "ulaw", "alaw", "f32"; audio_encoding).  All
        sentences render in one batch; with a session that delivers (MiSession.synthesize_delivered) post-processing,
        encoding and the packing happen on the device and only the encoded audio crosses the bus; any other session
        gets the same bytes from the host encoder.  In front of every sentence, the first included, lie
        int(sample_rate * sentence_silence * 2) // 2 samples of silence.  normalize_scope: "sentence" - each sentence by its
        own peak (what synthesize() does), "text" - all by the largest peak of the text, so that their relative levels
        survive.  alignments=True fills phoneme_alignments (per sentence; start_sample counted from the stream's start).
        trim_silence (None; a float: the threshold as a fraction of the sentence's peak; or a session.Trim with keep_lead /
        keep_tail in seconds) cuts every sentence to its first .. last sample above the threshold - on the device with a
        session that delivers (vitsmi.h, "trimmed delivery"), by audio_encoding.join_trimmed otherwise: the same bytes -
        and trailing_silence seconds of silence follow every sentence.  Peaks are then those of what is kept,
        sentence_samples the kept lengths, and the alignments are cut to the kept ranges (they still sum to
        sentence_samples; a phoneme that was trimmed away has num_samples == 0).
        loudness (None, or a target in LUFS) brings what is kept of every sentence (loudness_scope "sentence") or of the text
        as a whole ("text": one gain, relative levels survive) to that integrated loudness (ITU-R BS.1770-4; vitsmi.h,
        "levelled delivery") instead of peak-normalising it - the config must say normalize_audio=False.  The gain is at most
        max_gain_db; peak_ceiling > 0 keeps the levelled sample peak (not the true peak) at or below it.  A sentence shorter
        than 400 ms has no integrated loudness and keeps gain 1.  Measured on the device with a session that delivers, by
        audio_encoding.join_leveled otherwise (float64: the gains agree to meter accuracy, not bit for bit).  The result's
        `loudness` and `gain` hold what was measured and applied per sentence.
        fade_in / fade_out (seconds; int(sample_rate * seconds) samples) ramp what is kept of every sentence up from and down
        to exactly 0, along fade_curve "linear" or "smooth" - no step next to the silence of a pause.  phoneme_gain_db - a
        callable (sentence_index, [the tokens of the sentence's groups, as phonemes_to_id_groups gives them]) -> one volume
        in dB per group (-inf: silent; else within [-120, 36]): every phoneme is delivered at its own volume, with a ramp of
        10 ms around each change.  Both are a time-varying volume in front of the clip (vitsmi.h, "shaped delivery"): on the
        device with a session that delivers, by audio_encoding's shapes= otherwise - the same bytes; peaks, trimming and
        loudness see the unshaped audio.  phoneme_gain_db needs a session that reports durations.
        limit_ceiling (0: off; else within (0, 1]) puts a look-ahead peak limiter behind all of that, in front of the clip
        (vitsmi.h, "limited delivery"): no sample of a sentence exceeds the ceiling, and the gain ducks under a peak from
        limit_lookahead seconds ahead of it to as long behind it (round(limit_lookahead * sample_rate) samples, within
        [1, 1024]) - a loudness target or a boost can then be reached without flattening the peaks.  On the device with a
        session that delivers, by audio_encoding's limits= otherwise: the same bytes.
        phoneme_pitch - in semitones within [-12, 12]: a float for every sentence, or a value per phoneme as phoneme_gain_db
        gives a volume (a callable, or one sequence per sentence) - raises or lowers the voice by a time warp on the device
        (vitsmi.h, "intonation": the resampling shift - formants move along; good for a few semitones).  The tempo is kept.
        Alignments then come from the warp's token spans, and every sample-valued option - fades, per-phoneme volume, trims,
        look-ahead - is laid out over the warped audio.  It needs a session that warps (ValueError otherwise) and a voice
        without an output_sample_rate (ValueError "not covered with an output rate set") - unless the voice was made with
        pitch_at_rate=True: an output_sample_rate (or output_sample_rates per request) is then folded into the warp on the device (vitsmi.h,
        "pitch at an output rate"): one filter pass, spans and alignments in delivered samples; a rate outside a quarter .. four
        times the voice's own is refused by the engine for a pitched sentence.
        pitch_contour - SSML's contour, applied to each sentence: a sequence of (position in [0, 1], semitones within
        [-12, 12]) points with non-decreasing positions, or a callable (sentence_index, tokens) -> such a sequence.  The pitch
        GLIDES through the points (vitsmi.h, "pitch contours"): linear in semitones between them, the first and the last
        value held outside them.  Positions are fractions of the sentence's PHONEME COUNT, not of time - durations do not
        exist before the run: with n phoneme groups, group i glides from the contour's value at i / n to its value at
        (i + 1) / n.  phoneme_pitch, if given too, is added to both ends; a sum outside [-12, 12] is a ValueError naming the
        sentence.  Tempo, alignments and sample-valued options as for phoneme_pitch.  It needs a session that glides
        (ValueError otherwise) and is refused with an output rate set, or takes it, as phoneme_pitch does.
        duration - SSML's <prosody duration>, in seconds: the text is FITTED to that length on the device (vitsmi.h, "fitted
        durations": all sentences form one group and share one multiplier on the model's own durations, so the speech is what
        the model renders at another length scale).  duration_mode "exact" meets it - to within half a frame, plus one sample
        per sentence at an output rate -, "at_most" leaves a text alone that is already shorter.  The duration is that of the
        RENDERED audio, the pauses this call adds included, BEFORE trim_silence: trimming shortens it further.  The model's
        multiplier stays within [1/16, 16].  It needs a session whose synthesize_delivered takes fit= (ValueError otherwise), is
        not covered together with phoneme_pitch / pitch_contour (ValueError), and a target below one frame is a ValueError.
        The result's fit_scale and fit_status hold the multiplier and the outcome (session.last_fit()).
        Returns an audio_encoding.EncodedAudio."""
        from . import audio_encoding as ae
        from .sharding import pad_batch
        cfg = syn_config if syn_config is not None else SynthesisConfig()
        ae._check(encoding)
        if normalize_scope not in ("sentence", "text"):
            raise ValueError(f"normalize_scope must be 'sentence' or 'text' (got {normalize_scope!r})")
        lead = self._lead_samples(sentence_silence)
        trim = self._trim(trim_silence, trailing_silence)
        level = self._level(loudness, loudness_scope, peak_ceiling, max_gain_db, [cfg])
        shape = self._shape(fade_in, fade_out, fade_curve)
        limit = self._limit(limit_ceiling, limit_lookahead)
        tail = trim.tail_samples if trim is not None else 0
        kept = loud = gains = None
        want_dur = alignments and hasattr(self.session, "last_durations") and hasattr(self.session, "synthesize_batch")
        if phoneme_gain_db is not None and not (hasattr(self.session, "synthesize_delivered") or hasattr(self.session, "synthesize_batch")):
            raise ValueError("phoneme_gain_db needs a session that reports durations (synthesize_batch)")
        self._pitch_check(phoneme_pitch)
        self._contour_check(pitch_contour)
        pitched = phoneme_pitch is not None or pitch_contour is not None
        groups = self._sentence_groups(text, cfg) if want_dur or phoneme_gain_db is not None or pitched else None
        all_ids = [[i for _, ids in g for i in ids] for g in groups] if groups is not None else self._sentence_ids(text, cfg)
        if not all_ids:
            return ae.EncodedAudio(ae.silence(0, encoding), encoding, self.sample_rate, [], [], [] if want_dur else None)
        token_db = None if phoneme_gain_db is None else [self._group_db(phoneme_gain_db, k, g) for k, g in enumerate(groups)]
        token_st = token_st_end = None
        if pitched:
            pairs = [self._sentence_semitones(phoneme_pitch, pitch_contour, k, g) for k, g in enumerate(groups)]
            token_st = [a for a, _ in pairs]
            token_st_end = None if pitch_contour is None else [b for _, b in pairs]
        durs = frames = spans = None
        fit = self._duration_fit(duration, duration_mode, len(all_ids), len(all_ids) * (lead + tail), "synthesize_delivered", pitched)
        fit_scale = fit_status = None
        if hasattr(self.session, "synthesize_delivered"):
            from .session import Segment
            ids, lens = pad_batch(all_ids)
            expected = [i.name for i in self.session.get_inputs()]
            if "sid" in expected:  # (checked before anything runs, as synthesize_requests_encoded does)
                n_spk = int(self.session.hparam("n_speakers")) if hasattr(self.session, "hparam") else self.config.num_speakers
                if not 0 <= (cfg.speaker_id or 0) < max(n_spk, 1):
                    raise ValueError(f"speaker_id {cfg.speaker_id or 0} is out of range [0, {max(n_spk, 1)})")
            sid = np.full((len(all_ids),), cfg.speaker_id or 0, np.int64) if "sid" in expected else None
            norm = 0 if not cfg.normalize_audio else (2 if normalize_scope == "text" else 1)
            segs = [Segment(b, 0, lead, norm, float(cfg.volume)) for b in range(len(all_ids))]
            more = {} if trim is None else {"trim": trim}
            if level is not None:
                more["levels"] = level
            if shape is not None:
                more["shapes"] = shape
            if token_db is not None:
                more["token_gain_db"], more["gain_ramp"] = self._padded_db(token_db), _GAIN_RAMP
            if limit is not None:  # (passed down only when asked for: sessions from before the limiter do not know the keyword)
                more["limits"] = limit
            if token_st is not None:
                more["token_semitones"] = self._padded_db(token_st)
            if token_st_end is not None:
                more["token_semitones_end"] = self._padded_db(token_st_end)
            if fit is not None:
                more["fit"] = fit
            out = self.session.synthesize_delivered(ids, lens, self._scales(cfg), sid, segments=segs, n_streams=1,
                                                    encoding=encoding, return_durations=want_dur, **more)
            data = out["streams"][0]
            counts = [int(n) for n in out["sample_lengths"]]
            if fit is not None:
                fit_scale, fit_status = float(out["fit_scale"][0]), int(out["fit_status"][0])
            if token_st is not None and want_dur:
                spans = out["token_spans"]
            if trim is not None:
                kept = [(int(a), int(c)) for a, c in zip(out["kept_first"], out["kept_count"])]
            if level is not None:
                loud, gains = [float(v) for v in out["loudness"]], [float(v) for v in out["gain"]]
            if want_dur:
                durs, frames = out["durations"], [int(f) for f in out["y_lengths"]]
        else:
            need_dur = want_dur or token_db is not None
            if hasattr(self.session, "synthesize_batch"):
                res = self.phoneme_ids_batch_to_audio(all_ids, cfg, return_durations=need_dur)
                audios, durs = res if need_dur else (res, None)
            else:
                audios = [self.phoneme_ids_to_audio(ids, cfg) for ids in all_ids]
            counts = [len(np.atleast_1d(a)) for a in audios]
            norm = 0 if not cfg.normalize_audio else (2 if normalize_scope == "text" else 1)
            # (without fades and gains: exactly the calls made before there were any)
            more = {} if shape is None and token_db is None else {"shapes": self._row_shapes(shape, token_db, durs, counts)}
            if limit is not None:
                more["limits"] = limit
            if level is not None:
                data, cut, loud, gains = ae.join_leveled([np.atleast_1d(a) for a in audios], self.sample_rate, level, encoding, lead,
                                                         tail, trim, cfg.volume, **more)
                gains = [float(g) for g in gains]
            else:
                data, cut = ae.join_trimmed([np.atleast_1d(a) for a in audios], encoding, lead, tail, trim, norm, cfg.volume, **more)
            kept = cut if trim is not None else None
        valid = counts
        if kept is not None:
            counts = [c for _, c in kept]
        starts, pos = [], 0
        for n in counts:
            starts.append(pos + lead)
            pos += lead + n + tail
        aligned = None
        if want_dur:
            hop, ratio = self.session.hparam("hop"), self._ratio()
            aligned = []
            for b, g in enumerate(groups):
                total = frames[b] if frames is not None else max(1, int(np.sum(durs[b])))
                if spans is not None:  # (a warped sentence: its phonemes lie where the warp put them)
                    al = build_span_alignments(g, spans[b], valid[b])
                else:
                    al = build_alignments(g, durs[b], hop, total_frames=total, ratio=ratio)
                if kept is not None:
                    self._cut_alignments(al, *kept[b])
                for a in al:
                    a.start_sample += starts[b]
                aligned.append(al)
        return ae.EncodedAudio(data, encoding, self.sample_rate, starts, counts, aligned, loud, gains, fit_scale, fit_status)

    def stream_encoded(self, text: str, syn_config: Optional[SynthesisConfig] = None, encoding: str = "pcm16",
                       chunk_frames: int = 64, sentence_silence: float = 0.0, ref_peak=None, fade_in: float = 0.0,
                       fade_out: float = 0.0, fade_curve: str = "linear", phoneme_gain_db=None, limit_ceiling: float = 0.0,
                       limit_lookahead: float = 0.005, trim_silence=None, phoneme_pitch=None, pitch_contour=None,
                       duration: Optional[float] = None, duration_mode: str = "exact"):
        """Extension: synthesize_encoded's ONE stream as a generator of `bytes`, handed out while the audio still renders.
        All sentences render as one chunked batch (MiSession.synthesize_stream_encoded: post-processing, encoding and the
        masking to each sentence's own length happen on the device, per chunk).  Sentence 0's chunks are yielded as they
        arrive, behind its pause; the later sentences' bytes are kept on the host and yielded - each behind its pause - once
        their predecessor is complete.  Joined, the pieces are synthesize_encoded(...).data.tobytes() for the same audio.
        A stream cannot know its own peak: syn_config.normalize_audio needs `ref_peak` (a float, or one per sentence - the
        peak each sentence is normalised by, e.g. the final EncodedChunk.peak of an earlier stream with the same seeds) and
        raises ValueError without one; with normalize_audio off, ref_peak is not used.  volume is the config's.  A session
        without synthesize_stream_encoded gets the same bytes from the host encoder: over synthesize_stream's chunks where
        that exists, else over the whole rendering.
        fade_in / fade_out / fade_curve, phoneme_gain_db and limit_ceiling / limit_lookahead have the meanings and refusals of
        synthesize_encoded, for every sentence (vitsmi.h, "shaped streaming"): a streamed sentence meets the silence of its
        pause at exactly 0, takes a volume per phoneme and ducks under its peaks instead of clipping - joined, still
        synthesize_encoded's bytes.  With a limiter every chunk arrives limit_lookahead of audio later.  They are passed
        down only when asked for; a session that streams fp32 only takes audio_encoding.stream_shaped.
        trim_silence (None; a float: the threshold as a fraction of the sentence's ref_peak - it needs normalize_audio and
        ref_peak; or a session.Onset with keep_lead in seconds) cuts the LEADING silence of every sentence on the device
        (vitsmi.h, "trimmed streaming"): every sentence is yielded from its onset on, behind its pause, and its fade-in and
        limiter start there.  A stream keeps as much of keep_lead as it has not handed over yet: with keep_lead <=
        limit_lookahead, or an onset within the first chunk, the bytes are synthesize_encoded's under the same leading trim.
        The trailing silence stays: a stream learns where its audio ends only at the end.
        phoneme_pitch and pitch_contour have the meanings and refusals of synthesize_encoded, for every sentence (vitsmi.h,
        "streamed pitch"): the sentences are warped and glided piece by piece on the device - joined, still
        synthesize_encoded's bytes.  They need a session whose synthesize_stream_encoded takes token_semitones /
        token_semitones_end (ValueError otherwise: such a session's chunked entries have no warped form) and are refused with
        an output rate set unless the voice has pitch_at_rate, as in synthesize_encoded.
        duration / duration_mode have the meanings and refusals of synthesize_encoded (vitsmi.h, "fitted durations"): the
        duration is that of the rendered audio with its pauses, before trim_silence - joined, still synthesize_encoded's bytes.
        They need a session whose synthesize_stream_encoded takes fit= (ValueError otherwise)."""
        import inspect
        from . import audio_encoding as ae
        fn = getattr(self.session, "synthesize_stream_encoded", None)
        takes = inspect.signature(fn).parameters if fn is not None else {}
        if pitch_contour is not None:
            if "token_semitones_end" not in takes:
                raise ValueError("pitch_contour is not covered by stream_encoded: the chunked entries have no warped form "
                                 "(synthesize_encoded takes it)")
            if self._ratio() is not None and not self.pitch_at_rate:
                raise ValueError("pitch_contour is not covered with an output rate set")
            if self.pitch_at_rate:
                self._rate_admitted("pitch_contour")
        if phoneme_pitch is not None:
            if "token_semitones" not in takes:
                raise ValueError("phoneme_pitch is not covered by stream_encoded: the chunked entries have no warped form "
                                 "(synthesize_encoded takes it)")
            if self._ratio() is not None and not self.pitch_at_rate:
                raise ValueError("phoneme_pitch is not covered with an output rate set")
            if self.pitch_at_rate:
                self._rate_admitted("phoneme_pitch")
        cfg = syn_config if syn_config is not None else SynthesisConfig()
        ae._check(encoding)
        lead = self._lead_samples(sentence_silence)
        shape = self._shape(fade_in, fade_out, fade_curve)
        limit = self._limit(limit_ceiling, limit_lookahead)
        onset = self._onset(trim_silence, cfg, ref_peak)
        if phoneme_gain_db is not None and not hasattr(self.session, "synthesize_batch"):
            raise ValueError("phoneme_gain_db needs a session that reports durations (synthesize_batch)")
        if cfg.normalize_audio and ref_peak is None:
            raise ValueError("a stream cannot know its own peak: pass ref_peak (the peak to normalise by), or switch "
                             "normalize_audio off")
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames must be >= 1 (got {chunk_frames})")
        if duration is not None:  # (what does not depend on the text is refused by the call itself)
            self._duration_fit(duration, duration_mode, 1, 0, "synthesize_stream_encoded", phoneme_pitch is not None or pitch_contour is not None)
        return self._stream_encoded(text, cfg, encoding, int(chunk_frames), lead, ref_peak, shape, phoneme_gain_db, limit, onset,
                                    phoneme_pitch, pitch_contour, duration, duration_mode)

    def _onset(self, trim_silence, cfg, ref_peak):
        """trim_silence of stream_encoded -> a session.Onset in samples at the delivered rate, or None.  A float is a threshold
        relative to the sentence's ref_peak (mode 2); an Onset is taken with keep_lead in SECONDS, converted like the pause."""
        from .session import Onset
        if trim_silence is None:
            return None
        if isinstance(trim_silence, Onset):
            o = trim_silence
            if not o.keep_lead >= 0:
                raise ValueError(f"trim_silence: keep_lead must be >= 0 seconds (got {o.keep_lead})")
            o = Onset(int(o.mode), float(o.threshold), self._lead_samples(o.keep_lead))
        else:
            thr = float(trim_silence)
            o = Onset(2, thr, 0)
        if not (o.threshold >= 0.0 and np.isfinite(o.threshold)):
            raise ValueError(f"trim_silence must be a finite threshold >= 0 (got {o.threshold})")
        if o.mode == 2 and (not cfg.normalize_audio or ref_peak is None):
            raise ValueError("trim_silence relative to the peak needs normalize_audio and ref_peak (a stream cannot know its own "
                             "peak): pass them, or an absolute threshold as Onset(1, threshold)")
        return o if o.mode else None

    def _stream_encoded(self, text, cfg, encoding, chunk_frames, lead, ref_peak, shape=None, phoneme_gain_db=None, limit=None,
                        onset=None, phoneme_pitch=None, pitch_contour=None, duration=None, duration_mode="exact"):
        from . import audio_encoding as ae
        from .sharding import pad_batch
        token_db = token_st = token_st_end = None
        pitched = phoneme_pitch is not None or pitch_contour is not None
        if phoneme_gain_db is not None or pitched:
            groups = self._sentence_groups(text, cfg)
            all_ids = [[i for _, ids in g for i in ids] for g in groups]
            if phoneme_gain_db is not None:
                token_db = [self._group_db(phoneme_gain_db, k, g) for k, g in enumerate(groups)]
            if pitched:
                pairs = [self._sentence_semitones(phoneme_pitch, pitch_contour, k, g) for k, g in enumerate(groups)]
                token_st = [a for a, _ in pairs]
                token_st_end = None if pitch_contour is None else [b for _, b in pairs]
        else:
            all_ids = self._sentence_ids(text, cfg)
        B = len(all_ids)
        if not B:
            return
        fit = self._duration_fit(duration, duration_mode, B, B * lead, "synthesize_stream_encoded", pitched)
        shaped = shape is not None or token_db is not None or limit is not None or onset is not None
        peaks = None
        if cfg.normalize_audio:
            peaks = np.asarray(ref_peak, np.float32)
            if peaks.shape not in ((), (B,)):
                raise ValueError(f"ref_peak must be a float or one per sentence ({B}), got shape {peaks.shape}")
            peaks = np.ascontiguousarray(np.broadcast_to(peaks, (B,)))
        volume = float(cfg.volume)
        pause = ae.silence(lead, encoding).tobytes()
        session = self.session

        def host_bytes(b, audio):
            return ae.encode(self._scaled(audio, None if peaks is None else peaks[b], volume), encoding).tobytes()

        streams = hasattr(session, "synthesize_stream_encoded") or hasattr(session, "synthesize_stream")
        if not streams:  # the whole rendering, sentence by sentence through the host encoder
            durs = None
            if hasattr(session, "synthesize_batch"):
                res = self.phoneme_ids_batch_to_audio(all_ids, cfg, return_durations=token_db is not None)
                audios, durs = res if token_db is not None else (res, None)
            else:
                audios = (self.phoneme_ids_to_audio(ids, cfg) for ids in all_ids)
            if not shaped:
                for b, a in enumerate(audios):
                    yield pause + host_bytes(b, np.atleast_1d(a))
                return
            audios = [np.atleast_1d(a) for a in audios]
            shapes = self._row_shapes(shape, token_db, durs, [len(a) for a in audios])
            for b, a in enumerate(audios):
                a0 = 0
                if onset is not None:  # (one piece: a = max(0, f - keep_lead); no onset: nothing is kept)
                    hit = np.flatnonzero(np.abs(a) > ae.onset_threshold(onset, None if peaks is None else peaks[b]))
                    a0 = max(int(hit[0]) - onset.keep_lead, 0) if hit.size else len(a)
                mul = ae.shape_multiplier(a0, len(a) - a0, shapes[b])
                yield pause + ae.encode(ae.scaled(a[a0:], None if peaks is None else peaks[b], volume, mul, limit), encoding).tobytes()
            return
        ids, lens = pad_batch(all_ids)
        expected = [i.name for i in session.get_inputs()]
        if "sid" in expected:  # (checked before anything runs, as synthesize_encoded does)
            n_spk = int(session.hparam("n_speakers")) if hasattr(session, "hparam") else self.config.num_speakers
            if not 0 <= (cfg.speaker_id or 0) < max(n_spk, 1):
                raise ValueError(f"speaker_id {cfg.speaker_id or 0} is out of range [0, {max(n_spk, 1)})")
        sid = np.full((B,), cfg.speaker_id or 0, np.int64) if "sid" in expected else None
        if hasattr(session, "synthesize_stream_encoded"):
            more = {}   # (passed down only when asked for: sessions from before the shaped stream do not know the keywords)
            if shape is not None:
                more["shapes"] = shape
            if token_db is not None:
                more["token_gain_db"], more["gain_ramp"] = self._padded_db(token_db), _GAIN_RAMP
            if limit is not None:
                more["limit"] = limit
            if onset is not None:
                more["onsets"] = onset
            if token_st is not None:
                more["token_semitones"] = self._padded_db(token_st)
            if token_st_end is not None:
                more["token_semitones_end"] = self._padded_db(token_st_end)
            if fit is not None:
                more["fit"] = fit

            def skipped(c, b):  # (a stream that is not trimmed has nothing to skip)
                skip = getattr(c, "skip", None)
                return 0 if skip is None else int(skip[b])

            chunks = ((c.first_sample, c.data.shape[1], c.total_samples, c.valid,
                       [c.data[b, skipped(c, b):int(c.valid[b])].tobytes() for b in range(B)])
                      for c in session.synthesize_stream_encoded(ids, lens, self._scales(cfg), sid, chunk_frames=chunk_frames,
                                                                 encoding=encoding, ref_peak=peaks, volume=volume, **more))
        elif shaped:
            if token_db is not None and not hasattr(session, "last_durations"):
                raise ValueError("phoneme_gain_db needs a session that reports durations (last_durations)")

            def sample_counts():
                return (np.asarray(session.last_sample_counts(), np.int64) if hasattr(session, "last_sample_counts")
                        else np.asarray(session.last_y_lengths(), np.int64) * session.hparam("hop"))

            def row_shapes(counts):  # (counts and durations are known from the first chunk on: stream_shaped asks there)
                durs = None if token_db is None else np.asarray(session.last_durations())
                return self._row_shapes(shape, token_db, durs, [int(c) for c in counts])

            def shaped_chunks():
                fp32 = session.synthesize_stream(ids, lens, self._scales(cfg), sid, chunk_frames=chunk_frames)
                for first, data, valid, _, total, *skip in ae.stream_shaped(fp32, sample_counts, encoding, peaks, volume, row_shapes, limit,
                                                                            onset):
                    lo = skip[0] if skip else np.zeros(B, np.int32)
                    yield first, data.shape[1], total, valid, [data[b, int(lo[b]):int(valid[b])].tobytes() for b in range(B)]
            chunks = shaped_chunks()
        else:
            def host_chunks():
                counts = None
                for first, x, total in session.synthesize_stream(ids, lens, self._scales(cfg), sid, chunk_frames=chunk_frames):
                    if counts is None:  # (known from the first chunk on)
                        counts = (np.asarray(session.last_sample_counts(), np.int64) if hasattr(session, "last_sample_counts")
                                  else np.asarray(session.last_y_lengths(), np.int64) * session.hparam("hop"))
                    n = x.shape[1]
                    valid = np.clip(counts - first, 0, n)
                    yield first, n, total, valid, [host_bytes(b, x[b, :int(valid[b])]) for b in range(B)]
            chunks = host_chunks()
        cur, kept = 0, [[] for _ in range(B)]
        if pause:
            yield pause
        for first, n, total, valid, rows in chunks:
            if rows[cur]:
                yield rows[cur]
            for b in range(cur + 1, B):
                kept[b].append(rows[b])
            # a sentence is complete once a chunk holds less of it than the chunk is long, or the stream ends
            while cur + 1 < B and (int(valid[cur]) < n or first + n >= total):
                cur += 1
                yield pause + b"".join(kept[cur])
                kept[cur] = []
        for b in range(cur + 1, B):  # (a stream that ended early: what was kept still goes out in order)
            yield pause + b"".join(kept[b])

    def synthesize_requests_encoded(self, requests: Sequence[Tuple[str, Optional[SynthesisConfig]]],
                                    seeds: Optional[Sequence[int]] = None, max_batch: int = 32, encoding: str = "pcm16",
                                    sentence_silence: float = 0.0, alignments: bool = False, trim_silence=None,
                                    trailing_silence: float = 0.0, loudness=None, loudness_scope: str = "sentence",
                                    peak_ceiling: float = 0.0, max_gain_db: float = 30.0, fade_in: float = 0.0,
                                    fade_out: float = 0.0, fade_curve: str = "linear", phoneme_gain_db=None,
                                    limit_ceiling: float = 0.0, limit_lookahead: float = 0.005,
                                    output_sample_rates: Optional[Sequence[Optional[int]]] = None,
                                    encodings: Optional[Sequence[Optional[str]]] = None, phoneme_pitch=None,
                                    pitch_contour=None):
        """Extension: synthesize_requests with every request's audio returned as one stream of encoded audio
        (audio_encoding.EncodedAudio; the pause of synthesize_encoded in front of each sentence).  The batching is
        synthesize_requests': sentences sorted by length, max_batch at a time, each with its request's settings and seed.
        With a session that delivers, every sentence leaves the device as its own encoded stream, post-processed with its
        request's normalize_audio / volume; a request's pieces are joined with their silence on the host, because its
        sentences may render in different runs (for the same reason each sentence is normalised by its own peak).  Any other
        session: the host encoder over synthesize_requests' chunks - the same bytes.  trim_silence / trailing_silence as in
        synthesize_encoded: every sentence cut to its kept range (normalised by the peak of what is kept) and followed by
        its trailing silence.  loudness / loudness_scope / peak_ceiling / max_gain_db as in synthesize_encoded, per request
        ("text": the request's sentences pooled); every request's config must say normalize_audio=False.  With scope
        "sentence" a session that delivers measures and levels on the device.  With scope "text" a request's sentences may
        render in different runs, so the device delivers them cut but unlevelled as float32 and the host levels them
        (audio_encoding.level_rows).  fade_in / fade_out / fade_curve / phoneme_gain_db as in synthesize_encoded, for every
        sentence of every request (phoneme_gain_db's sentence_index counts within its request); with loudness scope "text"
        the host that levels applies them too (audio_encoding.shape_multiplier).  limit_ceiling / limit_lookahead as in
        synthesize_encoded, for every sentence of every request (where the host levels, it limits too).
        output_sample_rates / encodings: None, or one value per request (None in the list: this voice's rate / `encoding`) -
        request r's audio at its own rate and in its own encoding, out of the same batched runs: the batching does not look
        at either, each row of a run is resampled on the device at its request's rate (MiSession.set_output_rates) and each
        run is delivered once per (rate, encoding) group.  Every seconds-valued argument - sentence_silence,
        trailing_silence, a Trim's keep_lead / keep_tail, the fades, limit_lookahead - is converted at each request's own rate,
        alignments count samples at it, and every EncodedAudio carries its request's sample_rate and encoding: request r is
        what this call returns for it on a voice loaded at that rate with that encoding, bit for bit.  ValueError with a
        session that has no set_output_rates.
        phoneme_pitch as in synthesize_encoded, for every sentence of every request (a callable's sentence_index counts within
        its request); ValueError with a session that does not warp, and together with an output rate of the voice or of a request.
        pitch_contour as in synthesize_encoded, applied to every sentence of every request, with phoneme_pitch's refusals."""
        from . import audio_encoding as ae
        ae._check(encoding)
        self._pitch_check(phoneme_pitch, [r for r in output_sample_rates or () if r is not None])
        self._contour_check(pitch_contour, [r for r in output_sample_rates or () if r is not None])
        pitched = phoneme_pitch is not None or pitch_contour is not None
        lead = self._lead_samples(sentence_silence)
        trim = self._trim(trim_silence, trailing_silence)
        shape = self._shape(fade_in, fade_out, fade_curve)
        shaped = shape is not None or phoneme_gain_db is not None
        limit = self._limit(limit_ceiling, limit_lookahead)
        level = self._level(loudness, loudness_scope, peak_ceiling, max_gain_db,
                            [cfg if cfg is not None else SynthesisConfig() for _, cfg in requests])
        # what a request's audio is delivered as: (rate, encoding, lead, trim, shape, limit) - this voice's for every request,
        # or with a rate or an encoding per request the same things at that request's own
        R = len(requests)
        mixed = output_sample_rates is not None or encodings is not None
        as_of = [(self.sample_rate, encoding, lead, trim, shape, limit)] * R
        if mixed:
            if not (hasattr(self.session, "set_output_rates") and hasattr(self.session, "synthesize_delivered")):
                raise ValueError("output_sample_rates / encodings need a session that resamples each row of a run on the device "
                                 "(MiSession.set_output_rates); this session has no set_output_rates")
            for name, v in (("output_sample_rates", output_sample_rates), ("encodings", encodings)):
                if v is not None and len(v) != R:
                    raise ValueError(f"{name} must hold one value per request ({R}), got {len(v)}")
            made = {}
            as_of = []
            for r in range(R):
                fo = output_sample_rates[r] if output_sample_rates is not None else None
                enc = encodings[r] if encodings is not None and encodings[r] is not None else encoding
                if fo is not None and (not isinstance(fo, (int, np.integer)) or fo <= 0):
                    raise ValueError(f"request {r}: output_sample_rates must hold None or positive integers (got {fo!r})")
                fo = self.sample_rate if fo is None else int(fo)
                ae._check(enc)
                if fo not in made:
                    made[fo] = (self._lead_samples(sentence_silence, fo), self._trim(trim_silence, trailing_silence, fo),
                                self._shape(fade_in, fade_out, fade_curve, fo), self._limit(limit_ceiling, limit_lookahead, fo))
                as_of.append((fo, enc) + made[fo])
            shaped = phoneme_gain_db is not None or any(a[4] is not None for a in as_of)
            # (below, "is there a trim / a shape / a limit" asks whether any request has one)
            trim = next((a[3] for a in as_of if a[3] is not None), None)
            shape = next((a[4] for a in as_of if a[4] is not None), None)
            limit = next((a[5] for a in as_of if a[5] is not None), None)

        def join(r, pieces, aligns, kept=None, loud=None, gains=None):
            rate, encoding, lead, trim = as_of[r][:4]
            tail = trim.tail_samples if trim is not None else 0
            starts, pos = [], 0
            for p in pieces:
                starts.append(pos + lead)
                pos += lead + len(p) + tail
            parts = [q for p in pieces for q in ((ae.silence(lead, encoding), p, ae.silence(tail, encoding)) if tail else
                                                 (ae.silence(lead, encoding), p))]
            data = np.concatenate(parts) if parts else ae.silence(0, encoding)
            if aligns is not None:
                for k, (st, al) in enumerate(zip(starts, aligns)):
                    if kept is not None:
                        self._cut_alignments(al or [], *kept[k])
                    for a in al or []:
                        a.start_sample += st
            return ae.EncodedAudio(data, encoding, rate, starts, [len(p) for p in pieces], aligns,
                                   None if loud is None else [float(v) for v in loud], None if gains is None else [float(g) for g in gains])

        def level_on_host(r, rows, volume, muls=None):
            """request r's kept rows (float32, unlevelled) -> (encoded pieces, loudness, gains); muls: their shapes' multipliers"""
            rate, encoding, limit = as_of[r][0], as_of[r][1], as_of[r][5]
            loud, gains = ae.level_rows(rows, rate, level)
            muls = muls if muls is not None else [None] * len(rows)
            return [ae.encode(ae.leveled(v, g, volume, m, limit), encoding) for v, g, m in zip(rows, gains, muls)], loud, gains

        def request_db(r, text, cfg):
            """the dB per phoneme id of every sentence of request r, or None"""
            if phoneme_gain_db is None:
                return None
            return [self._group_db(phoneme_gain_db, k, g) for k, g in enumerate(self._sentence_groups(text, cfg))]

        if not hasattr(self.session, "synthesize_delivered"):
            want_al = lambda cs: alignments and all(c.phoneme_alignments is not None for c in cs)
            durs = {} if phoneme_gain_db is not None else None
            more = {} if durs is None else {"_durations": durs}

            def host_shapes(r, text, cfg, cs):
                """request r's shapes, one per sentence (None: nothing shapes)"""
                if not shaped:
                    return None
                db = request_db(r, text, cfg)
                return self._row_shapes(shape, db, None if db is None else [durs[r, k] for k in range(len(cs))],
                                        [len(c.audio_float_array) for c in cs])

            if level is not None:
                chunks = self.synthesize_requests(requests, seeds=seeds, max_batch=max_batch, alignments=alignments, postprocess=False,
                                                  **more)
                result = []
                for r, ((text, cfg), cs) in enumerate(zip(requests, chunks)):
                    cfg = cfg if cfg is not None else SynthesisConfig()
                    kept = [ae.trim_range(c.audio_float_array, len(c.audio_float_array), trim) for c in cs]
                    rows = [np.asarray(c.audio_float_array, np.float32)[a:a + n] for c, (a, n) in zip(cs, kept)]
                    shapes = host_shapes(r, text, cfg, cs)
                    muls = None if shapes is None else [ae.shape_multiplier(a, n, sh) for (a, n), sh in zip(kept, shapes)]
                    pieces, loud, gains = level_on_host(r, rows, cfg.volume, muls)
                    result.append(join(r, pieces, [c.phoneme_alignments for c in cs] if want_al(cs) else None,
                                       kept if trim is not None else None, loud, gains))
                return result
            if shaped or limit is not None:
                # the rows as rendered, each cut (or whole), shaped and limited in front of the clip
                chunks = self.synthesize_requests(requests, seeds=seeds, max_batch=max_batch, alignments=alignments, postprocess=False,
                                                  **more)
                result = []
                for r, ((text, cfg), cs) in enumerate(zip(requests, chunks)):
                    cfg = cfg if cfg is not None else SynthesisConfig()
                    shapes = host_shapes(r, text, cfg, cs) or [None] * len(cs)
                    pieces, kept = [], []
                    for c, sh in zip(cs, shapes):
                        data, k = ae.join_trimmed([c.audio_float_array], encoding, 0, 0, trim, 1 if cfg.normalize_audio else 0,
                                                  cfg.volume, shapes=None if sh is None else [sh], limits=limit)
                        pieces.append(data)
                        kept += k
                    result.append(join(r, pieces, [c.phoneme_alignments for c in cs] if want_al(cs) else None,
                                       kept if trim is not None else None))
                return result
            if trim is None:
                chunks = self.synthesize_requests(requests, seeds=seeds, max_batch=max_batch, alignments=alignments)
                return [join(r, [ae.encode(c.audio_float_array, encoding) for c in cs],
                             [c.phoneme_alignments for c in cs] if want_al(cs) else None) for r, cs in enumerate(chunks)]
            # the rows as rendered, each cut, then post-processed by the peak of what is kept
            chunks = self.synthesize_requests(requests, seeds=seeds, max_batch=max_batch, alignments=alignments, postprocess=False)
            result = []
            for r, ((_, cfg), cs) in enumerate(zip(requests, chunks)):
                cfg = cfg if cfg is not None else SynthesisConfig()
                pieces, kept = [], []
                for c in cs:
                    data, k = ae.join_trimmed([c.audio_float_array], encoding, 0, 0, trim, 1 if cfg.normalize_audio else 0, cfg.volume)
                    pieces.append(data)
                    kept += k
                result.append(join(r, pieces, [c.phoneme_alignments for c in cs] if want_al(cs) else None, kept))
            return result
        if max_batch < 1:
            raise ValueError(f"max_batch must be >= 1 (got {max_batch})")
        if seeds is not None and len(seeds) != len(requests):
            raise ValueError(f"seeds must hold one seed per request ({len(requests)}), got {len(seeds)}")
        cfgs = [cfg if cfg is not None else SynthesisConfig() for _, cfg in requests]
        expected = [i.name for i in self.session.get_inputs()]
        if "sid" in expected:  # every request's speaker is checked before anything runs
            n_spk = int(self.session.hparam("n_speakers"))
            for r, cfg in enumerate(cfgs):
                spk = cfg.speaker_id or 0
                if not 0 <= spk < max(n_spk, 1):
                    raise ValueError(f"request {r}: speaker_id {spk} is out of range [0, {max(n_spk, 1)})")
        from .session import Segment, Shape, Trim
        from .sharding import pad_batch
        want_dur = alignments and hasattr(self.session, "last_durations")
        rows, groups, db_of, st_of = [], {}, {}, {}
        for r, ((text, _), cfg) in enumerate(zip(requests, cfgs)):
            if want_dur or phoneme_gain_db is not None or pitched:
                for k, g in enumerate(self._sentence_groups(text, cfg)):
                    groups[r, k] = g
                    rows.append((r, k, [i for _, ids in g for i in ids]))
                    if phoneme_gain_db is not None:
                        db_of[r, k] = self._group_db(phoneme_gain_db, k, g)
                    if pitched:
                        st_of[r, k] = self._sentence_semitones(phoneme_pitch, pitch_contour, k, g)
            else:
                rows.extend((r, k, ids) for k, ids in enumerate(self._sentence_ids(text, cfg)))
        piece, aligned, kept_of, level_of, mul_of = {}, {}, {}, {}, {}
        hop = self.session.hparam("hop")
        order = sorted(range(len(rows)), key=lambda i: len(rows[i][2]))  # (stable: equal lengths keep request order)
        for c0 in range(0, len(order), max_batch):
            run = [rows[i] for i in order[c0:c0 + max_batch]]
            ids, lens = pad_batch([ids for _, _, ids in run])
            scales = np.stack([self._scales(cfgs[r]) for r, _, _ in run])
            sid = np.asarray([cfgs[r].speaker_id or 0 for r, _, _ in run], np.int64) if "sid" in expected else None
            row_seeds = None if seeds is None else np.asarray([sentence_seed(seeds[r], k) for r, k, _ in run], np.uint64)
            host_level = level is not None and level.mode == 2
            segs = [Segment(b, b, 0, 1 if cfgs[r].normalize_audio else 0, 1.0 if host_level else float(cfgs[r].volume))
                    for b, (r, _, _) in enumerate(run)]
            # (the tail is joined on the host like the pause: the device delivers each sentence's kept range alone)
            more = {} if trim is None else {"trim": dataclasses.replace(trim, tail_samples=0)}
            if level is not None and not host_level:
                more["levels"] = level
            # (scope "text": the host levels the float32 rows and shapes them there - the shape comes behind the gain)
            if shaped and not host_level:
                if shape is not None:
                    more["shapes"] = shape
                if phoneme_gain_db is not None:
                    more["token_gain_db"], more["gain_ramp"] = self._padded_db([db_of[r, k] for r, k, _ in run]), _GAIN_RAMP
            if limit is not None and not host_level:  # (scope "text": the host that levels limits too)
                more["limits"] = limit
            need_dur = want_dur or (host_level and phoneme_gain_db is not None)
            if pitched:
                more["token_semitones"] = self._padded_db([st_of[r, k][0] for r, k, _ in run])
            if pitch_contour is not None:
                more["token_semitones_end"] = self._padded_db([st_of[r, k][1] for r, k, _ in run])
            if mixed:
                # a rate and an encoding per row: the same call with its request's own things in every list (a request whose
                # trim or shape comes to nothing at its rate: the neutral one)
                of_row = [as_of[r] for r, _, _ in run]
                if "trim" in more:
                    more["trim"] = [dataclasses.replace(a[3], tail_samples=0) if a[3] is not None else Trim(0, 0.0, 0, 0, 0) for a in of_row]
                if "shapes" in more:
                    more["shapes"] = [a[4] if a[4] is not None else Shape() for a in of_row]
                if "limits" in more:
                    more["limits"] = [a[5] for a in of_row]
                native = int(self.config.sample_rate)
                out = self._delivered_at_row_rates([0 if a[0] == native else a[0] for a in of_row], ids, lens, scales, sid,
                                                   segments=segs, n_streams=len(run),
                                                   encoding=["f32" if host_level else a[1] for a in of_row], seeds=row_seeds,
                                                   return_durations=need_dur, **more)
            else:
                out = self.session.synthesize_delivered(ids, lens, scales, sid, segments=segs, n_streams=len(run),
                                                        encoding="f32" if host_level else encoding, seeds=row_seeds,
                                                        return_durations=need_dur, **more)
            if shaped and host_level:
                counts = [int(n) for n in out["sample_lengths"]]
                run_shapes = self._row_shapes([as_of[r][4] for r, _, _ in run] if mixed else shape,
                                              None if phoneme_gain_db is None else [db_of[r, k] for r, k, _ in run],
                                              None if phoneme_gain_db is None else [out["durations"][b, :len(i)] for b, (_, _, i) in enumerate(run)],
                                              counts, [as_of[r][0] for r, _, _ in run] if mixed else None,
                                              out["token_spans"] if pitched and phoneme_gain_db is not None else None)
                for b, (r, k, _) in enumerate(run):
                    a, c = (int(out["kept_first"][b]), int(out["kept_count"][b]))
                    mul_of[r, k] = ae.shape_multiplier(a, c, run_shapes[b])
            for b, (r, k, _) in enumerate(run):
                piece[r, k] = out["streams"][b]
                if level is not None and not host_level:
                    level_of[r, k] = (float(out["loudness"][b]), float(out["gain"][b]))
                if trim is not None:
                    kept_of[r, k] = (int(out["kept_first"][b]), int(out["kept_count"][b]))
                if want_dur and pitched:
                    aligned[r, k] = build_span_alignments(groups[r, k], out["token_spans"][b], int(out["sample_lengths"][b]))
                elif want_dur:
                    aligned[r, k] = build_alignments(groups[r, k], out["durations"][b], hop,
                                                     total_frames=int(out["y_lengths"][b]), ratio=self._ratio(as_of[r][0]))
        per_request = [[] for _ in requests]
        for r, k, _ in rows:  # (rows are in request, then sentence order)
            per_request[r].append((r, k))
        result = []
        for r, keys in enumerate(per_request):
            pieces, loud, gains = [piece[key] for key in keys], None, None
            if level is not None and level.mode == 2:
                pieces, loud, gains = level_on_host(r, pieces, cfgs[r].volume, [mul_of[key] for key in keys] if shaped else None)
            elif level is not None:
                loud, gains = [level_of[key][0] for key in keys], [level_of[key][1] for key in keys]
            result.append(join(r, pieces, [aligned[key] for key in keys] if want_dur else None,
                               [kept_of[key] for key in keys] if trim is not None else None, loud, gains))
        return result

    def _delivered_at_row_rates(self, rates, *args, **kw):
        """session.synthesize_delivered with row b resampled from the voice's rate to rates[b] (0: not at all); the session's
        own output rate, or rates, are put back afterwards"""
        s = self.session
        before = (s.output_rate, s.output_rates, s.input_rate)
        s.set_output_rates(rates, int(self.config.sample_rate))
        try:
            return s.synthesize_delivered(*args, **kw)
        finally:
            if before[1] is not None:
                s.set_output_rates(before[1], before[2])
            else:
                s.set_output_rate(before[0], before[2])

    def synthesize_wav(self, text: str, wav_file: wave.Wave_write, syn_config: Optional[SynthesisConfig] = None,
                       set_wav_format: bool = True, batch_sentences: bool = False, device_pcm16: bool = False) -> None:
        """Synthesize and write 16-bit PCM frames (voice.py:291-326).  `device_pcm16=True` (extension):
        all sentences in one batch, peak-normalise / volume / clip / int16 on the GPU, only PCM bytes cross PCIe;
        the frames written are bit-identical to the default path's."""
        if device_pcm16 and hasattr(self.session, "synthesize_batch_pcm16"):
            return self._synthesize_wav_device_pcm16(text, wav_file, syn_config or SynthesisConfig(), set_wav_format)
        sentence_silence = 0.0  # seconds of silence after each sentence (fixed in the reference)
        silence = bytes(int(self.sample_rate * sentence_silence * 2))
        first = True
        for chunk in self.synthesize(text, syn_config=syn_config, batch_sentences=batch_sentences):
            if first:
                if set_wav_format:
                    wav_file.setframerate(chunk.sample_rate)
                    wav_file.setsampwidth(chunk.sample_width)
                    wav_file.setnchannels(chunk.sample_channels)
                first = False
            # NOTE (mirrors voice.py:317-324): `first` was cleared just above, so the "silence between sentences" is also
            # written before the first one; it is zero bytes long today (sentence_silence = 0.0), which is the only
            # reason this is inaudible.  Kept for byte-identity with the reference (tests/golden/frontend.json).
            if not first:
                wav_file.writeframes(silence)
            wav_file.writeframes(chunk.audio_int16_bytes)

    def _synthesize_wav_device_pcm16(self, text: str, wav_file: wave.Wave_write, syn_config: SynthesisConfig,
                                     set_wav_format: bool) -> None:
        from .sharding import pad_batch
        if self.phonetic_spellings and syn_config.enable_phonetic_spellings:
            text = self.phonetic_spellings.apply(text)
        if syn_config.add_diacritics:
            text = self.phonemizer.add_diacritics(text, self.config.lang_code)
        all_ids = [self.phonemes_to_ids(p) for p in self.phonemize(text) if p]
        all_ids = [ids for ids in all_ids if ids]
        if set_wav_format:
            wav_file.setframerate(self.sample_rate)
            wav_file.setsampwidth(2)
            wav_file.setnchannels(1)
        if not all_ids:
            return
        ids, lens = pad_batch(all_ids)
        expected = [i.name for i in self.session.get_inputs()]
        sid = np.full((len(all_ids),), syn_config.speaker_id or 0, np.int64) if "sid" in expected else None
        pcm, ylen = self.session.synthesize_batch_pcm16(ids, lens, self._scales(syn_config), sid,
                                                        normalize=syn_config.normalize_audio, volume=syn_config.volume)
        # (with an output rate set the second value already counts samples at that rate: MiSession.synthesize_batch_pcm16)
        hop = 1 if self._ratio() is not None else self.session.hparam("hop")
        for b in range(len(all_ids)):
            wav_file.writeframes(pcm[b, :int(ylen[b]) * hop].tobytes())

    def _scales(self, syn_config: SynthesisConfig) -> np.ndarray:
        c = self.config
        length = c.length_scale if syn_config.length_scale is None else syn_config.length_scale
        noise = c.noise_scale if syn_config.noise_scale is None else syn_config.noise_scale
        noise_w = c.noise_w_scale if syn_config.noise_w_scale is None else syn_config.noise_w_scale
        return np.array([noise, length, noise_w], dtype=np.float32)

    def phoneme_ids_to_audio(self, phoneme_ids: List[int], syn_config: Optional[SynthesisConfig] = None) -> np.ndarray:
        """Raw (un-normalised) audio for one id sequence: the hot call (voice.py:328-379)."""
        if syn_config is None:
            syn_config = SynthesisConfig()
        expected = [i.name for i in self.session.get_inputs()]
        ids = np.expand_dims(np.array(phoneme_ids, dtype=np.int64), 0)
        feed = {"input": ids, "input_lengths": np.array([ids.shape[1]], dtype=np.int64)}
        if "scales" in expected:
            feed["scales"] = self._scales(syn_config)
        feed["langid"] = np.array([syn_config.lang_id or 0], dtype=np.int64)
        feed["sid"] = np.array([syn_config.speaker_id or 0], dtype=np.int64)
        feed = {k: v for k, v in feed.items() if k in expected}  # voices differ in their inputs
        return self.session.run(None, feed)[0].squeeze()

    def phoneme_ids_batch_to_audio(self, batch_ids: List[List[int]], syn_config: Optional[SynthesisConfig] = None,
                                   durations: Optional[Sequence[Sequence[int]]] = None,
                                   token_rate: Optional[Sequence[Sequence[float]]] = None,
                                   return_durations: bool = False):
        """Extension: all sequences in one padded batch; each waveform is trimmed to its own length
        (y_lengths * hop), since the generator also renders the padding (models.py:720).
        durations / token_rate: one sequence per utterance, as long as its ids - forced frames per id, or a multiplier on
        each id's predicted duration (MiSession.synthesize_batch); padded like the ids.  return_durations: returns
        (waveforms, [int64 array of frames per id, one per utterance]) instead of the waveforms alone."""
        if syn_config is None:
            syn_config = SynthesisConfig()
        from .sharding import pad_batch
        ids, lens = pad_batch(batch_ids)
        expected = [i.name for i in self.session.get_inputs()]
        sid = np.full((len(batch_ids),), syn_config.speaker_id or 0, np.int64) if "sid" in expected else None
        more = {}
        for name, seqs, dtype, fill in (("durations", durations, np.int64, 0), ("token_rate", token_rate, np.float32, 1.0)):
            if seqs is None:
                continue
            if len(seqs) != len(batch_ids) or any(len(q) != len(i) for q, i in zip(seqs, batch_ids)):
                raise ValueError(f"{name} must hold one value per phoneme id of every utterance")
            arr = np.full(ids.shape, fill, dtype)
            for b, q in enumerate(seqs):
                q = np.asarray(q)
                if name == "durations" and q.size and q.dtype.kind not in "iu":
                    raise ValueError(f"durations must be integers (frames per phoneme id), got {q.dtype}")
                arr[b, :len(q)] = q
            more[name] = arr
        if return_durations:
            more["return_durations"] = True
        out = self.session.synthesize_batch(ids, lens, self._scales(syn_config), sid, **more)
        hop = self.session.hparam("hop")
        valid = self._valid_samples(out, hop)
        audios = [out["output"][b, 0, 0, :int(valid[b])].copy() for b in range(len(batch_ids))]
        if return_durations:
            return audios, [out["durations"][b, :len(i)].copy() for b, i in enumerate(batch_ids)]
        return audios
