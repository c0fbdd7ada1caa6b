"""The encodings audio is delivered in - 16-bit PCM, G.711 mu-law and A-law, float32 - as NumPy code, and the container
they travel in.

`encode` is the host statement of the definition in include/vitsmi.h ("delivery"): what the engine computes on the device
for a session that can deliver (MiSession.deliver), computed here for one that cannot (the onnxruntime duck type, pipelined
and sharded sessions).  Both take the post-processed float32 samples in [-1, 1] (TTSVoice._postprocess) and give the same
bytes.  The two G.711 forms equal CPython's audioop.lin2ulaw / lin2alaw (width 2) on every int16 value.
"""
import io
import struct
import wave
from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np

ENCODINGS = ("pcm16", "ulaw", "alaw", "f32")   # in the order of the header's VITS_ENC_* codes (0 .. 3)
DTYPES = {"pcm16": np.int16, "ulaw": np.uint8, "alaw": np.uint8, "f32": np.float32}
# the encoding of sample value 0
SILENCE = {"pcm16": 0, "ulaw": 0xFF, "alaw": 0xD5, "f32": 0.0}
# WAVE format tags (mmreg.h): PCM, IEEE float, A-law, mu-law
_WAV_TAG = {"pcm16": 1, "f32": 3, "alaw": 6, "ulaw": 7}
_MAX_WAV_VALUE = 32767.0


def _check(encoding):
    if encoding not in ENCODINGS:
        raise ValueError(f"unknown encoding {encoding!r}: one of {ENCODINGS}")


def pcm16(samples: np.ndarray) -> np.ndarray:
    """float32 in [-1, 1] -> int16, as AudioChunk.audio_int16_array (phoonnx/voice.py:88-91)."""
    scaled = np.asarray(samples, np.float32) * np.float32(_MAX_WAV_VALUE)
    return np.clip(scaled, -_MAX_WAV_VALUE, _MAX_WAV_VALUE).astype(np.int16)


def _log2_floor(m: np.ndarray) -> np.ndarray:
    """floor(log2 m) of positive integers below 2^16, exactly (no floating point)"""
    r = np.zeros(m.shape, np.int32)
    for k in range(1, 16):
        r += (m >= (1 << k)).astype(np.int32)
    return r


def ulaw_from_pcm16(q: np.ndarray) -> np.ndarray:
    s = np.asarray(q, np.int16).astype(np.int32) >> 2
    neg = s < 0
    m = np.where(neg, -s, s) + 33
    seg = np.clip(_log2_floor(m) - 5, 0, 8)
    u = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
    return (u ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def alaw_from_pcm16(q: np.ndarray) -> np.ndarray:
    s = np.asarray(q, np.int16).astype(np.int32) >> 3
    neg = s < 0
    m = np.where(neg, -s - 1, s)
    seg = np.clip(_log2_floor(np.maximum(m, 1)) - 4, 0, 7)
    a = (seg << 4) | (np.where(seg < 2, m >> 1, m >> seg) & 15)
    return (a ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def encode(samples: np.ndarray, encoding: str = "pcm16") -> np.ndarray:
    """Post-processed float32 samples in [-1, 1] -> the elements of `encoding` (int16 / uint8 / float32)."""
    _check(encoding)
    samples = np.asarray(samples, np.float32)
    if encoding == "f32":
        return samples.copy()
    q = pcm16(samples)
    if encoding == "pcm16":
        return q
    return ulaw_from_pcm16(q) if encoding == "ulaw" else alaw_from_pcm16(q)


def silence(n: int, encoding: str = "pcm16") -> np.ndarray:
    """n elements of silence: the encoding of sample value 0"""
    _check(encoding)
    return np.full(int(n), SILENCE[encoding], DTYPES[encoding])


@dataclass
class EncodedAudio:
    """One stream of encoded audio: `data` holds the elements (int16 / uint8 / float32, one per sample), sentence k's audio
    is data[sentence_starts[k] : sentence_starts[k] + sentence_samples[k]] (what lies in front of it is its pause)."""
    data: np.ndarray
    encoding: str
    sample_rate: int
    sentence_starts: List[int]
    sentence_samples: List[int]
    # synthesize_encoded(..., alignments=True): per sentence, its PhonemeAlignment list with start_sample counted from the
    # beginning of `data`
    phoneme_alignments: Optional[List[List[Any]]] = None

    def tobytes(self) -> bytes:
        return np.ascontiguousarray(self.data).tobytes()

    def wav_bytes(self) -> bytes:
        """A RIFF/WAVE file of the stream.  PCM16: the bytes Python's `wave` module writes for these frames.  The others: an
        18-byte `fmt ` chunk (format tag 7 mu-law, 6 A-law, 3 float; cbSize 0) followed by a `fact` chunk with the sample
        count, as non-PCM formats require; a data chunk of odd length is padded to even."""
        _check(self.encoding)
        frames = self.tobytes()
        if self.encoding == "pcm16":
            out = io.BytesIO()
            with wave.open(out, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(int(self.sample_rate))
                w.writeframes(frames)
            return out.getvalue()
        align = np.dtype(DTYPES[self.encoding]).itemsize
        pad = len(frames) & 1
        fmt = struct.pack("<HHIIHHH", _WAV_TAG[self.encoding], 1, int(self.sample_rate), int(self.sample_rate) * align, align,
                          8 * align, 0)
        body = (b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, len(frames) // align) +
                b"data" + struct.pack("<I", len(frames)) + frames + b"\0" * pad)
        return b"RIFF" + struct.pack("<I", len(body)) + body
