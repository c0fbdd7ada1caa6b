"""The encodings audio is delivered in - 16-bit PCM, G.711 mu-law and A-law, float32 - as NumPy code, and the container
they travel in.

`encode` is the host statement of the definition in include/vitsmi.h ("delivery"): what the engine computes on the device
for a session that can deliver (MiSession.deliver), computed here for one that cannot (the onnxruntime duck type, pipelined
and sharded sessions).  Both take the post-processed float32 samples in [-1, 1] (TTSVoice._postprocess) and give the same
bytes.  The two G.711 forms equal CPython's audioop.lin2ulaw / lin2alaw (width 2) on every int16 value.

`trim_range` and `join_trimmed` are the same for the trimmed delivery (include/vitsmi.h, "trimmed delivery"): the kept range
of a row, and one stream of rows cut to their kept ranges with silence in front of and behind each.

`loudness`, `level_gain` and `join_leveled` are the same for the levelled delivery (include/vitsmi.h, "levelled delivery"), in
float64: the integrated loudness of ITU-R BS.1770-4 of a row, the gain that brings it to a target, and one stream of rows
levelled, encoded and joined.

`shape_multiplier` and the `shapes=` argument of the two joins are the same for the shaped delivery (include/vitsmi.h, "shaped
delivery"): fades and a breakpoint envelope as one float32 multiplier per kept sample, operation by operation as the device
computes it - the same bytes.

`limit_gains` and the `limits=` argument of the two joins are the same for the limited delivery (include/vitsmi.h, "limited
delivery"): the look-ahead peak limiter's gain per kept sample - integers up to one float32 division - and its product and
clamp in front of the clip: the same bytes.

`emit_range` and `stream_shaped` are the same for the shaped, limited encoded stream (include/vitsmi.h, "shaped streaming"):
the chunks of an fp32 stream shaped, limited across the chunk boundaries and encoded, on the engine's delayed timeline - the
same chunks.
"""
import io
import math
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


def trim_range(x, n, trim):
    """The kept range (a, c) of a row: x[:n] are its valid samples, `trim` anything with the fields of vits_trim - mode (0 off,
    1 absolute, 2 relative to the row's peak), threshold, keep_lead, keep_tail - or None (off).  A sample is active iff
    |x| > thr, strictly; no active sample: (0, 0)."""
    n = int(n)
    if trim is None or int(trim.mode) == 0:
        return 0, n
    if int(trim.mode) not in (1, 2):
        raise ValueError(f"trim mode {trim.mode} outside 0..2")
    mag = np.abs(np.asarray(x, np.float32)[:n])
    thr = np.float32(trim.threshold)
    if int(trim.mode) == 2:
        thr = np.float32(thr * (np.max(mag) if n else np.float32(0)))     # one float32 product
    active = np.flatnonzero(mag > thr)
    if active.size == 0:
        return 0, 0
    a = max(0, int(active[0]) - int(trim.keep_lead))
    e = min(n, int(active[-1]) + 1 + int(trim.keep_tail))
    return a, e - a


LIMIT_MAX_LOOKAHEAD = 1024


def limit_gains(u, ceiling, lookahead) -> np.ndarray:
    """The limiter's gain of every sample of one segment whose unlimited values are u (float32 [c]): the rule of
    include/vitsmi.h, "limited delivery" - q = floor(ceiling / |u| * 2^16) where |u| > ceiling, 2^16 elsewhere and outside the
    segment; M = the minimum of q over the next lookahead samples; S = the sum of M over the last lookahead + 1;
    g = float32(S) / float32((lookahead + 1) * 2^16).  Integers up to the division.  float32 [c]."""
    u = np.asarray(u, np.float32).ravel()
    c, L, ceil = u.size, int(lookahead), np.float32(ceiling)
    if not (np.isfinite(ceil) and 0 < ceil <= 1):
        raise ValueError(f"limit ceiling {ceiling} is not finite and within (0, 1]")
    if not 1 <= L <= LIMIT_MAX_LOOKAHEAD:
        raise ValueError(f"lookahead {lookahead} outside [1, {LIMIT_MAX_LOOKAHEAD}]")
    mag = np.abs(u)
    over = mag > ceil
    q = np.full(c + 2 * L, 65536, np.int64)          # q[j] at index j + L, j in [-L, c + L)
    with np.errstate(over="ignore"):
        q[L:L + c][over] = np.floor((ceil / mag[over]) * np.float32(65536.0)).astype(np.int64)
    # minima over L + 1 by doubling: m[t] = min q[t : t + span]
    m, span = q, 1
    while 2 * span <= L + 1:
        m = np.minimum(m[:-span], m[span:])
        span *= 2
    M = np.minimum(m[:c + L], m[L + 1 - span:L + 1 - span + c + L])      # M[j] at index j + L, j in [-L, c)
    E = np.concatenate([[0], np.cumsum(M)])
    S = E[L + 1:L + 1 + c] - E[:c]
    return S.astype(np.float32) / np.float32((L + 1) * 65536)


def limited(v: np.ndarray, limit) -> np.ndarray:
    """v (float32, the samples of one segment in front of the clip) under `limit` - anything with the fields ceiling and
    lookahead, or None (v itself): one float32 product with limit_gains, then the clamp to +-ceiling."""
    if limit is None:
        return v
    v = np.asarray(v, np.float32)
    ceil = np.float32(limit.ceiling)
    return np.minimum(np.maximum(v * limit_gains(v, ceil, limit.lookahead), -ceil), ceil).astype(np.float32)


def unlimited(audio: np.ndarray, peak, volume: float, mul=None) -> np.ndarray:
    """The front of the delivery's sample formula in float32, up to the shaped delivery's product: peak None - no
    normalisation; peak < 1e-8 - zeros; mul (float32, one per sample, or None) the multiplier."""
    audio = np.asarray(audio, np.float32)
    if peak is not None:
        audio = np.zeros_like(audio) if np.float32(peak) < np.float32(1e-8) else audio / np.float32(peak)
    if np.float32(volume) != np.float32(1.0):
        audio = audio * np.float32(volume)
    if mul is not None:
        audio = audio * np.asarray(mul, np.float32)
    return audio


def scaled(audio: np.ndarray, peak, volume: float, mul=None, limit=None) -> np.ndarray:
    """The delivery's sample formula in float32: peak None - no normalisation; peak < 1e-8 - zeros.  mul (float32, one per
    sample, or None): the shaped delivery's multiplier, one more product in front of the clip.  limit (or None): the limited
    delivery's limiter over these samples - one segment's - behind it."""
    audio = limited(unlimited(audio, peak, volume, mul), limit)
    return np.clip(audio, np.float32(-1.0), np.float32(1.0)).astype(np.float32)


_CURVES = {"linear": 0, "smooth": 1, 0: 0, 1: 1}


def _curve(t: np.ndarray, curve: int) -> np.ndarray:
    if curve == 0:
        return t
    return (t * t) * (np.float32(3.0) - np.float32(2.0) * t)       # four float32 operations, each rounded


def shape_multiplier(a, c, shape) -> np.ndarray:
    """The multiplier of every sample of the kept range [a, a + c) of a row under `shape` - anything with the fields of
    session.Shape: fade_in, fade_out (samples of the kept range), curve ("linear" / "smooth", or 0 / 1), points ((pos, gain),
    pos a sample index of the ROW, strictly ascending) - or None (ones).  float32 [c], every operation a float32 one, in the
    order of include/vitsmi.h, "shaped delivery"."""
    a, c = int(a), int(c)
    if shape is None:
        return np.ones(c, np.float32)
    if shape.curve not in _CURVES:
        raise ValueError(f"curve {shape.curve!r}: 'linear' or 'smooth'")
    curve = _CURVES[shape.curve]
    fade_in, fade_out = int(shape.fade_in), int(shape.fade_out)
    if fade_in < 0 or fade_out < 0:
        raise ValueError(f"fades must be >= 0 samples (got {fade_in}, {fade_out})")
    j = np.arange(c, dtype=np.int64)
    i = a + j
    e = np.ones(c, np.float32)
    pts = list(shape.points)
    if pts:
        p = np.array([int(q[0]) for q in pts], np.int64)
        g = np.array([q[1] for q in pts], np.float32)
        if (p < 0).any() or (np.diff(p) <= 0).any():
            raise ValueError("points: positions must be >= 0 and ascend strictly")
        e = np.where(i <= p[0], g[0], g[-1]).astype(np.float32)
        if len(p) > 1:
            s = (g[1:] - g[:-1]) / (p[1:] - p[:-1]).astype(np.float32)
            k = np.clip(np.searchsorted(p, i, side="right") - 1, 0, len(p) - 2)
            inner = (i > p[0]) & (i < p[-1])
            e[inner] = (g[k] + s[k] * (i - p[k]).astype(np.float32))[inner]
    w_in, w_out = np.ones(c, np.float32), np.ones(c, np.float32)
    if fade_in:
        m = j < fade_in
        w_in[m] = _curve(j[m].astype(np.float32) / np.float32(fade_in), curve)
    if fade_out:
        r = c - 1 - j
        m = r < fade_out
        w_out[m] = _curve(r[m].astype(np.float32) / np.float32(fade_out), curve)
    return ((e * w_in) * w_out).astype(np.float32)


def _row_shapes(shapes, n):
    """None, one shape or one per row -> a list of n (None: no shape)"""
    if shapes is None:
        return [None] * n
    if hasattr(shapes, "fade_in"):
        return [shapes] * n
    shapes = list(shapes)
    if len(shapes) != n:
        raise ValueError(f"shapes must be one shape or one per row ({n}), got {len(shapes)}")
    return shapes


def _row_limits(limits, n):
    """None, one limit or one per row (None in the list: off) -> a list of n"""
    if limits is None:
        return [None] * n
    if hasattr(limits, "ceiling"):
        return [limits] * n
    limits = list(limits)
    if len(limits) != n:
        raise ValueError(f"limits must be one limit or one per row ({n}), got {len(limits)}")
    return limits


def join_trimmed(rows, encoding="pcm16", lead=0, tail=0, trim=None, normalize=1, volume=1.0, shapes=None, limits=None):
    """ONE stream of a trimmed delivery on the host: every row (its valid float32 samples) cut to trim_range, then `lead`
    elements of silence, the row's kept samples post-processed and encoded, `tail` elements of silence.  normalize: 0 none,
    1 by the peak of the row's kept range, 2 by the largest of those peaks.  shapes (None, one shape or one per row): each
    row's kept samples times shape_multiplier in front of the clip; the peaks are those of the unshaped audio.  limits (None,
    one limit or one per row, None for a row without): each row's limiter (limit_gains) behind that, over its kept samples.
    Returns (data, [(a, c) per row])."""
    _check(encoding)
    kept = [trim_range(r, len(r), trim) for r in rows]
    cut = [np.asarray(r, np.float32)[a:a + c] for r, (a, c) in zip(rows, kept)]
    peaks = [np.max(np.abs(v)) if len(v) else np.float32(0) for v in cut]
    if normalize == 0:
        peaks = [None] * len(cut)
    elif normalize == 2:
        peaks = [max(peaks)] * len(cut) if cut else []
    pieces = []
    if shapes is None and limits is None:
        for v, pk in zip(cut, peaks):
            pieces += [silence(lead, encoding), encode(scaled(v, pk, volume), encoding), silence(tail, encoding)]
        return (np.concatenate(pieces) if pieces else silence(0, encoding)), kept
    for v, pk, (a, c), sh, lm in zip(cut, peaks, kept, _row_shapes(shapes, len(cut)), _row_limits(limits, len(cut))):
        mul = None if sh is None else shape_multiplier(a, c, sh)
        pieces += [silence(lead, encoding), encode(scaled(v, pk, volume, mul, lm), encoding), silence(tail, encoding)]
    return (np.concatenate(pieces) if pieces else silence(0, encoding)), kept


def emit_range(first, n, is_last, total, lookahead):
    """The timeline of a shaped stream (include/vitsmi.h, "shaped streaming"): the rendered piece [first, first + n) of rows of
    `total` samples delivers (e_first, e_n) - everything whose look-ahead has been rendered, the last piece the rest."""
    first, n, total, L = int(first), int(n), int(total), int(lookahead)
    e_first = max(first - L, 0)
    end = min(total if is_last else first + n - L, total)
    return e_first, max(end - e_first, 0)


def _row_onsets(onsets, n):
    """None, one onset or one per row (None in the list: off) -> a list of n"""
    if onsets is None:
        return [None] * n
    if hasattr(onsets, "keep_lead"):
        return [onsets] * n
    onsets = list(onsets)
    if len(onsets) != n:
        raise ValueError(f"onsets must be one onset or one per row ({n}), got {len(onsets)}")
    return onsets


def onset_threshold(onset, ref_peak):
    """thr of a trimmed row (include/vitsmi.h, "trimmed streaming"): mode 1 - the threshold; mode 2 - one float32 product with
    the row's ref_peak."""
    mode, thr = int(onset.mode), np.float32(onset.threshold)
    if mode not in (0, 1, 2):
        raise ValueError(f"onset mode {mode} outside 0..2")
    if not np.isfinite(thr) or thr < 0 or int(onset.keep_lead) < 0:
        raise ValueError(f"onset threshold {float(thr)} / keep_lead {int(onset.keep_lead)}: finite and >= 0")
    if mode == 2:
        if ref_peak is None:
            raise ValueError("onset mode 2 needs ref_peak")
        return np.float32(thr * np.float32(ref_peak))
    return thr


NO_START = 2 ** 31 - 1      # start of a trimmed row whose onset has not been found


def stream_shaped(chunks, counts, encoding="pcm16", ref_peak=None, volume=None, shapes=None, limits=None, onsets=None):
    """The shaped, limited encoded stream on the host: `chunks` yields (first_sample, float32 [B, n], total_samples) - an fp32
    stream, MiSession.synthesize_stream's -, counts (int [B], or a callable asked once, at the first chunk) are the rows'
    valid samples.  ref_peak / volume: None or one per row; shapes: None, one shape or one per row, over the whole row (a
    fade-out ends at the row's own end) - or a callable of the counts that gives them, asked with them; limits: None, one limit or one per row (None: that row is not limited), with ONE
    lookahead L.  Yields (first_sample, data [B, n] in the encoding's dtype, valid int32 [B], peak float32 [B],
    total_samples) - the chunks, timeline included, of the engine's shaped stream: a piece is delivered L samples late, the
    last one L longer, one that completes nothing not at all; `peak` is the running max |x| over what has been rendered.
    onsets (None, one onset - anything with mode, threshold, keep_lead - or one per row, None for a row that is not trimmed):
    the leading trim of "trimmed streaming" on the same timeline - a row is kept from a_b = max(f_b - keep_lead, D_k) on, its
    fades count from there, everything in front is silence; the items then carry a sixth element, skip int32 [B]."""
    _check(encoding)
    state = None
    for first, x, total in chunks:
        x = np.asarray(x, np.float32)
        B, n = x.shape
        first, total = int(first), int(total)
        if state is None:
            cnt = np.asarray(counts() if callable(counts) else counts, np.int64)
            shp, lim = _row_shapes(shapes(cnt) if callable(shapes) else shapes, B), _row_limits(limits, B)
            ahead = sorted({int(l.lookahead) for l in lim if l is not None})
            if len(ahead) > 1:
                raise ValueError(f"limits: one lookahead per stream, got {ahead}")
            L = ahead[0] if ahead else 0
            muls = [None if shp[b] is None else shape_multiplier(0, cnt[b], shp[b]) for b in range(B)]
            pk = [None] * B if ref_peak is None else list(np.broadcast_to(np.asarray(ref_peak, np.float32), (B,)))
            vol = np.broadcast_to(np.asarray(1.0 if volume is None else volume, np.float32), (B,))
            state = np.zeros((B, 2 * L), np.float32), np.zeros(B, np.float32)     # the carry, the running peaks
            ons = _row_onsets(onsets, B)
            thr = [None if o is None or int(o.mode) == 0 else onset_threshold(o, pk[b]) for b, o in enumerate(ons)]
            start = [0 if t is None else NO_START for t in thr]
        carry, peak = state
        joined = np.concatenate([carry, x], axis=1)                  # samples [first - 2 L, first + n) of the rows
        base = first - 2 * L
        for b in range(B):
            seen = x[b, :int(np.clip(cnt[b] - first, 0, n))]
            if seen.size:
                peak[b] = max(peak[b], np.max(np.abs(seen)))
        state = joined[:, joined.shape[1] - 2 * L:], peak
        ef, en = emit_range(first, n, first + n >= total, total, L)
        for b in range(B):      # the scan: every rendered piece, whether or not it completes anything
            if start[b] != NO_START:
                continue
            hit = np.flatnonzero(np.abs(x[b, :int(np.clip(cnt[b] - first, 0, n))]) > thr[b])
            if hit.size:
                start[b] = max(first + int(hit[0]) - int(ons[b].keep_lead), ef)
                if shp[b] is not None:
                    muls[b] = shape_multiplier(start[b], cnt[b] - start[b], shp[b])
        if en == 0:
            continue
        data = np.full((B, en), SILENCE[encoding], DTYPES[encoding])
        valid = np.clip(cnt - ef, 0, en).astype(np.int32)
        skip = np.clip(np.asarray(start, np.int64) - ef, 0, valid).astype(np.int32)
        for b in range(B):
            if skip[b] >= valid[b]:
                continue
            # g of [ef, ef + valid) needs q of L samples on either side: u over [lo, hi), inside the kept range
            a, d0 = start[b], ef + int(skip[b])
            lo, hi = max(ef - L, a), int(min(ef + en + L, cnt[b]))
            u = unlimited(joined[b, lo - base:hi - base], pk[b], vol[b], None if muls[b] is None else muls[b][lo - a:hi - a])
            v = limited(u, lim[b])[d0 - lo:ef - lo + int(valid[b])]
            data[b, int(skip[b]):int(valid[b])] = encode(np.clip(v, np.float32(-1.0), np.float32(1.0)).astype(np.float32), encoding)
        if onsets is None:
            yield ef, data, valid, peak.copy(), total
        else:
            yield ef, data, valid, peak.copy(), total, skip


def k_weighting(rate):
    """The K-weighting of BS.1770 at `rate` Hz: ((b, a) of the shelf, (b, a) of the high-pass), the standard's analogue
    prototypes through the bilinear transform (at 48 kHz: its table)."""
    G, Q, f0 = 3.999843853973347, 0.7071752369554196, 1681.974450955533
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    Q, f0 = 0.5003270373238773, 38.13547087602444
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    return shelf, ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def _biquad(b, a, x):
    """one biquad from rest over a list of floats (transposed direct form II, float64)"""
    b0, b1, b2 = b
    _, a1, a2 = a
    z1 = z2 = 0.0
    y = [0.0] * len(x)
    for n, v in enumerate(x):
        w = b0 * v + z1
        z1 = b1 * v - a1 * w + z2
        z2 = b2 * v - a2 * w
        y[n] = w
    return y


def sub_block_energies(x, rate) -> np.ndarray:
    """The K-weighted energies of the whole 100 ms sub-blocks of x (float64 [len(x) // hop]), hop = (rate + 5) // 10."""
    hop = (int(rate) + 5) // 10
    n_sub = len(x) // hop
    if n_sub == 0:
        return np.zeros(0, np.float64)
    shelf, hp = k_weighting(rate)
    y = np.array(_biquad(*hp, _biquad(*shelf, np.asarray(x, np.float64)[:n_sub * hop].tolist())), np.float64)
    return (y * y).reshape(n_sub, hop).sum(axis=1)


def gated_loudness(rows_e, rate) -> float:
    """The gates of BS.1770-4 over the sub-block energies of one or several rows, pooled: 400 ms blocks at 75 % overlap within
    each row, the absolute gate at -70 LUFS, the relative gate 10 LU below the absolute-gated mean.  -inf: no block passes."""
    hop = (int(rate) + 5) // 10
    z = [np.zeros(0)]
    for e in rows_e:
        e = np.asarray(e, np.float64)
        if e.size >= 4:
            z.append((e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * hop))
    z = np.concatenate(z)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return -math.inf
    both = keep & (l > -0.691 + 10.0 * math.log10(z[keep].mean()) - 10.0)
    return -0.691 + 10.0 * math.log10(z[both].mean()) if both.any() else -math.inf


def loudness(x, rate) -> float:
    """The integrated loudness of x at `rate` Hz in LUFS (ITU-R BS.1770-4, mono); -inf for less than 400 ms or silence."""
    return gated_loudness([sub_block_energies(x, rate)], rate)


def level_gain(loudness, peak, target_lufs, max_gain_db=30.0, peak_ceiling=0.0) -> np.float32:
    """The gain that brings audio of integrated loudness `loudness` to target_lufs: at most max_gain_db, and with
    peak_ceiling > 0 no more than what keeps the sample peak `peak` at or below it; 1 for a loudness of -inf."""
    if loudness == -math.inf:
        return np.float32(1.0)
    g = min(10.0 ** ((float(np.float32(target_lufs)) - loudness) / 20.0), 10.0 ** (float(np.float32(max_gain_db)) / 20.0))
    if peak_ceiling > 0 and peak > 0:
        g = min(g, float(np.float32(peak_ceiling)) / float(peak))
    return np.float32(g)


def leveled(audio: np.ndarray, gain, volume: float, mul=None, limit=None) -> np.ndarray:
    """The levelled delivery's sample formula in float32: one product with the gain, the volume's, (a shape's, a limiter's,)
    the clip."""
    return scaled(np.asarray(audio, np.float32) * np.float32(gain), None, volume, mul, limit)


def level_rows(rows, rate, level):
    """The loudness and the gain of every row (its float32 samples, already cut to what is kept) under `level`: anything with
    the fields of vits_level - mode (1: every row by itself, 2: the rows pooled into one gating computation, one gain by the
    largest peak), target_lufs, max_gain_db, peak_ceiling.  Returns (loudness per row, gain per row)."""
    if int(level.mode) not in (1, 2):
        raise ValueError(f"level mode {level.mode} outside 1..2")
    peaks = [np.max(np.abs(v)) if len(v) else np.float32(0) for v in rows]
    energies = [sub_block_energies(v, rate) for v in rows]
    if int(level.mode) == 1:
        loud = [gated_loudness([e], rate) for e in energies]
    else:
        loud = [gated_loudness(energies, rate)] * len(rows)
        peaks = [max(peaks)] * len(rows) if rows else []
    return loud, [level_gain(L, pk, level.target_lufs, level.max_gain_db, level.peak_ceiling) for L, pk in zip(loud, peaks)]


def join_leveled(rows, rate, level, encoding="pcm16", lead=0, tail=0, trim=None, volume=1.0, shapes=None, limits=None):
    """ONE stream of a levelled delivery on the host: join_trimmed with every row's kept range brought to a loudness target
    (level_rows) instead of peak-normalised.  shapes and limits as in join_trimmed: the loudness is that of the unshaped,
    unlimited audio.
    Returns (data, [(a, c) per row], loudness per row, gain per row)."""
    _check(encoding)
    kept = [trim_range(r, len(r), trim) for r in rows]
    cut = [np.asarray(r, np.float32)[a:a + c] for r, (a, c) in zip(rows, kept)]
    loud, gains = level_rows(cut, rate, level)
    pieces = []
    if shapes is None and limits is None:
        for v, g in zip(cut, gains):
            pieces += [silence(lead, encoding), encode(leveled(v, g, volume), encoding), silence(tail, encoding)]
        return (np.concatenate(pieces) if pieces else silence(0, encoding)), kept, loud, gains
    for v, g, (a, c), sh, lm in zip(cut, gains, kept, _row_shapes(shapes, len(cut)), _row_limits(limits, len(cut))):
        mul = None if sh is None else shape_multiplier(a, c, sh)
        pieces += [silence(lead, encoding), encode(leveled(v, g, volume, mul, lm), encoding), silence(tail, encoding)]
    return (np.concatenate(pieces) if pieces else silence(0, encoding)), kept, loud, gains


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
    # synthesize_encoded(..., loudness=): per sentence, the integrated loudness measured in front of the gain (LUFS; with
    # loudness_scope="text" the text's, repeated; -inf below 400 ms) and the gain applied
    loudness: Optional[List[float]] = None
    gain: Optional[List[float]] = None
    # synthesize_encoded(..., duration=): the multiplier s* the text's durations were fitted with and the outcome (vitsmi.h,
    # "fitted durations": 0 met, 1 floor, 2 ceiling, 3 kept)
    fit_scale: Optional[float] = None
    fit_status: Optional[int] = None

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
