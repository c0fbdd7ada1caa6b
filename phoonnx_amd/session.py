"""MiSession — the object that stands where `onnxruntime.InferenceSession` stands in
phoonnx (`phoonnx/voice.py:107,167-171,347,374-377`).

It duck-types exactly the three calls the reference makes:
    MiSession(path, sess_options=..., providers=...)      voice.py:167-171
    session.get_inputs() -> objects with .name            voice.py:347
    session.run(None, feed)[0] -> float32 [B,1,1,S]       voice.py:374-377
and forwards them over the C ABI (include/vitsmi.h) to the gfx950 engine.  There is no CPU
fallback: without libvitsmi.so + an MI355X this raises.
"""
import contextlib
import ctypes as C
import dataclasses
import time
from collections import namedtuple
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi


class SessionError(RuntimeError):
    """Raised for every failure of the engine (onnxruntime raises its own
    InvalidArgument/RuntimeException at voice.py:374; callers there do not catch either)."""


class RangeError(SessionError):
    """VITS_E_RANGE: the f16x3 generator arithmetic met an activation beyond the range of its fp16 operand planes
    (|x| > 65504) or a non-finite value.  The engine reports this instead of returning clamped audio; `MiSession`
    (range_fallback=True, the default) then reopens the voice with the bf16x6 arithmetic (fp32 range) and repeats the
    call, so user code only sees this when the fallback is switched off or impossible (borrowed weight arena)."""


class _PinnedPool:
    """Page-locked host blocks handed out as NumPy arrays (the DMA engine writes a result straight into the array the
    caller receives: no staging copy, no second copy into a fresh array).  A block goes back to the pool when the last
    array viewing it has been garbage-collected; at most `keep_bytes` of idle blocks are retained.

    The finalizer takes no lock: it may run inside ANY allocation of ANY thread (a cyclic-GC pass), including one made by
    array() while it holds the pool's lock.  It only appends to a deque (atomic); array() sorts the returned blocks into
    the free lists, under the lock, the next time it runs."""

    def __init__(self, keep_bytes=2 << 30):
        import collections
        import threading
        self._free = {}
        self._idle = 0
        self._keep = keep_bytes
        self._mu = threading.Lock()
        self._returned = collections.deque()   # (ptr, cap) of blocks whose arrays have died; drained by array()
        self._types = {}                       # cap -> ctypes array type (ctypes caches every distinct type forever)

    @staticmethod
    def _cap(nbytes):
        return max(1 << 16, (int(nbytes) + (1 << 20) - 1) >> 20 << 20) if nbytes > (1 << 16) else 1 << 16

    def _give(self, ptr, cap):
        self._returned.append((ptr, cap))  # (lock-free: see the class docstring)

    def _drain(self):
        """(under self._mu) returned blocks -> free lists; what exceeds keep_bytes is released"""
        release = []
        while True:
            try:
                ptr, cap = self._returned.popleft()
            except IndexError:
                break
            if self._idle + cap <= self._keep:
                self._free.setdefault(cap, []).append(ptr)
                self._idle += cap
            else:
                release.append(ptr)
        return release

    def drain(self, keep_bytes=None):
        """Sort the blocks whose arrays have died into the free lists NOW and release what exceeds `keep_bytes` (default: the
        pool's cap; 0 releases every idle block).  array() does this as it goes; a process that rendered one large batch and
        then goes idle, streams, or asks for pageable results calls it through MiSession.close() / _fetch so that the host
        memory does not stay page-locked until the next pooled allocation."""
        with self._mu:
            release = self._drain()
            if keep_bytes is not None:
                for c in sorted(self._free, reverse=True):
                    while self._free[c] and self._idle > keep_bytes:
                        release.append(self._free[c].pop())
                        self._idle -= c
        for q in release:
            _ffi.load().vits_host_free(q)
        return len(release)

    def array(self, shape, dtype=np.float32):
        import weakref
        count = int(np.prod(shape))
        n = count * np.dtype(dtype).itemsize
        cap = self._cap(n)
        ptr = None
        with self._mu:
            release = self._drain()
            # an idle block of this size class, or the smallest one up to twice as large
            for c in sorted([k for k, v in self._free.items() if v and cap <= k <= 2 * cap]):
                ptr, cap = self._free[c].pop(), c
                self._idle -= c
                break
            ctype = self._types.get(cap)
            if ctype is None:
                ctype = self._types[cap] = C.c_char * cap   # one type per size class, not per output length
        for q in release:
            _ffi.load().vits_host_free(q)
        if ptr is None:
            ptr = _ffi.load().vits_host_alloc(cap)
            if not ptr:
                raise SessionError(f"cannot allocate {cap} bytes of pinned host memory")
        buf = ctype.from_address(ptr)
        fin = weakref.finalize(buf, self._give, ptr, cap)
        fin.atexit = False  # (at interpreter exit the driver reclaims it)
        return np.frombuffer(buf, dtype, count=count).reshape(shape)


_POOL = _PinnedPool()


@dataclass
class NodeArg:
    name: str
    type: str
    shape: list


_INPUT_SPECS = {
    "input": ("tensor(int64)", ["batch_size", "phonemes"]),
    "input_lengths": ("tensor(int64)", ["batch_size"]),
    "scales": ("tensor(float)", [3]),
    "sid": ("tensor(int64)", ["batch_size"]),
    "langid": ("tensor(int64)", ["batch_size"]),  # third-party exports (voice.py:369); accepted, validated, unused
}


class ModelMeta:
    def __init__(self, custom):
        self.custom_metadata_map = custom
        self.producer_name = "pytorch"
        self.graph_name = "vits"


def _settings(scales, B, seeds=None):
    """Per-utterance synthesis settings of a batch call: `scales` float32 [3] (every utterance) or [B, 3] (utterance b:
    row b = [noise_scale, length_scale, noise_w]), `seeds` None or B integers in [0, 2^64) (each utterance's own noise
    stream, vitsmi.h).  Returns (scales, seeds as uint64 [B] or None); raises SessionError before anything reaches the
    device."""
    scales = np.ascontiguousarray(scales)
    if scales.dtype != np.float32 or scales.shape not in ((3,), (B, 3)):
        raise SessionError("Unexpected input: 'scales' must be float32 of shape [3] or [batch_size, 3]")
    if scales.ndim == 2:
        bad = np.flatnonzero(~np.isfinite(scales).all(axis=1))
        if bad.size:
            raise SessionError(f"scales row {int(bad[0])} = {scales[bad[0]].tolist()} is not finite")
    if seeds is None:
        return scales, None
    arr = np.asarray(seeds)
    if arr.shape != (B,) or not (arr.dtype.kind in "iu" or (arr.dtype == object and all(isinstance(v, int) for v in arr))):
        raise SessionError("Unexpected input: 'seeds' must be integers of shape [batch_size]")
    if arr.dtype != np.uint64:
        vals = [int(v) for v in arr]
        if any(v < 0 or v >= 1 << 64 for v in vals):
            raise SessionError("Unexpected input: 'seeds' must lie in [0, 2^64)")
        arr = np.array(vals, dtype=np.uint64)
    return scales, np.ascontiguousarray(arr)


def _timing(durations, token_rate, lens, B, T):
    """Timing controls of a batch call (vitsmi.h, vits_controls): `durations` None or integers [B, T] (forced: token t of
    utterance b occupies durations[b, t] frames; the duration predictor does not run), `token_rate` None or floats [B, T]
    (a multiplier on each token's predicted duration; finite, >= 0).  Positions behind lens[b] are ignored.  Returns
    (int64 [B, T] or None, float32 [B, T] or None); raises SessionError naming the argument before anything reaches the
    device (the engine checks the same, and the frame-count limits, once more)."""
    if durations is None and token_rate is None:
        return None, None
    if durations is not None and token_rate is not None:
        raise SessionError("Unexpected input: 'durations' and 'token_rate' are contradictory (forced durations leave "
                           "nothing to scale): pass one of them")
    valid = np.arange(T)[None, :] < np.clip(np.asarray(lens).reshape(-1, 1), 0, T)
    if durations is not None:
        d = np.asarray(durations)
        if d.dtype.kind not in "iu":
            raise SessionError(f"Unexpected input data type: 'durations' must be integers (frames per token), got {d.dtype}")
        if d.shape != (B, T):
            raise SessionError(f"Invalid shape for 'durations': {d.shape}, expected [batch_size, phonemes] = {(B, T)}")
        if d.dtype == np.uint64:
            d = np.minimum(d, np.uint64(1 << 62))   # (far above the engine's limit either way; keeps the sign bit clear)
        d = np.ascontiguousarray(d, np.int64)
        bad = np.argwhere((d < 0) & valid)
        if bad.size:
            b, t = (int(v) for v in bad[0])
            raise SessionError(f"durations[{b},{t}]={int(d[b, t])} is negative")
        return d, None
    r = np.asarray(token_rate)
    if r.dtype.kind != "f":
        raise SessionError(f"Unexpected input data type: 'token_rate' must be floats, got {r.dtype}")
    if r.shape != (B, T):
        raise SessionError(f"Invalid shape for 'token_rate': {r.shape}, expected [batch_size, phonemes] = {(B, T)}")
    r = np.ascontiguousarray(r, np.float32)
    bad = np.argwhere(~(np.isfinite(r) & (r >= 0)) & valid)
    if bad.size:
        b, t = (int(v) for v in bad[0])
        raise SessionError(f"token_rate[{b},{t}]={float(r[b, t])} is not a finite value >= 0")
    return None, r


def _controls(rows, seeds, durations, token_rate):
    """The vits_controls struct over host arrays.  The struct holds bare addresses, so it also holds the arrays themselves
    (`_keep`): whoever keeps the struct - a chunked run's closure, which runs on a worker thread after its caller has
    returned - keeps the memory it points into."""
    c = _ffi.VitsControls()
    c._keep = (rows, seeds, durations, token_rate)
    c.scales_rows = rows.ctypes.data
    c.seeds = None if seeds is None else seeds.ctypes.data
    c.durations = None if durations is None else durations.ctypes.data
    c.token_rate = None if token_rate is None else token_rate.ctypes.data
    return c


def _noise(seed, noise_dp=None, noise_z=None):
    """The vits_noise struct of a call: the session's seed and, for parity runs, the injected noise as contiguous float32.
    Like _controls, the struct holds the arrays it points into (`_keep`)."""
    n = _ffi.VitsNoise()
    n.seed = seed
    n._keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (noise_dp, noise_z)]
    if noise_dp is not None:
        n.noise_dp = n._keep[0].ctypes.data
    if noise_z is not None:
        n.noise_z, n.noise_z_stride = n._keep[1].ctypes.data, n._keep[1].shape[2]
    return n


FIT_MODES = {"exact": 1, "at_most": 2}
VITS_MAX_FORCED_FRAMES = 1 << 24


class Fit:
    """Fitted durations of a run (vitsmi.h, "fitted durations"): `groups` - one entry per row, the row's group or -1 for a row
    that keeps its own durations; `target_frames` - one frame count per group, the sum of the durations of all the group's
    tokens; `modes` - "exact" (1) or "at_most" (2), one for all groups or one per group.  Fit.one_group(B, frames) puts all
    rows of a batch - the sentences of a text - into one group."""

    def __init__(self, groups, target_frames, modes="exact"):
        self.groups = np.atleast_1d(np.asarray(groups))
        self.target_frames = np.atleast_1d(np.asarray(target_frames))
        m = [modes] * len(self.target_frames) if isinstance(modes, (str, int, np.integer)) else list(modes)
        self.modes = np.array([FIT_MODES.get(v, v) if isinstance(v, str) else v for v in m], dtype=object)

    @classmethod
    def one_group(cls, B, target_frames, mode="exact"):
        return cls(np.zeros(int(B), np.int32), [int(target_frames)], mode)


def _fit(fit, B, hop, durations=None, semitones=None):
    """fit= of a run -> the vits_fit struct over validated host arrays (None: no fit, or no row in any group - the entry
    without a fit).  What the engine would refuse is raised here, by the call, in the engine's words: nothing was started."""
    if fit is None:
        return None
    if not isinstance(fit, Fit):
        raise SessionError(f"Unexpected input: 'fit' must be a session.Fit, got {type(fit).__name__}")
    if durations is not None:
        raise ValueError("fit= and durations= are contradictory: forced durations leave nothing to fit")
    if semitones is not None:
        raise ValueError("fit= together with token_semitones= / token_semitones_end= is not covered: with compensate the "
                         "delivered length is not the native frame count")
    g, t, m = fit.groups, fit.target_frames, fit.modes
    G = len(t)
    if g.ndim != 1 or g.dtype.kind not in "iu" or g.shape[0] != B:
        raise SessionError(f"Invalid shape for 'fit.groups': {g.shape} {g.dtype}, expected [batch_size] = ({B},) integers")
    if t.ndim != 1 or t.dtype.kind not in "iu" or len(m) != G:
        raise SessionError(f"'fit.target_frames' must be integers [n_groups] with one mode per group (got {t.shape} {t.dtype}, "
                           f"{len(m)} modes)")
    for b in range(B):
        if not -1 <= int(g[b]) < G:
            raise SessionError(f"fit group[{b}]={int(g[b])} outside [-1,{G})")
    max_frames = min(VITS_MAX_FORCED_FRAMES, (2 ** 31 - 1) // max(int(hop), 1))
    for k in range(G):
        if not 1 <= int(t[k]) <= max_frames:
            raise SessionError(f"fit target_frames[{k}]={int(t[k])} outside [1,{max_frames}] (VITS_MAX_FORCED_FRAMES, INT_MAX / hop)")
        if m[k] not in (1, 2):
            raise SessionError(f"fit mode[{k}]={m[k]!r} is neither 1 (exact) nor 2 (at most)")
        if not (g == k).any():
            raise SessionError(f"fit group {k} has no rows")
    if G == 0 or not (g >= 0).any():
        return None
    g32, t64, m32 = np.ascontiguousarray(g, np.int32), np.ascontiguousarray(t, np.int64), np.array([int(v) for v in m], np.int32)
    c = _ffi.VitsFit(g32.ctypes.data, G, t64.ctypes.data, m32.ctypes.data)
    c._keep = (g32, t64, m32)
    return c


def fit_plan(w, lens, fit):
    """The plan of a fit over weights float32 [B, T] (vits_fit_plan: pure host code) -> (durations int64 [B, T] with -1 in
    the rows of no group, scale float64 [G], frames int64 [G], status int32 [G])"""
    w = np.ascontiguousarray(w, np.float32)
    lens = np.ascontiguousarray(lens, np.int64)
    if w.ndim != 2 or lens.shape != (w.shape[0],):
        raise SessionError(f"fit_plan: w must be [B, T] and lens [B] (got {w.shape}, {lens.shape})")
    B, T = w.shape
    g32, t64 = np.ascontiguousarray(fit.groups, np.int32), np.ascontiguousarray(fit.target_frames, np.int64)
    m32 = np.array([int(v) for v in fit.modes], np.int32)
    G = len(t64)
    c = _ffi.VitsFit(g32.ctypes.data, G, t64.ctypes.data, m32.ctypes.data)
    dur = np.full((B, T), -1, np.int64)
    scale, frames, status = np.zeros(G, np.float64), np.zeros(G, np.int64), np.zeros(G, np.int32)
    rc = _ffi.load().vits_fit_plan(_ffi.ptr(w), _ffi.ptr(lens), B, T, C.byref(c), _ffi.ptr(dur), _ffi.ptr(scale), _ffi.ptr(frames),
                                   _ffi.ptr(status))
    if rc != 0:
        raise SessionError(f"vits_fit_plan failed [{rc}]: {_ffi.last_error(None)}")
    return dur, scale, frames, status


def _semitones(token_semitones, lens, B, T, name="token_semitones"):
    """token_semitones - None, or floats [B, T] within [-12, 12] in front of lens[b] (vitsmi.h, "intonation") -> float32
    [B, T], contiguous"""
    if token_semitones is None:
        return None
    st = np.asarray(token_semitones)
    if st.dtype.kind not in "fiu":
        raise SessionError(f"Unexpected input data type: '{name}' must be floats, got {st.dtype}")
    if st.shape != (B, T):
        raise SessionError(f"Invalid shape for '{name}': {st.shape}, expected [batch_size, phonemes] = {(B, T)}")
    st = np.ascontiguousarray(st, np.float32)
    live = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    bad = live & ~(np.isfinite(st) & (np.abs(st) <= 12))
    if bad.any():
        b, t = (int(v) for v in np.argwhere(bad)[0])
        raise SessionError(f"{name}[{b},{t}]={float(st[b, t])} is not a finite value within [-12, 12]")
    return st


def _contour(token_semitones, token_semitones_end, lens, B, T):
    """(start, end) values of a run (vitsmi.h, "pitch contours"): end None - no glide: (_semitones(...), None); else both
    float32 [B, T], the start values zeros where only the end values are given"""
    st0 = _semitones(token_semitones, lens, B, T)
    if token_semitones_end is None:
        return st0, None
    st1 = _semitones(token_semitones_end, lens, B, T, "token_semitones_end")
    return (np.zeros((B, T), np.float32) if st0 is None else st0), st1


def _pitched(semitones, semitones_end, lens) -> bool:
    """does a run with these (start, end) values of _contour warp at all - some value in front of lens[b] that is not 0"""
    if semitones is None:
        return False
    live = np.arange(semitones.shape[1])[None, :] < np.asarray(lens)[:, None]
    return bool((live & ((semitones != 0) | (False if semitones_end is None else (semitones_end != 0)))).any())


def token_span_bounds(spans, count) -> np.ndarray:
    """token_bounds of a warped row: the boundaries of its tokens in delivered samples from the warp's own spans (k per
    token, last_token_spans()) -> int64 [len(spans) + 1]; a row's last boundary is its count N."""
    bounds = np.minimum(int(count), np.concatenate([[0], np.cumsum(np.asarray(spans, np.int64))]))
    bounds[-1] = int(count)   # (a row whose tokens were all dropped still has its one frame)
    return bounds


def resample_plan(in_rate: int, out_rate: int, table: bool = False):
    """The output-rate resampler's plan for a pair of rates (vitsmi.h, "output rate"; pure host code): (L, M, K), or with
    table=True (L, M, K, h float32 [L, K]).  Raises SessionError for a pair the engine refuses."""
    lib = _ffi.load()
    L, M, K = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.vits_resample_plan(int(in_rate), int(out_rate), C.byref(L), C.byref(M), C.byref(K), None, 0)
    if rc != 0:
        raise SessionError(f"vits_resample_plan({in_rate}, {out_rate}) failed [{rc}]: {_ffi.last_error(None)}")
    if not table:
        return L.value, M.value, K.value
    h = np.empty((L.value, K.value), np.float32)
    rc = lib.vits_resample_plan(int(in_rate), int(out_rate), None, None, None, _ffi.ptr(h), h.size)
    if rc != 0:
        raise SessionError(f"vits_resample_plan({in_rate}, {out_rate}) failed [{rc}]: {_ffi.last_error(None)}")
    return L.value, M.value, K.value, h


def output_sample_counts(n_samples, in_rate: int, out_rate) -> np.ndarray:
    """ceil(n * L / M): the output samples of rows of n valid input samples (what last_sample_counts() reports per row).
    out_rate: one rate, or one per row of n_samples (vitsmi.h, "output rate per row"; None, 0 or in_rate: a native row)."""
    n = np.asarray(n_samples, np.int64)
    if np.ndim(out_rate) == 0 and out_rate is not None:
        L, M, _ = resample_plan(in_rate, out_rate)
        return -(-n * L // M)
    rates = [in_rate] * n.size if out_rate is None else list(out_rate)
    if n.ndim != 1 or len(rates) != n.shape[0]:
        raise SessionError(f"output_sample_counts: {len(rates)} rates for rows of shape {n.shape}")
    out = n.copy()
    for b, r in enumerate(rates):
        if r not in (None, 0, in_rate):
            L, M, _ = resample_plan(in_rate, int(r))
            out[b] = -(-int(n[b]) * L // M)
    return out


@dataclass
class Segment:
    """One segment of a delivery plan (vitsmi.h, vits_segment): row `row` of the last run goes into stream `stream`, behind
    `lead_samples` samples of silence; normalize: 0 none, 1 by the row's own peak, 2 by the peak of the stream."""
    row: int
    stream: int = 0
    lead_samples: int = 0
    normalize: int = 1
    volume: float = 1.0


@dataclass
class Trim:
    """The trim of one segment (vitsmi.h, vits_trim): mode 0 off, 1 - a sample is active above `threshold`, 2 - above
    `threshold` times the row's peak; the segment keeps its first to its last active sample and keep_lead / keep_tail samples
    around them, and is followed by tail_samples samples of silence."""
    mode: int = 0
    threshold: float = 0.0
    keep_lead: int = 0
    keep_tail: int = 0
    tail_samples: int = 0


@dataclass
class Level:
    """The level of one segment (vitsmi.h, vits_level): mode 0 off, 1 - the segment is brought to `target_lufs` (integrated
    loudness, ITU-R BS.1770-4) by itself, 2 - together with the stream's other mode-2 segments, by one gain; the gain is at
    most max_gain_db, and with peak_ceiling > 0 the levelled SAMPLE peak stays at or below it."""
    mode: int = 0
    target_lufs: float = -23.0
    max_gain_db: float = 30.0
    peak_ceiling: float = 0.0


@dataclass
class Shape:
    """The shape of one segment (vitsmi.h, vits_shape): fade_in / fade_out - the samples of the kept range that ramp up from 0
    and down to 0; curve "linear" or "smooth"; points - (pos, gain) breakpoints of a piecewise-linear volume over the ROW's
    samples at the delivered rate (pos counted from the row's start, strictly ascending; gain 0 or within [2^-20, 64])."""
    fade_in: int = 0
    fade_out: int = 0
    curve: str = "linear"
    points: Sequence = ()


@dataclass
class Limit:
    """The look-ahead peak limiter of one segment (vitsmi.h, vits_limit): no delivered sample of the segment exceeds `ceiling`
    ((0, 1]) in magnitude; the gain begins to fall `lookahead` samples (at the delivered rate, [1, 1024]) ahead of a peak and
    has recovered as many behind it.  In a list of limits, None stands for a segment that is not limited."""
    ceiling: float = 1.0
    lookahead: int = 110


@dataclass
class Onset:
    """The leading trim of one row of an encoded stream (vitsmi.h, vits_stream_onset): mode 0 off, 1 - a sample is active
    above `threshold`, 2 - above `threshold` times the row's ref_peak; the row is kept from its first active sample on, with
    up to keep_lead samples (at the delivered rate) in front of it - as many of them as the stream has not handed over yet."""
    mode: int = 0
    threshold: float = 0.0
    keep_lead: int = 0


_CURVES = {"linear": 0, "smooth": 1}


def _encoding(encoding):
    try:
        return _ffi.ENCODINGS[encoding]
    except (KeyError, TypeError):
        raise SessionError(f"unknown encoding {encoding!r}: one of {sorted(_ffi.ENCODINGS)}") from None


def _segments(segments):
    """Segment objects -> (ctypes array of vits_segment, its length)"""
    segments = list(segments)
    arr = (_ffi.VitsSegment * max(len(segments), 1))()
    for i, g in enumerate(segments):
        try:
            arr[i] = _ffi.VitsSegment(int(g.row), int(g.stream), int(g.lead_samples), int(g.normalize), float(g.volume))
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"segment {i}: {e}") from None
    return arr, len(segments)


def _trims(trims, n):
    """None, one Trim or one per segment -> ctypes array of n vits_trim (None: no trims)"""
    if trims is None:
        return None
    trims = [trims] * n if isinstance(trims, Trim) else list(trims)
    if len(trims) != n:
        raise SessionError(f"trims must be one Trim or one per segment ({n}), got {len(trims)}")
    arr = (_ffi.VitsTrim * max(n, 1))()
    for i, t in enumerate(trims):
        try:
            arr[i] = _ffi.VitsTrim(int(t.mode), float(t.threshold), int(t.keep_lead), int(t.keep_tail), int(t.tail_samples))
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"segment {i}: trim: {e}") from None
    return arr


def _levels(levels, n):
    """None, one Level or one per segment -> ctypes array of n vits_level (None: no levels)"""
    if levels is None:
        return None
    levels = [levels] * n if isinstance(levels, Level) else list(levels)
    if len(levels) != n:
        raise SessionError(f"levels must be one Level or one per segment ({n}), got {len(levels)}")
    arr = (_ffi.VitsLevel * max(n, 1))()
    for i, l in enumerate(levels):
        try:
            arr[i] = _ffi.VitsLevel(int(l.mode), float(l.target_lufs), float(l.max_gain_db), float(l.peak_ceiling))
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"segment {i}: level: {e}") from None
    return arr


# shapes as the C structs hold them, for the tests of the validation: shapes - (fade_in, fade_out, curve, n_points, first_point)
# per segment; points - (pos, gain) pairs; n_points - the count the call states (None: len(points))
RawShapes = namedtuple("RawShapes", "shapes points n_points", defaults=(None,))


def _points(flat):
    """(pos, gain) pairs -> a C array of vits_env_point (at least one element)"""
    arr = np.zeros(max(len(flat), 1), np.dtype([("pos", "<i4"), ("gain", "<f4")]))
    if flat:
        pos = np.array([p for p, _ in flat], np.int64)
        if ((pos < -2 ** 31) | (pos >= 2 ** 31)).any():
            k = int(np.flatnonzero((pos < -2 ** 31) | (pos >= 2 ** 31))[0])
            raise SessionError(f"point {k}: pos {int(pos[k])} outside [0, {2 ** 31 - 1}]")
        arr["pos"], arr["gain"] = pos, np.array([g for _, g in flat], np.float32)
    return arr


def _shapes(shapes, n):
    """None, one Shape or one per segment -> (ctypes array of n vits_shape, the points of all of them back to back as a
    structured array of vits_env_point, their count); (None, None, 0) for None"""
    if shapes is None:
        return None, None, 0
    if isinstance(shapes, RawShapes):
        arr = (_ffi.VitsShape * max(len(shapes.shapes), 1))(*[_ffi.VitsShape(*(int(v) for v in r)) for r in shapes.shapes])
        flat = [(int(p), float(g)) for p, g in shapes.points]
        return arr, _ffi.ptr(_points(flat)), len(flat) if shapes.n_points is None else int(shapes.n_points)
    shapes = [shapes] * n if isinstance(shapes, Shape) else list(shapes)
    if len(shapes) != n:
        raise SessionError(f"shapes must be one Shape or one per segment ({n}), got {len(shapes)}")
    arr = (_ffi.VitsShape * max(n, 1))()
    flat = []
    for i, sh in enumerate(shapes):
        try:
            curve = _CURVES[sh.curve] if isinstance(sh.curve, str) else int(sh.curve)
            pts = [(int(pos), float(gain)) for pos, gain in sh.points]
            arr[i] = _ffi.VitsShape(int(sh.fade_in), int(sh.fade_out), curve, len(pts), len(flat))
            flat += pts
        except KeyError:
            raise SessionError(f"segment {i}: shape: curve {sh.curve!r}: one of {sorted(_CURVES)}") from None
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"segment {i}: shape: {e}") from None
    return arr, _ffi.ptr(_points(flat)), len(flat)


# limits as the C structs hold them, for the tests of the validation: (mode, ceiling, lookahead, reserved) per segment
RawLimits = namedtuple("RawLimits", "limits")


def _limits(limits, n):
    """None, one Limit or one per segment (None in the list: that segment is off) -> ctypes array of n vits_limit (None: no
    limits)"""
    if limits is None:
        return None
    if isinstance(limits, RawLimits):
        return (_ffi.VitsLimit * max(len(limits.limits), 1))(*[_ffi.VitsLimit(int(m), float(c), int(l), int(r)) for m, c, l, r in limits.limits])
    limits = [limits] * n if isinstance(limits, Limit) else list(limits)
    if len(limits) != n:
        raise SessionError(f"limits must be one Limit or one per segment ({n}), got {len(limits)}")
    arr = (_ffi.VitsLimit * max(n, 1))()
    for i, l in enumerate(limits):
        try:
            arr[i] = _ffi.VitsLimit(0, 1.0, 1, 0) if l is None else _ffi.VitsLimit(1, float(l.ceiling), int(l.lookahead), 0)
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"segment {i}: limit: {e}") from None
    return arr


def limit_check(limits, segments=None, n=None):
    """The validation of a limited delivery's limits (vits_limit_check: pure host code) over `segments` (None: the volumes are
    not looked at); a refusal raises SessionError."""
    if n is None:
        n = 1 if isinstance(limits, Limit) else len(limits.limits if isinstance(limits, RawLimits) else list(limits))
    sarr = None
    if segments is not None:
        sarr, ns = _segments(segments)
        if ns != n:
            raise SessionError(f"limit_check: {n} limits over {ns} segments")
    rc = _ffi.load().vits_limit_check(_limits(limits, n), sarr, n)
    if rc != 0:
        raise SessionError(f"vits_limit_check failed [{rc}]: {_ffi.last_error(None)}")


def limit_gains(u, limit):
    """The gains of one segment whose unlimited values are u (float32 [c]) under `limit` (a Limit, or None: off) -> float32
    [c] (vits_limit_gains: pure host code, the rule written for clarity: c * lookahead steps)."""
    u = np.ascontiguousarray(u, np.float32)
    if u.ndim != 1:
        raise SessionError(f"u must be float32 [c], got {u.shape}")
    g = np.empty(u.shape, np.float32)
    arr = _limits(limit if isinstance(limit, RawLimits) else [limit], 1)
    rc = _ffi.load().vits_limit_gains(_ffi.ptr(u), u.size, arr, _ffi.ptr(g))
    if rc != 0:
        raise SessionError(f"vits_limit_gains failed [{rc}]: {_ffi.last_error(None)}")
    return g


def shape_check(shapes, n=None):
    """The validation of a shaped delivery's shapes (vits_shape_check: pure host code); a refusal raises SessionError."""
    if n is None:
        n = 1 if isinstance(shapes, Shape) else len(shapes.shapes if isinstance(shapes, RawShapes) else list(shapes))
    arr, points, n_points = _shapes(shapes, n)
    rc = _ffi.load().vits_shape_check(arr, n, points, n_points)
    if rc != 0:
        raise SessionError(f"vits_shape_check failed [{rc}]: {_ffi.last_error(None)}")


def shape_gain(shape, a, c, i):
    """The multiplier of row sample i of a segment with kept range [a, a + c) under `shape` (vits_shape_gain: pure host code)
    -> float32"""
    arr, points, _ = _shapes(shape, 1)
    mul = C.c_float()
    rc = _ffi.load().vits_shape_gain(arr, points, int(a), int(c), int(i), C.byref(mul))
    if rc != 0:
        raise SessionError(f"vits_shape_gain failed [{rc}]: {_ffi.last_error(None)}")
    return np.float32(mul.value)


def token_envelope(bounds, gains, ramp):
    """A per-token volume as breakpoints: bounds - int [T + 1], the tokens' boundaries in row samples at the delivered rate
    (build_alignments' rule: min(N, ceil(e * L / M))); gains - float32 [T], one linear gain per token; ramp - the samples a
    change of gain takes, centred on the boundary -> [(pos, gain)].
    Tokens of zero samples are skipped.  Every boundary s between consecutive non-empty tokens u, v with g_u != g_v gets
    h = min(ramp // 2, len_u // 2, len_v // 2) and the points (s - h, g_u), (s + h, g_v) - for h == 0: (s - 1, g_u), (s, g_v);
    a point whose pos equals the previous point's is dropped (it then has the same gain).  All gains equal to g != 1: the
    single point (0, g); all equal to 1: no points."""
    bounds = np.asarray(bounds, np.int64).ravel()
    gains = np.asarray(gains, np.float32).ravel()
    if bounds.size != gains.size + 1:
        raise SessionError(f"token_envelope: {gains.size} gains need {gains.size + 1} boundaries, got {bounds.size}")
    if (np.diff(bounds) < 0).any() or (bounds.size and bounds[0] < 0):
        raise SessionError("token_envelope: boundaries must be >= 0 and must not descend")
    ramp = int(ramp)
    if ramp < 0:
        raise SessionError(f"token_envelope: ramp {ramp} is negative")
    live = [t for t in range(gains.size) if bounds[t + 1] > bounds[t]]
    if not live:
        return []
    if all(gains[t] == gains[live[0]] for t in live):
        g = float(gains[live[0]])
        return [] if g == 1.0 else [(0, g)]
    points = []
    for u, v in zip(live[:-1], live[1:]):
        if gains[u] == gains[v]:
            continue
        s = int(bounds[v])
        h = min(ramp // 2, int(bounds[u + 1] - bounds[u]) // 2, int(bounds[v + 1] - bounds[v]) // 2)
        pair = ((s - h, gains[u]), (s + h, gains[v])) if h > 0 else ((s - 1, gains[u]), (s, gains[v]))
        for pos, g in pair:
            if not points or pos != points[-1][0]:
                points.append((pos, float(g)))
    return points


def token_bounds(durations, n_tokens, hop, count, ratio=None) -> np.ndarray:
    """The boundaries of one row's tokens in samples at the delivered rate: durations - the frames per token (a padded row is
    fine), n_tokens - the row's own tokens, count - the row's valid samples N, ratio - (L, M) of an output rate or None ->
    int64 [len(durations) + 1], by build_alignments' rule: the boundary at input sample e lies at min(N, ceil(e * L / M)),
    and at N behind the row's last token (the engine renders at least one frame)."""
    L, M = (int(v) for v in ratio) if ratio is not None else (1, 1)
    e = np.concatenate([[0], np.cumsum(np.asarray(durations, np.int64))]) * int(hop)
    bounds = np.minimum(int(count), -(-e * L // M))
    bounds[int(n_tokens):] = int(count)
    return bounds


def token_gain_shapes(segments, shapes, gains, bounds, ramp):
    """The shapes of a delivery with every segment's points set from the token gains of its row: gains float32 [B][T],
    bounds one token_bounds per row, ramp in samples - one value, or one per row where the rows are at rates of their own.
    A segment that already has points is refused."""
    out = []
    for i, (g, sh) in enumerate(zip(segments, shapes)):
        if len(sh.points):
            raise SessionError(f"segment {i}: token_gain_db and explicit points on the same segment")
        bd = bounds[int(g.row)]          # (a row's own tokens, or the padded row's: what lies behind them has no samples)
        rp = ramp[int(g.row)] if np.ndim(ramp) else ramp
        out.append(dataclasses.replace(sh, points=token_envelope(bd, gains[int(g.row)][:len(bd) - 1], rp)))
    return out


def token_gains(token_gain_db, B, T):
    """token_gain_db [B][T] in dB -> float32 [B, T] linear gains (float32(10 ** (dB / 20)); -inf: 0)"""
    try:
        db = np.asarray(token_gain_db, np.float64)
    except (TypeError, ValueError):
        raise SessionError(f"token_gain_db must be [{B}][{T}] numbers") from None
    if db.shape != (B, T):
        raise SessionError(f"token_gain_db must be [{B}][{T}], got {db.shape}")
    ok = (db == -np.inf) | (np.isfinite(db) & (db >= -120.0) & (db <= 36.0))
    if not ok.all():
        b, t = (int(v) for v in np.argwhere(~ok)[0])
        raise SessionError(f"token_gain_db[{b}][{t}] = {db[b, t]}: -inf, or within [-120, 36] dB")
    with np.errstate(over="ignore"):
        return np.where(db == -np.inf, 0.0, 10.0 ** (db / 20.0)).astype(np.float32)


def _n_streams(segments, n_streams):
    if n_streams is not None:
        return int(n_streams)
    return max([int(g.stream) for g in segments], default=0) + 1


def _plan_call(name, counts, segments, n_streams, encoding, arrays=(), rate=(), out=None):
    """One of the vits_delivery_plan* entries over counts int64 [B]: arrays - (marshaller, value) of what the entry takes
    between the segments and their count (trims, levels), rate - () or (sample_rate,), out - (stream_samples, stream_offsets)
    arrays to fill."""
    counts = np.ascontiguousarray(counts, np.int64)
    if counts.ndim != 1:
        raise SessionError(f"counts must be int64 [B], got {counts.shape}")
    segments = list(segments)
    code, _ = _encoding(encoding)
    J = _n_streams(segments, n_streams)
    arr, n = _segments(segments)
    samples, offsets = out if out is not None else (np.zeros(max(J, 0), np.int64), np.zeros(max(J, 0) + 1, np.int64))
    total = C.c_int64()
    rc = getattr(_ffi.load(), name)(_ffi.ptr(counts), counts.shape[0], arr, *[f(v, n) for f, v in arrays], n, J, code, *rate,
                                    _ffi.ptr(samples), _ffi.ptr(offsets), C.byref(total))
    if rc != 0:
        raise SessionError(f"{name} failed [{rc}]: {_ffi.last_error(None)}")
    return {"stream_samples": samples, "stream_offsets": offsets, "total_bytes": int(total.value)}


def delivery_plan(counts, segments, n_streams=None, encoding="pcm16", trims=None, kept=None):
    """The layout of a delivery (vits_delivery_plan: pure host code, no session, no device): counts int64 [B] - the rows' valid
    samples - and a plan -> {"stream_samples": int64 [J], "stream_offsets": int64 [J + 1] (bytes), "total_bytes": int}.
    A plan the engine would refuse raises SessionError with its message.  trims (one Trim or one per segment) and kept
    (int64 [B]: what a trimmed delivery keeps of each row, in the place of counts) give the layout of a trimmed delivery
    (vits_delivery_plan_trimmed)."""
    if trims is not None or kept is not None:
        return _plan_call("vits_delivery_plan_trimmed", counts if kept is None else kept, segments, n_streams, encoding,
                          arrays=((_trims, trims),))
    return _plan_call("vits_delivery_plan", counts, segments, n_streams, encoding)


def level_plan(counts, segments, levels, sample_rate, n_streams=None, encoding="pcm16", trims=None, out=None):
    """delivery_plan(..., kept=counts) with the levels' validation (vits_delivery_plan_leveled: pure host code).  The layout
    never depends on the levels.  out: (stream_samples, stream_offsets) arrays to fill; a refusal raises SessionError and
    leaves them untouched."""
    return _plan_call("vits_delivery_plan_leveled", counts, segments, n_streams, encoding, arrays=((_trims, trims), (_levels, levels)),
                      rate=(int(sample_rate),), out=out)


def loudness_filter(sample_rate):
    """The K-weighting of a rate (vits_loudness_filter: pure host code) -> (coef float64 [10]: shelf b0 b1 b2 a1 a2, high-pass
    b0 b1 b2 a1 a2; hop)"""
    coef, hop = np.zeros(10, np.float64), C.c_int32()
    rc = _ffi.load().vits_loudness_filter(int(sample_rate), _ffi.ptr(coef), C.byref(hop))
    if rc != 0:
        raise SessionError(f"vits_loudness_filter failed [{rc}]: {_ffi.last_error(None)}")
    return coef, hop.value


def loudness_gate(rows_e, hop):
    """The gates of BS.1770-4 over the sub-block energies of one or several rows, pooled (vits_loudness_gate: pure host code)
    -> (L, blocks, blocks past the absolute gate, blocks past both)"""
    rows_e = [np.ascontiguousarray(e, np.float32).ravel() for e in rows_e]
    n_sub = np.array([e.size for e in rows_e], np.int32)
    e = np.concatenate(rows_e) if rows_e else np.zeros(0, np.float32)
    L, nb, na, nr = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
    rc = _ffi.load().vits_loudness_gate(_ffi.ptr(e), _ffi.ptr(n_sub), len(rows_e), int(hop), C.byref(L), C.byref(nb), C.byref(na),
                                        C.byref(nr))
    if rc != 0:
        raise SessionError(f"vits_loudness_gate failed [{rc}]: {_ffi.last_error(None)}")
    return L.value, nb.value, na.value, nr.value


def level_gain(loudness, peak, level):
    """The gain of a segment of integrated loudness `loudness` (LUFS, -inf allowed) and sample peak `peak` under `level`
    (vits_level_gain: pure host code) -> float32"""
    g = C.c_float()
    lv = _levels(level, 1)
    rc = _ffi.load().vits_level_gain(float(loudness), float(peak), lv, C.byref(g))
    if rc != 0:
        raise SessionError(f"vits_level_gain failed [{rc}]: {_ffi.last_error(None)}")
    return np.float32(g.value)


@dataclass
class EncodedChunk:
    """One chunk of an encoded stream (vitsmi.h, "encoded streaming"): `data` [B, n] in the encoding's dtype - row b holds
    valid[b] encoded samples and silence behind them - covering samples [first_sample, first_sample + n) of the rows;
    peak[b]: the running max |x| of row b's valid samples so far (before any gain)."""
    first_sample: int
    data: np.ndarray
    valid: np.ndarray
    peak: np.ndarray
    total_samples: int
    # a trimmed stream (vitsmi.h, "trimmed streaming"): skip[b] leading elements of row b lie in front of the row's kept range -
    # the caller sends data[b, skip[b]:valid[b]]; None: the stream is not trimmed (nothing to skip)
    skip: Optional[np.ndarray] = None


def _stream_format(encoding, ref_peak, volume, B):
    """The vits_stream_format struct of an encoded stream: `ref_peak` / `volume` None, a scalar (every row) or [B] floats.
    Like _controls the struct holds the arrays it points into (`_keep`).  Returns (struct, dtype); raises SessionError naming
    the argument, the row and the value before anything reaches the handle (the engine checks the same once more)."""
    code, dtype = _encoding(encoding)
    fmt = _ffi.VitsStreamFormat()
    fmt.encoding = code
    keep = []
    for name, val in (("ref_peak", ref_peak), ("volume", volume)):
        if val is None:
            keep.append(None)
            continue
        try:
            arr = np.asarray(val, np.float32)
        except (TypeError, ValueError):
            raise SessionError(f"Unexpected input: '{name}' must be a float or floats of shape [batch_size]") from None
        if arr.shape not in ((), (B,)):
            raise SessionError(f"Invalid shape for '{name}': {arr.shape}, expected a scalar or [batch_size] = {(B,)}")
        arr = np.ascontiguousarray(np.broadcast_to(arr, (B,)), np.float32)
        ok = np.isfinite(arr) if name == "volume" else np.isfinite(arr) & (arr >= 0)
        bad = np.flatnonzero(~ok)
        if bad.size:
            what = "is not finite" if name == "volume" else "is not a finite value >= 0"
            raise SessionError(f"{name}[{int(bad[0])}]={float(arr[bad[0]])} {what}")
        keep.append(arr)
        setattr(fmt, name, arr.ctypes.data)
    fmt._keep = tuple(keep)
    return fmt, dtype


def _stream_limit(limit, B):
    """The limiter of a shaped stream: None, one Limit (every row) or one per row (None in the list: that row is not limited)
    -> (lookahead, ceilings float32 [B] or None).  One look-ahead per call keeps a chunk rectangular: limits that differ in
    it are refused."""
    if limit is None:
        return 0, None
    rows = [limit] * B if isinstance(limit, Limit) else list(limit)
    if len(rows) != B:
        raise SessionError(f"limit must be one Limit or one per row ({B}), got {len(rows)}")
    try:
        ahead = sorted({int(l.lookahead) for l in rows if l is not None})
        ceilings = np.array([0.0 if l is None else float(l.ceiling) for l in rows], np.float32)
    except (AttributeError, TypeError, ValueError, OverflowError) as e:
        raise SessionError(f"limit: {e}") from None
    if len(ahead) > 1:
        raise SessionError(f"limit: one lookahead per stream, got {ahead}")
    if not ahead:
        return 0, None
    for b, l in enumerate(rows):
        if l is not None and not ceilings[b] > 0:
            raise SessionError(f"row {b}: limit ceiling {float(l.ceiling)} is not finite and within (0, 1]")
    return ahead[0], ceilings


def _stream_shaping(shapes, limit, B):
    """The vits_stream_shaping struct of a shaped stream (vitsmi.h, "shaped streaming"), or None when neither is asked for:
    shapes - None, one Shape or one per row (or RawShapes); limit - as _stream_limit.  Like _stream_format the struct holds
    what it points into (`_keep`)."""
    if shapes is None and limit is None:
        return None
    shp = _ffi.VitsStreamShaping()
    keep = []
    if shapes is not None:
        arr, points, n_points = _shapes(shapes, B)
        keep += [arr, points]
        shp.shapes, shp.points, shp.n_points = C.addressof(arr), points, n_points
    if isinstance(limit, RawStreamLimit):
        ceilings = None if limit.ceiling is None else np.ascontiguousarray(limit.ceiling, np.float32)
        shp.lookahead = int(limit.lookahead)
    else:
        shp.lookahead, ceilings = _stream_limit(limit, B)
    if ceilings is not None:
        keep.append(ceilings)
        shp.ceiling = ceilings.ctypes.data
    shp._keep = keep
    return shp


# a stream's limiter as the C struct holds it, for the tests of the validation: lookahead, and ceiling [B] or None
RawStreamLimit = namedtuple("RawStreamLimit", "lookahead ceiling")

# a row's onset as the C struct holds it, for the tests of the validation
RawOnset = namedtuple("RawOnset", "mode threshold keep_lead reserved")


def _stream_onsets(onsets, B):
    """The vits_stream_onset array of a trimmed stream (vitsmi.h, "trimmed streaming"), or None: onsets - None, one Onset
    (every row) or one per row (None in the list: that row is not trimmed; RawOnset: the struct's four fields as they are)."""
    if onsets is None:
        return None
    rows = [onsets] * B if isinstance(onsets, (Onset, RawOnset)) else list(onsets)
    if len(rows) != B:
        raise SessionError(f"onsets must be one Onset or one per row ({B}), got {len(rows)}")
    arr = (_ffi.VitsStreamOnset * B)()
    for b, o in enumerate(rows):
        if o is None:
            continue
        try:
            arr[b].mode, arr[b].threshold, arr[b].keep_lead = int(o.mode), float(o.threshold), int(o.keep_lead)
            arr[b].reserved = int(getattr(o, "reserved", 0))
        except (AttributeError, TypeError, ValueError, OverflowError) as e:
            raise SessionError(f"row {b}: onset: {e}") from None
    return arr


def stream_onset_check(onsets, B=1, ref_peak=None):
    """The validation of a trimmed stream's onsets (vits_stream_onset_check: pure host code) over B rows, with or without a
    ref_peak; a refusal raises SessionError."""
    arr = _stream_onsets(onsets, B)
    fmt = _ffi.VitsStreamFormat()
    peak = None if ref_peak is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ref_peak, np.float32), (B,)), np.float32)
    if peak is not None:
        fmt.ref_peak = peak.ctypes.data
    rc = _ffi.load().vits_stream_onset_check(arr, C.byref(fmt), int(B))
    if rc != 0:
        raise SessionError(f"vits_stream_onset_check failed [{rc}]: {_ffi.last_error(None)}")


def stream_onset_start(f, keep_lead, delivered_before):
    """a_b of a row whose first active sample f lies in a piece that delivers from `delivered_before` on
    (vits_stream_onset_start: pure host code)."""
    a = C.c_int64()
    rc = _ffi.load().vits_stream_onset_start(int(f), int(keep_lead), int(delivered_before), C.byref(a))
    if rc != 0:
        raise SessionError(f"vits_stream_onset_start failed [{rc}]: {_ffi.last_error(None)}")
    return a.value


def stream_shaping_check(shapes=None, limit=None, B=1, volume=None):
    """The validation of a shaped stream's shaping (vits_stream_shaping_check: pure host code) over B rows of `volume` (None:
    the volumes are not looked at); a refusal raises SessionError."""
    shp = _stream_shaping(shapes, limit, B)
    fmt = None
    if volume is not None:
        fmt = _ffi.VitsStreamFormat()
        vol = np.ascontiguousarray(np.broadcast_to(np.asarray(volume, np.float32), (B,)), np.float32)
        fmt.volume = vol.ctypes.data
    rc = _ffi.load().vits_stream_shaping_check(None if shp is None else C.byref(shp), None if fmt is None else C.byref(fmt), int(B))
    if rc != 0:
        raise SessionError(f"vits_stream_shaping_check failed [{rc}]: {_ffi.last_error(None)}")


def stream_emit_range(first, n, is_last, total, lookahead):
    """What the rendered piece [first, first + n) of rows of `total` samples delivers under a look-ahead (vits_stream_emit_range:
    pure host code) -> (first, n) of the delivered range; n == 0: the piece completes nothing."""
    ef, en = C.c_int64(), C.c_int64()
    rc = _ffi.load().vits_stream_emit_range(int(first), int(n), int(bool(is_last)), int(total), int(lookahead), C.byref(ef), C.byref(en))
    if rc != 0:
        raise SessionError(f"vits_stream_emit_range failed [{rc}]: {_ffi.last_error(None)}")
    return ef.value, en.value


def _rows(scales, B):
    """[3] -> [B, 3] (the row twins of the C ABI take one row per utterance)"""
    return np.ascontiguousarray(np.broadcast_to(scales, (B, 3)) if scales.ndim == 1 else scales, np.float32)


def _part(scales, seeds, b0, b1):
    """The settings of rows [b0, b1) of a batch (a [3] vector is every part's)."""
    return (scales[b0:b1] if np.ndim(scales) == 2 else scales), (None if seeds is None else seeds[b0:b1])


def _device_settings(scales, B, seeds):
    """run_device's [B, 3] rows or seeds, checked like synthesize_batch's (float32: run_device always converted scales)."""
    return _settings(np.ascontiguousarray(scales, np.float32), B, seeds)


class MiSession:
    def __init__(self, path_or_bytes, sess_options=None, providers=None, provider_options=None, device_id: int = 0,
                 arena_device_ptr: Optional[int] = None, arena_bytes: int = 0, host_only: bool = False,
                 gen_precision: Optional[str] = None, range_fallback: bool = True, layout_only: bool = False,
                 pinned_results: bool = True, tails: Optional[str] = None, output_rate: Optional[int] = None,
                 pitch_at_rate: bool = False, **kwargs):
        """tails: what a padded batch (B > 1, unequal frame counts) holds behind each utterance's end - None (VITSMI_TAILS or
        the default "zero"), "zero" (those samples are not rendered at all and read 0.0; every valid sample is bit-identical to
        the padded rendering), "reference" (the exported graph's own padded rendering: its generator is not masked,
        models.py:348-368, so the tails are its response to zeros - what onnxruntime returns).  The reference calls the
        model with B = 1 only (voice.py:350-351), where the two are the same thing.
        gen_precision: arithmetic of the generator's convs - None (VITSMI_GEN_PRECISION or the default "f16x3"),
        "f16x3", "bf16x6" (exact products), "f16" (the reduced-precision vocoder of BASELINE config 4: fp16 storage, one
        fp16 product per fp32 product, fp32 accumulation).  range_fallback: on a RangeError of an fp16 arithmetic, reopen
        with "bf16x6" and repeat the call (never silently clamped audio).
        output_rate: None (the voice's own rate) or the sample rate in Hz every result is delivered at, resampled on the device
        (set_output_rate; vitsmi.h, "output rate").
        pitch_at_rate: True makes the pitched calls (token_semitones= / token_semitones_end=) take an output rate or per-row
        rates - the rate is folded into the warp's step on the device (set_pitch_at_rate; vitsmi.h, "pitch at an output rate");
        False, the default, keeps their refusal "not covered with an output rate set".
        pinned_results: run() / synthesize_batch() return arrays that VIEW page-locked host memory (the DMA engine's
        target; recycled when the array is garbage-collected).  An application that keeps many results alive thereby pins
        that much host RAM: pass False to get ordinary pageable arrays (one extra host copy per call).
        Thread safety: like onnxruntime's session.run, every entry point may be called from several threads; calls on one
        session are serialised by a per-session lock (a run is three C calls - enqueue, frame counts, copy-out - on one
        handle's workspace)."""
        import threading
        self._mu = threading.RLock()
        self.pinned_results = bool(pinned_results)
        if not isinstance(path_or_bytes, (str, bytes)) or isinstance(path_or_bytes, bytes):
            if isinstance(path_or_bytes, bytes):
                raise SessionError("MiSession loads a model from a file path, not from serialized bytes")
            path_or_bytes = str(path_or_bytes)
        self._lib = _ffi.load()
        self._h = C.c_void_p()
        self.path = path_or_bytes
        self.device_id = device_id
        self.host_only = host_only or layout_only
        self.range_fallback = bool(range_fallback) and arena_device_ptr is None
        self._open_args = dict(arena_device_ptr=arena_device_ptr, arena_bytes=arena_bytes, host_only=self.host_only,
                               layout_only=layout_only)
        if tails not in (None, "zero", "reference"):
            raise SessionError(f"tails must be None, 'zero' or 'reference' (got {tails!r})")
        self.tails = tails
        if output_rate is not None and (not isinstance(output_rate, (int, np.integer)) or output_rate <= 0):
            raise SessionError(f"output_rate must be None or a positive integer (got {output_rate!r})")
        self.output_rate = None if output_rate is None else int(output_rate)
        self.input_rate = None   # (None: the file's sample_rate metadata)
        self.output_rates = None  # (set_output_rates: a rate per row, in the place of output_rate)
        self.pitch_at_rate = bool(pitch_at_rate)
        self._seed = 0
        self.range_fallbacks = 0  # times this session reopened itself with bf16x6 after a RangeError (stats())
        self._open(gen_precision)

    def _open(self, gen_precision):
        a = self._open_args
        o = _ffi.VitsOpenOptions()
        o.device_id = self.device_id
        o.gen_precision = gen_precision.encode() if gen_precision else None
        o.arena_dev = a["arena_device_ptr"]
        o.arena_bytes = a["arena_bytes"] if a["arena_device_ptr"] is not None else 0
        o.host_only = 1 if a["host_only"] else 0
        o.layout_only = 1 if a["layout_only"] else 0
        h = C.c_void_p()
        rc = self._lib.vits_open_opts(self.path.encode(), C.byref(o), C.byref(h))
        if rc != 0:
            raise SessionError(f"vits_open({self.path!r}) failed [{rc}]: {_ffi.last_error(None)}")
        self._h = h
        self.gen_precision = gen_precision
        if self.tails is not None:
            self._lib.vits_set_tails(self._h, 1 if self.tails == "reference" else 0)
        if self.pitch_at_rate:  # (a reopened session keeps it)
            self._lib.vits_set_pitch_at_rate(self._h, 1)
        if self.output_rate is not None:
            rc = self._lib.vits_set_output_rate(self._h, self.input_rate or 0, self.output_rate)
            if rc != 0:
                msg = self._err()
                self.close()
                raise SessionError(f"vits_set_output_rate({self.input_rate}, {self.output_rate}) failed [{rc}]: {msg}")
        if self.output_rates is not None:  # (a reopened session keeps its row rates)
            arr = np.asarray(self.output_rates, np.int32)
            rc = self._lib.vits_set_output_rates(self._h, self.input_rate or 0, _ffi.ptr(arr), arr.size)
            if rc != 0:
                msg = self._err()
                self.close()
                raise SessionError(f"vits_set_output_rates({self.input_rate}, {self.output_rates}) failed [{rc}]: {msg}")
        n = self._lib.vits_num_inputs(self._h)
        self._input_names = [self._lib.vits_input_name(self._h, i).decode() for i in range(n)]

    def _raise(self, what, rc):
        cls = RangeError if rc == _ffi.VITS_E_RANGE else SessionError
        raise cls(f"{what} failed [{rc}]: {self._err()}")

    # How long a call from ANOTHER thread waits for a chunked run in progress before it gives up (a generator that was
    # neither exhausted nor closed keeps its run - and the session lock - until it is garbage-collected).
    busy_timeout_s = 120.0

    def _locked(self, read_only: bool = False):
        """The per-session lock, aware of chunked runs.  A chunked run holds the lock on its worker thread from the first
        chunk to the last, and the engine holds the handle's own mutex with it.  The CONSUMER of that generator must not
        block on either: its read-only calls (frame counts - valid from the first chunk on - and everything answered from
        host state) pass, anything that needs the handle raises instead of deadlocking.  Other threads wait for the run
        to end, for at most busy_timeout_s."""
        import contextlib
        import threading
        import time

        @contextlib.contextmanager
        def cm():
            owner = getattr(self, "_stream_owner", None)
            if owner is not None and owner == threading.get_ident():
                if read_only:
                    yield
                    return
                raise SessionError("a chunked run is in progress on this session (the synthesize_stream / vocoder_stream "
                                   "generator this thread is consuming): exhaust or close() it before other calls")
            deadline = None
            while not self._mu.acquire(timeout=0.25):
                if getattr(self, "_stream_owner", None) is None:
                    deadline = None      # an ordinary batch call of another thread: wait as long as it takes
                    continue
                now = time.monotonic()
                deadline = deadline or now + float(self.busy_timeout_s)
                if now > deadline:
                    raise SessionError(f"session busy: a chunked run has been in progress for more than "
                                       f"{self.busy_timeout_s:g} s (an unclosed synthesize_stream generator?)")
            try:
                yield
            finally:
                self._mu.release()
        return cm()

    def _fall_back_to_bf16x6(self, exc):
        """After a RangeError: reopen this voice with the exact six-product arithmetic (bf16 planes: fp32 range)."""
        import logging
        if not self.range_fallback or self.gen_precision == "bf16x6":  # (only fp16 planes raise it: encoder, flow, generator)
            raise exc
        logging.getLogger(__name__).warning("%s: %s - reopening with gen_precision='bf16x6' (1.8x slower; "
                                            "stats()['range_fallbacks'] counts these)", self.path, exc)
        self.close()
        self._open("bf16x6")
        self.range_fallbacks += 1

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.vits_close(self._h)
            self._h = C.c_void_p()
            try:
                _POOL.drain()   # dead result arrays of this session: back to the pool, the excess over its cap released
            except Exception:
                pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self):
        return _ffi.last_error(self._h)

    # ------------------------------------------------------------------ onnxruntime surface
    def get_inputs(self) -> List[NodeArg]:
        out = []
        for n in self._input_names:
            t, s = _INPUT_SPECS.get(n, ("tensor(int64)", ["batch_size"]))
            out.append(NodeArg(n, t, list(s)))
        return out

    def get_outputs(self) -> List[NodeArg]:
        return [NodeArg("output", "tensor(float)", ["batch_size", 1, 1, "time"])]

    def get_providers(self):
        return ["MI355XExecutionProvider"]

    def get_modelmeta(self) -> ModelMeta:
        keys = ("model_type", "n_speakers", "n_vocab", "sample_rate", "alphabet", "phoneme_type",
                "phonemizer_model", "phoneme_id_map", "has_espeak", "comment")
        return ModelMeta({k: v for k in keys if (v := self.meta(k)) is not None})

    def run(self, output_names: Optional[Sequence[str]], input_feed: Dict[str, np.ndarray], run_options=None):
        if output_names is not None and list(output_names) != ["output"]:
            raise SessionError(f"unknown output names {output_names!r}; the graph has one output 'output'")
        for k in input_feed:
            if k not in self._input_names:
                raise SessionError(f"Invalid input name: {k}")
        for k in self._input_names:
            if k not in input_feed:
                raise SessionError(f"Required input {k} is missing")
        if "langid" in input_feed:  # declared by the graph, consumed by nothing this engine runs: validate, then ignore
            lg = np.asarray(input_feed["langid"])
            if lg.dtype != np.int64 or lg.shape != (np.asarray(input_feed["input"]).shape[0],):
                raise SessionError("Unexpected input: 'langid' must be int64 of shape [batch_size]")
        scales = input_feed["scales"] if "scales" in self._input_names else np.array([0.667, 1.0, 0.8], np.float32)
        if np.shape(scales) != (3,):  # (the graph's declaration, get_inputs(); [B, 3] rows are synthesize_batch's extension)
            raise SessionError("Unexpected input: 'scales' must be float32 of shape [3]")
        out = self.synthesize_batch(input_feed["input"], input_feed["input_lengths"], scales, input_feed.get("sid"))
        return [out["output"]]

    # ------------------------------------------------------------------ extensions
    def set_seed(self, seed: int):
        """Seed of the device-side Philox stream that replaces the graph's two unseeded
        RandomNormalLike nodes (models.py:111, :718)."""
        self._seed = int(seed)

    def synthesize_batch(self, ids, lens, scales, sid=None, noise_dp=None, noise_z=None, taps=(), seeds=None,
                         durations=None, token_rate=None, return_durations=False, output_rates=None, token_semitones=None,
                         compensate=True, token_semitones_end=None, fit=None):
        """One batched run.  Returns {"output": [B,1,1,S] float32, "y_lengths": int64 [B], taps...}.
        output_rates: None, or a rate per row for this call (set_output_rates; what was set before is put back afterwards);
        with row rates the result also holds "sample_rates" (int32 [B]).
        With an output rate set (set_output_rate) "output" is the resampled waveform [B,1,1,S_out] and "sample_lengths"
        (int64 [B]) holds each row's valid samples at that rate; "y_lengths" stay frames.
        noise_dp [B,2,T] / noise_z [B,inter,>=F] inject the graph's noise for parity runs.
        scales: float32 [3] for every utterance, or [B, 3] - utterance b's own [noise_scale, length_scale, noise_w];
        seeds: None (the session's stream, set_seed) or B integers - utterance b's own noise stream, which does not
        depend on the rest of the batch (vitsmi.h, vits_run_async_rows).
        durations: None or integers [B, T] - forced frames per token: the duration predictor is not run, everything else is
        (with a free run's durations and seeds: that run's audio bit for bit); token_rate: None or floats [B, T] - a
        multiplier on each token's predicted duration (0 drops the token).  One or the other (vitsmi.h, vits_controls).
        return_durations: adds "durations", int64 [B, T] - the frames each token occupies (last_durations()).
        token_semitones: None or floats [B, T] within [-12, 12] - token t is raised or lowered by that many semitones, by a
        time warp on the device (vitsmi.h, "intonation": the resampling shift, formants move along); compensate=True keeps
        the tempo (the token is rendered longer by 2^(st/12) first), False is the pure warp.  The result then holds
        "sample_lengths" - each row's valid samples behind the warp - and, with return_durations, "token_spans" (int64
        [B, T]: the output samples of each token; "durations" stay the rendered frames).
        token_semitones_end: None or floats [B, T] within [-12, 12] - token t GLIDES from token_semitones[b, t] (zeros where
        that is None) to this value across its output samples (vitsmi.h, "pitch contours"); compensate=True renders it longer
        by the mean of 2^(st/12) at its two ends.  Equal ends everywhere are the token_semitones run, bit for bit.
        fit: None or a session.Fit - the durations of its groups of rows are rescaled on the device so that each group renders
        its target number of frames (vitsmi.h, "fitted durations"); the result then holds "fit_scale" (float64 [G]: the
        multiplier s*), "fit_frames" (int64 [G]: the frames achieved) and "fit_status" (int32 [G]: 0 met, 1 floor, 2 ceiling,
        3 kept).  Not together with durations or token_semitones (ValueError)."""
        ids, lens, scales, sid, noise_dp, noise_z, noise, seeds, durations, token_rate = self._run_arguments(
            ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate)
        B = ids.shape[0]
        semitones, semitones_end = _contour(token_semitones, token_semitones_end, lens, B, ids.shape[1])
        cfit = _fit(fit, B, self.hparam("hop"), durations, semitones)
        # enqueue -> frame counts -> copy-out -> taps all use this handle's one workspace
        with self._locked(), self._rates_for_call(output_rates):
            try:
                self._begin(ids, lens, scales, sid, noise, seeds, durations, token_rate, semitones, compensate, semitones_end, cfit)
                ylen = self.last_y_lengths()
                dur = self.last_durations() if return_durations else None
                fitted = self.last_fit() if cfit is not None else None
                counts = self.last_sample_counts() if self.resampling or self.output_rates is not None or semitones is not None else None
                spans = self._token_spans(semitones, lens, semitones_end) if return_durations and semitones is not None else None
                S = int(ylen.max()) * self.hparam("hop") if counts is None else int(counts.max())
                audio = _POOL.array((B, 1, 1, S)) if self.pinned_results else np.empty((B, 1, 1, S), np.float32)
                self._fetch(audio, 0, B)
            except RangeError as exc:
                self._fall_back_to_bf16x6(exc)
                return self.synthesize_batch(ids, lens, scales, sid, noise_dp, noise_z, taps, seeds=seeds,
                                             durations=durations, token_rate=token_rate, return_durations=return_durations,
                                             token_semitones=token_semitones, compensate=compensate,
                                             token_semitones_end=token_semitones_end, fit=fit)
            res = {"output": audio, "y_lengths": ylen}
            if fitted is not None:
                res["fit_scale"], res["fit_frames"], res["fit_status"] = fitted
            if counts is not None:
                res["sample_lengths"] = counts
            if self.output_rates is not None:
                res["sample_rates"] = self.last_sample_rates()
            if return_durations:
                res["durations"] = dur
            if spans is not None:
                res["token_spans"] = spans
            for t in taps:
                res[t] = self.tap(t)
            return res

    def _run_arguments(self, ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate):
        """The arguments of one batched run, validated and made contiguous (synthesize_batch, synthesize_delivered); the
        noise arrays are returned too: the VitsNoise struct only points into them."""
        ids = np.ascontiguousarray(ids)
        lens = np.ascontiguousarray(lens)
        if ids.dtype != np.int64 or lens.dtype != np.int64:
            raise SessionError("Unexpected input data type: 'input'/'input_lengths' must be tensor(int64)")
        if ids.ndim != 2 or lens.ndim != 1 or lens.shape[0] != ids.shape[0]:
            raise SessionError(f"Invalid rank/shape for input: {ids.shape} / input_lengths: {lens.shape}")
        B, T = ids.shape
        scales, seeds = _settings(scales, B, seeds)
        durations, token_rate = _timing(durations, token_rate, lens, B, T)
        if sid is not None:
            sid = np.ascontiguousarray(sid)
            if sid.dtype != np.int64 or sid.shape != (B,):
                raise SessionError("Unexpected input: 'sid' must be int64 of shape [batch_size]")
        if noise_dp is not None:
            noise_dp = np.ascontiguousarray(noise_dp, np.float32)
            if noise_dp.shape != (B, 2, T):
                raise SessionError(f"noise_dp must be [B,2,T], got {noise_dp.shape}")
        if noise_z is not None:
            noise_z = np.ascontiguousarray(noise_z, np.float32)
            if noise_z.ndim != 3 or noise_z.shape[0] != B or noise_z.shape[1] != self.hparam("inter"):
                raise SessionError(f"noise_z must be [B,inter,F], got {noise_z.shape}")
        return ids, lens, scales, sid, noise_dp, noise_z, _noise(self._seed, noise_dp, noise_z), seeds, durations, token_rate

    def _begin(self, ids, lens, scales, sid, noise, seeds=None, durations=None, token_rate=None, semitones=None, compensate=True,
               semitones_end=None, fit=None):
        """vits_run_async: validated host arrays in, the whole path enqueued; frame counts and durations are known on
        return.  ([B, 3] scales or seeds: vits_run_async_rows; durations or token_rate: vits_run_async_ctl; semitones:
        vits_run_async_warped; semitones_end too: vits_run_async_glided.)"""
        B, T = ids.shape
        head = (self._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T)
        rows = _rows(scales, B)
        ctl = _controls(rows, seeds, durations, token_rate)
        with_ctl = head + (_ffi.ptr(sid), C.byref(noise), C.byref(ctl))
        if fit is not None:  # (a vits_fit struct of _fit)
            rc = self._lib.vits_run_async_fitted(*with_ctl, C.byref(fit))
        elif semitones_end is not None:
            contour = _ffi.VitsContour(semitones.ctypes.data, semitones_end.ctypes.data, 1 if compensate else 0)
            rc = self._lib.vits_run_async_glided(*with_ctl, C.byref(contour))
        elif semitones is not None:
            into = _ffi.VitsIntonation(semitones.ctypes.data, 1 if compensate else 0)
            rc = self._lib.vits_run_async_warped(*with_ctl, C.byref(into))
        elif durations is not None or token_rate is not None:
            rc = self._lib.vits_run_async_ctl(*with_ctl)
        elif scales.ndim == 1 and seeds is None:
            rc = self._lib.vits_run_async(*head, _ffi.ptr(scales), _ffi.ptr(sid), C.byref(noise))
        else:
            rc = self._lib.vits_run_async_rows(*head, _ffi.ptr(rows), _ffi.ptr(sid), C.byref(noise), _ffi.ptr(seeds))
        if rc != 0:
            self._raise("vits_run", rc)

    def _fetch(self, out, row0, rows):
        """vits_fetch_output: this handle's [rows, S] waveform -> rows [row0, row0 + rows) of `out` [B,1,1,S_out]
        (pinned or pageable host memory), zero-filled past S.  Waits for the run."""
        S_out = out.shape[3]
        dst = out.ctypes.data + row0 * S_out * 4
        rc = self._lib.vits_fetch_output(self._h, C.c_void_p(dst), S_out, rows * S_out)
        if rc != 0:
            self._raise("vits_run", rc)
        if not self.pinned_results:
            _POOL.drain()   # (no pooled allocation will come along to do it)

    def vocoder(self, z, sid=None):
        z = np.ascontiguousarray(z, np.float32)
        B, Cc, F = z.shape
        if Cc != self.hparam("inter"):
            raise SessionError(f"z must have {self.hparam('inter')} channels")
        sid = None if sid is None else np.ascontiguousarray(sid, np.int64)
        out = _ffi.VitsOutput()
        with self._locked():
            rc = self._lib.vits_run_vocoder(self._h, _ffi.ptr(z), B, F, _ffi.ptr(sid), C.byref(out))
            if rc == _ffi.VITS_E_RANGE:
                try:
                    self._raise("vits_run_vocoder", rc)
                except RangeError as exc:
                    self._fall_back_to_bf16x6(exc)
                return self.vocoder(z, sid)
            if rc != 0:
                self._raise("vits_run_vocoder", rc)
            try:
                dims = tuple(out.dims[i] for i in range(4))
                return np.ctypeslib.as_array(out.data, shape=(int(np.prod(dims)),)).reshape(dims).copy()
            finally:
                self._lib.vits_free_output(self._h, C.byref(out))

    # ------------------------------------------------------------------ chunked (streaming) rendering, SURVEY §8 f1
    def _stream(self, start, wrap=None):
        """Run `start(callback)` (a blocking C call) on a worker thread and yield (first_sample, samples [B, n], total) as
        the engine hands chunks over: the consumer works on chunk i while chunk i + 1 renders.  `wrap` (callback type,
        function of the callback's arguments behind `user` -> the item to yield) replaces the fp32 chunk callback by
        another one; stop flag, bounded queue and lock ownership are the same for both."""
        import queue
        import threading
        if getattr(self, "_stream_owner", None) == threading.get_ident():
            raise SessionError("a chunked run is already in progress on this session in this thread: exhaust or close() "
                               "its generator first")
        q = queue.Queue(maxsize=2)  # the engine renders at most two chunks ahead of the consumer
        stop = threading.Event()

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return
                except queue.Full:
                    pass

        def fp32_chunk(samples, B, first, n, total):
            return int(first), np.ctypeslib.as_array(samples, shape=(B * n,)).reshape(B, n).copy(), int(total)

        fn_type, item_of = wrap if wrap is not None else (_ffi.CHUNK_FN, fp32_chunk)

        @fn_type
        def on_chunk(user, *args):
            if stop.is_set():
                return 1  # the consumer is gone: end the run (vits_chunk_fn's "stop" return)
            put(item_of(*args))
            return 1 if stop.is_set() else 0

        def work():
            # the session lock is held for the whole chunked run (taken on THIS thread: an RLock belongs to the thread that
            # acquired it): a batch call from another thread then waits instead of running between this run's chunks on the
            # same workspace - and returning this run's frame counts and audio as its own
            try:
                with self._mu:
                    self._stream_owner = consumer
                    try:
                        rc = start(on_chunk)
                        err = None if rc == 0 or stop.is_set() else (rc, self._err())
                    finally:
                        self._stream_owner = None
                put(err)
            except BaseException as e:  # noqa: BLE001 - re-raised on the consumer's thread
                put(e)

        # (the consumer = the thread that iterates this generator: its frame-count queries pass the lock, see _locked)
        consumer = threading.get_ident()
        t = threading.Thread(target=work, daemon=True)
        t.start()
        try:
            while True:
                item = q.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                if isinstance(item, tuple) and len(item) == 2:
                    cls = RangeError if item[0] == _ffi.VITS_E_RANGE else SessionError
                    raise cls(f"chunked run failed [{item[0]}]: {item[1]}")
                yield item
        finally:
            # generator closed early (break / GeneratorExit) or failed: tell the engine to stop after the chunk in
            # flight, so that the handle's mutex is released and the next call does not queue behind a dead render
            stop.set()
            t.join()

    def synthesize_stream(self, ids, lens, scales, sid=None, chunk_frames: int = 64, noise_dp=None, noise_z=None,
                          seeds=None, durations=None, token_rate=None, token_semitones=None, compensate=True,
                          token_semitones_end=None, fit=None):
        """The whole path with the waveform delivered in chunks of `chunk_frames` frames (hop samples each): yields
        (first_sample, float32 [B, n], total_samples).  Concatenated, the chunks are bit-identical to
        synthesize_batch(...)["output"][:, 0, 0, :]; frame counts afterwards from last_y_lengths().  Chunks are handed out
        as they finish, so a range violation of the f16x3 arithmetic cannot be repaired by a silent re-run: it raises
        RangeError at the end (no bf16x6 fallback here; reopen with gen_precision="bf16x6").  Closing the generator
        early stops the engine after the chunk in flight.  scales [3] or [B, 3], seeds, durations and token_rate as
        synthesize_batch.  The consumer may call last_durations() - like last_y_lengths() - from the first chunk on: the
        timing of the whole utterance is known before most of its audio exists.
        token_semitones, compensate, token_semitones_end - as synthesize_batch (vitsmi.h, "streamed pitch"): the chunks, joined,
        are that run's warped "output"; their ranges lie on the warped timeline and follow what the rows' plans have completed -
        a chunk of the run may deliver nothing, or several ranges -, total_samples is the longest warped row, and
        last_sample_counts() / last_token_spans() answer from the first chunk on.  Not covered with an output rate set, unless
        the session was opened with pitch_at_rate (set_pitch_at_rate): then one rate is folded into the warp (vitsmi.h, "pitch at
        an output rate") and the chunks are that run's at the rate; a rate per row stays refused.
        fit - as synthesize_batch (vitsmi.h, "fitted durations"): the chunks, joined, are the fitted run's "output"; last_fit()
        answers from the first chunk on.  Not together with durations or token_semitones (ValueError)."""
        ids, lens, scales, seeds, sid, noise, ctl, on_top, _, _ = self._stream_arguments(
            "synthesize_stream", ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate, token_semitones,
            compensate, token_semitones_end, fit)
        B, T = ids.shape

        def start(cb):
            def call(name, *args):
                return getattr(self._lib, name)(self._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, *args, int(chunk_frames), cb, None)
            if on_top is not None:
                return call("vits_run_chunked" + on_top[0], _ffi.ptr(sid), C.byref(noise), C.byref(ctl), C.byref(on_top[1]))
            if ctl.durations or ctl.token_rate:
                return call("vits_run_chunked_ctl", _ffi.ptr(sid), C.byref(noise), C.byref(ctl))
            if scales.ndim == 1 and seeds is None:
                return call("vits_run_chunked", _ffi.ptr(scales), _ffi.ptr(sid), C.byref(noise))
            return call("vits_run_chunked_rows", ctl.scales_rows, _ffi.ptr(sid), C.byref(noise), _ffi.ptr(seeds))

        return self._stream(start)

    def _stream_arguments(self, name, ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate, token_semitones,
                          compensate, token_semitones_end, fit):
        """The arguments that synthesize_stream and synthesize_stream_encoded (`name`) share, validated and made contiguous -
        the C call runs on _stream's worker thread after the method has returned: every host array it reads must belong to
        its closure, the converted ones ride on the struct that points into them (`_keep`).  `on_top`: None, or what goes on
        top of the controls as (the suffix of the entry that takes it, the struct) - ("_fitted", vits_fit) or ("_glided",
        vits_contour); behind it the (start, end) semitones of _contour."""
        ids = np.ascontiguousarray(ids, np.int64)
        lens = np.ascontiguousarray(lens, np.int64)
        B, T = ids.shape
        semitones, semitones_end = _contour(token_semitones, token_semitones_end, lens, B, T)
        scales, seeds = _settings(np.ascontiguousarray(scales, np.float32), B, seeds)
        durations, token_rate = _timing(durations, token_rate, lens, B, T)
        cfit = _fit(fit, B, self.hparam("hop"), durations, semitones)
        sid = None if sid is None else np.ascontiguousarray(sid, np.int64)
        noise = _noise(self._seed, noise_dp, noise_z)
        ctl = _controls(_rows(scales, B), seeds, durations, token_rate)
        on_top = None if cfit is None else ("_fitted", cfit)
        if semitones is not None:  # (never with a fit: _fit has refused that)
            self._pitch_admit(name, durations, compensate, semitones, semitones_end, lens)
            contour = _ffi.VitsContour(semitones.ctypes.data, None if semitones_end is None else semitones_end.ctypes.data,
                                       1 if compensate else 0)
            contour._keep = (semitones, semitones_end)
            on_top = ("_glided", contour)
        return ids, lens, scales, seeds, sid, noise, ctl, on_top, semitones, semitones_end

    @staticmethod
    def _encoded_items(dtype):
        """_stream's `wrap` of an encoded run: the callback type and the EncodedChunk of one call - `data` is a copy cut from
        the pitched rows (the engine's buffer is only valid during the call)."""
        width = np.dtype(dtype).itemsize

        def item(data, B, pitch, first, n, valid, peak, total):
            raw = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), shape=(B * pitch,)).reshape(B, pitch)
            rows = np.array(raw[:, :n * width]).view(dtype).reshape(B, n)   # (np.array: a copy also where the pitch is n * width)
            return EncodedChunk(int(first), rows, np.ctypeslib.as_array(valid, shape=(B,)).copy(),
                                np.ctypeslib.as_array(peak, shape=(B,)).copy(), int(total))

        return _ffi.ENC_CHUNK_FN, item

    @staticmethod
    def _trimmed_items(dtype):
        """_encoded_items for a trimmed run: the callback with the rows' skips"""
        _, plain = MiSession._encoded_items(dtype)

        def item(data, B, pitch, first, n, valid, skip, peak, total):
            chunk = plain(data, B, pitch, first, n, valid, peak, total)
            chunk.skip = np.ctypeslib.as_array(skip, shape=(B,)).copy()
            return chunk

        return _ffi.ENC_CHUNK_TRIM_FN, item

    def _onsets_check(self, onsets, fmt, B):
        """onsets the engine would refuse up front raise here, by the call itself: nothing was started"""
        if self._lib.vits_stream_onset_check(onsets, C.byref(fmt), B) != 0:
            raise SessionError(f"trimmed stream refused: {_ffi.last_error(None)}")

    def synthesize_stream_encoded(self, ids, lens, scales, sid=None, chunk_frames: int = 64, encoding="pcm16", ref_peak=None,
                                  volume=None, noise_dp=None, noise_z=None, seeds=None, durations=None, token_rate=None,
                                  shapes=None, token_gain_db=None, gain_ramp=0.01, limit=None, onsets=None, token_semitones=None,
                                  compensate=True, token_semitones_end=None, fit=None):
        """synthesize_stream with every chunk post-processed, encoded and masked to each row's own length on the device
        (vitsmi.h, "encoded streaming"): yields EncodedChunk.  encoding "pcm16" / "ulaw" / "alaw" / "f32"; `volume` and
        `ref_peak` None, a scalar or [B]: row b is scaled by volume[b] and - with ref_peak - normalised by ref_peak[b] (a
        stream cannot know its own peak: feed back the final `peak` of an earlier stream with the same seeds, or a
        calibrated one).  The same chunk ranges as synthesize_stream, at the session's output rate; each row's valid
        elements, joined, are what deliver() gives for that row (normalize 0, or 1 with ref_peak = its peak).
        shapes (one Shape or one per row), token_gain_db ([B][T] dB, with gain_ramp seconds around every change) and limit
        (one Limit, or one per row with None for a row that is not limited; one lookahead for all) are those of
        synthesize_delivered(shapes=, token_gain_db=, gain_ramp=, limits=) for segments that keep their whole rows (vitsmi.h,
        "shaped streaming"): each row's valid elements, joined, are what that delivery gives - a fade-out ends at the row's
        own end, and with a look-ahead of L samples every chunk is delivered L samples late (the first chunk is L shorter,
        the last L longer; EncodedChunk.peak then runs up to L samples ahead of the audio).  token_gain_db places its
        breakpoints on the token boundaries of THIS run - free or forced durations - inside the engine's plan callback,
        before the first chunk is rendered.
        onsets (one Onset or one per row, None for a row that is not trimmed) cuts the leading silence of every row on the
        device (vitsmi.h, "trimmed streaming"): EncodedChunk.skip[b] elements of row b lie in front of its kept range; fades
        and limiter count from there, and data[b, skip[b]:valid[b]], joined, is what the delivery gives under the equivalent
        Trim.  The chunk ranges do not change.
        token_semitones, compensate, token_semitones_end - as synthesize_stream (vitsmi.h, "streamed pitch"): everything above
        then works on the warped audio - valid counts, fades and the limiter by each row's warped length, token_gain_db's
        breakpoints on the warp's own token spans -, and every chunk carries `skip` (zeros without onsets): data[b,
        skip[b]:valid[b]], joined, is what synthesize_delivered(token_semitones=...) gives for the row.
        fit - as synthesize_batch (vitsmi.h, "fitted durations"): everything above then works on the fitted run - joined, the
        rows are what synthesize_delivered(fit=...) gives -, every chunk carries `skip` (zeros without onsets), and last_fit()
        answers from the first chunk on.  Not together with durations or token_semitones (ValueError)."""
        ids, lens, _, _, sid, noise, ctl, on_top, semitones, semitones_end = self._stream_arguments(
            "synthesize_stream_encoded", ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate, token_semitones,
            compensate, token_semitones_end, fit)
        B, T = ids.shape
        fmt, dtype = _stream_format(encoding, ref_peak, volume, B)
        shaping = self._stream_plan(shapes, token_gain_db, gain_ramp, limit, lens, B, T, semitones, semitones_end)
        suffix, rest, wrap = self._encoded_entry(fmt, dtype, shaping, _stream_onsets(onsets, B), B, on_top)
        return self._stream(lambda cb: getattr(self._lib, "vits_run_chunked_enc" + suffix)(
            self._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(sid), C.byref(noise), C.byref(ctl), C.byref(fmt), *rest,
            int(chunk_frames), cb, None), wrap)

    def _encoded_entry(self, fmt, dtype, shaping, trim, B, on_top=None):
        """Which encoded entry a stream reaches - whole path or vocoder -, after the pre-checks of what it passes down: (the
        entry's suffix, its arguments between the format and chunk_frames, _stream's `wrap`).  on_top as _stream_arguments
        makes it; those entries and the trimmed one hand out chunks with `skip`."""
        if shaping is not None:
            self._shaping_check(shaping, fmt, B)
        if trim is not None:
            self._onsets_check(trim, fmt, B)
        rest = (None if shaping is None else C.byref(shaping), trim)
        if on_top is not None:
            return on_top[0], rest + (C.byref(on_top[1]),), self._trimmed_items(dtype)
        if trim is not None:  # (passed down only when asked for)
            return "_trimmed", rest, self._trimmed_items(dtype)
        if shaping is None:  # (nothing asked for: the call made before there was any shaping)
            return "", (), self._encoded_items(dtype)
        return "_shaped", rest[:1], self._encoded_items(dtype)

    def _pitch_admit(self, name, durations, compensate, semitones, semitones_end, lens):
        """what the engine refuses of a stream with pitch, raised by the call itself: nothing was started (all zeros: the
        unwarped stream, which refuses nothing)"""
        if not _pitched(semitones, semitones_end, lens):
            return
        if (self.resampling or self.output_rates is not None) and not self.pitch_at_rate:
            raise SessionError(f"{name}(token_semitones=...) is not covered with an output rate set")
        if self.output_rates is not None:  # (one output rate is folded into the warp: vitsmi.h, "pitch at an output rate")
            raise SessionError(f"{name}(token_semitones=...) is not covered with an output rate set per row")
        if self.resampling:
            fi = self.input_rate or int(self.meta("sample_rate") or 22050)
            L, M = resample_plan(fi, self.output_rate)[:2]
            if M > 4 * L or L > 4 * M:
                raise SessionError(f"{name}(token_semitones=...): pitch at {fi} -> {self.output_rate} Hz is not covered: the ratio of the "
                                   "rates lies outside [1/4, 4]")
        if compensate and durations is not None:
            raise SessionError("compensate and forced durations are contradictory: forced durations are the rendered ones")

    def _shaping_check(self, shaping, fmt, B):
        """a shaping the engine would refuse up front raises here, by the call itself: nothing was started"""
        if self._lib.vits_stream_shaping_check(C.byref(shaping), C.byref(fmt), B) != 0:
            raise SessionError(f"shaped stream refused: {_ffi.last_error(None)}")

    def _stream_plan(self, shapes, token_gain_db, gain_ramp, limit, lens, B, T, semitones=None, semitones_end=None):
        """_stream_shaping with the plan callback of a per-token volume: the callback builds every row's envelope from the
        run's own durations and sample counts (token_bounds / token_envelope: what synthesize_delivered(token_gain_db=)
        computes between its run and its delivery) and hands the engine the shapes that carry them."""
        if token_gain_db is None:
            return _stream_shaping(shapes, limit, B)
        tgains = token_gains(token_gain_db, B, T)
        if not (np.isfinite(gain_ramp) and gain_ramp >= 0):
            raise SessionError(f"gain_ramp must be >= 0 seconds (got {gain_ramp})")
        base = [Shape()] * B if shapes is None else ([shapes] * B if isinstance(shapes, Shape) else list(shapes))
        if len(base) != B:
            raise SessionError(f"shapes must be one Shape or one per row ({B}), got {len(base)}")
        for i, sh in enumerate(base):
            if len(sh.points):
                raise SessionError(f"row {i}: token_gain_db and explicit points on the same row")
        shaping = _stream_shaping(base, limit, B)
        hop = self.hparam("hop")
        ratio = None
        if self.resampling:
            ratio = resample_plan(self.input_rate or int(self.meta("sample_rate") or 22050), self.output_rate)[:2]
        ramp = int(self.delivered_rate * float(gain_ramp))
        keep = shaping._keep
        pitched = _pitched(semitones, semitones_end, lens)

        @_ffi.STREAM_PLAN_FN
        def plan(user, Bc, Tc, dur, counts, inout):
            try:
                d = np.ctypeslib.as_array(dur, shape=(Bc * Tc,)).reshape(Bc, Tc)
                n = np.ctypeslib.as_array(counts, shape=(Bc,))
                if pitched:  # the boundaries are the warp's: the host plan over THIS run's durations (counts are its N_b)
                    bounds = [token_span_bounds(_pitched_spans(d[b, :lens[b]], semitones[b, :lens[b]],
                                                               None if semitones_end is None else semitones_end[b, :lens[b]], hop, ratio),
                                                  n[b]) for b in range(Bc)]
                else:
                    bounds = [token_bounds(d[b], lens[b], hop, n[b], ratio) for b in range(Bc)]
                used = token_gain_shapes([Segment(b) for b in range(Bc)], base, tgains, bounds, ramp)
                arr, points, n_points = _shapes(used, Bc)
                keep.extend([arr, points])
                shaping.used_shapes = used
                inout.contents.shapes, inout.contents.points, inout.contents.n_points = C.addressof(arr), points.value, n_points
                return 0
            except Exception as e:  # noqa: BLE001 - a Python error must not cross the C frames: the run is refused instead
                shaping.plan_error = e
                return 1

        shaping.plan = plan
        keep.append(plan)
        return shaping

    def vocoder_stream_encoded(self, z, sid=None, chunk_frames: int = 64, encoding="pcm16", ref_peak=None, volume=None, shapes=None,
                               limit=None, onsets=None):
        """Vocoder only, chunked and encoded: yields EncodedChunk (every row has F * hop samples, or their count at the
        output rate).  shapes / limit / onsets as synthesize_stream_encoded."""
        z = np.ascontiguousarray(z, np.float32)
        B, Cc, F = z.shape
        fmt, dtype = _stream_format(encoding, ref_peak, volume, B)
        shaping = _stream_shaping(shapes, limit, B)
        if Cc != self.hparam("inter"):
            raise SessionError(f"z must have {self.hparam('inter')} channels")
        sid = None if sid is None else np.ascontiguousarray(sid, np.int64)
        suffix, rest, wrap = self._encoded_entry(fmt, dtype, shaping, _stream_onsets(onsets, B), B)
        return self._stream(lambda cb: getattr(self._lib, "vits_run_vocoder_chunked_enc" + suffix)(
            self._h, _ffi.ptr(z), B, F, _ffi.ptr(sid), C.byref(fmt), *rest, int(chunk_frames), cb, None), wrap)

    def vocoder_stream(self, z, sid=None, chunk_frames: int = 64):
        """Vocoder only, chunked: yields (first_sample, float32 [B, n], total_samples)."""
        z = np.ascontiguousarray(z, np.float32)
        B, Cc, F = z.shape
        if Cc != self.hparam("inter"):
            raise SessionError(f"z must have {self.hparam('inter')} channels")
        sid = None if sid is None else np.ascontiguousarray(sid, np.int64)
        return self._stream(lambda cb: self._lib.vits_run_vocoder_chunked(self._h, _ffi.ptr(z), B, F, _ffi.ptr(sid),
                                                                          int(chunk_frames), cb, None))

    def tap(self, name):
        with self._locked():  # (two C calls on the last run's workspace)
            dims = (C.c_int64 * 4)()
            nd = self._lib.vits_tap(self._h, name.encode(), None, 0, dims)
            if nd < 0:
                raise SessionError(f"vits_tap({name}) failed: {self._err()}")
            shape = tuple(dims[i] for i in range(nd))
            buf = np.empty(shape, np.float32)
            nd = self._lib.vits_tap(self._h, name.encode(), _ffi.ptr(buf), buf.size, dims)
            if nd < 0:
                raise SessionError(f"vits_tap({name}) failed: {self._err()}")
            return buf

    def meta(self, key):
        buf = C.create_string_buffer(1 << 16)
        n = self._lib.vits_meta(self._h, key.encode(), buf, len(buf))
        return None if n < 0 else buf.value.decode()

    def hparam(self, key) -> int:
        v = C.c_int64()
        if self._lib.vits_hparam(self._h, key.encode(), C.byref(v)) != 0:
            raise SessionError(self._err())
        return v.value

    def set_tails(self, tails: str):
        """"zero" / "reference": see the constructor (applies to the following runs)."""
        if tails not in ("zero", "reference"):
            raise SessionError(f"tails must be 'zero' or 'reference' (got {tails!r})")
        with self._locked():
            self.tails = tails
            self._lib.vits_set_tails(self._h, 1 if tails == "reference" else 0)

    def set_output_rate(self, rate: Optional[int], input_rate: Optional[int] = None):
        """Deliver the following runs' audio at `rate` Hz, resampled on the device (vitsmi.h, "output rate"): batch results,
        device PCM and stream chunks alike.  None switches it off; `input_rate` None means the file's sample_rate metadata
        (22050 without it).  A rate equal to the input rate is the native path, bit for bit.  Kept across a bf16x6 fallback."""
        if rate is not None and (not isinstance(rate, (int, np.integer)) or rate <= 0):
            raise SessionError(f"output rate must be None or a positive integer (got {rate!r})")
        if input_rate is not None and (not isinstance(input_rate, (int, np.integer)) or input_rate <= 0):
            raise SessionError(f"input rate must be None or a positive integer (got {input_rate!r})")
        with self._locked():
            rc = self._lib.vits_set_output_rate(self._h, int(input_rate or 0), int(rate or 0))
            if rc != 0:
                self._raise("vits_set_output_rate", rc)
            self.output_rate = None if rate is None else int(rate)
            self.input_rate = None if input_rate is None else int(input_rate)
            self.output_rates = None  # (a handle rate, or none, replaces a rate per row)

    def set_pitch_at_rate(self, on: bool = True):
        """Whether the pitched calls take an output rate or per-row rates (vits_set_pitch_at_rate; vitsmi.h, "pitch at an output
        rate"): on, the rate is folded into the warp's step - one filter pass, token spans in delivered samples -; off, the
        default, they are refused with "not covered with an output rate set"."""
        with self._locked():
            rc = self._lib.vits_set_pitch_at_rate(self._h, 1 if on else 0)
            if rc != 0:
                self._raise("vits_set_pitch_at_rate", rc)
            self.pitch_at_rate = bool(on)

    def set_output_rates(self, rates, input_rate: Optional[int] = None):
        """Deliver row b of the following runs at rates[b] Hz (vitsmi.h, "output rate per row"): one entry per row of the
        run - None, 0 or the input rate for a native row -, at most 8 distinct resampling rates.  Row b of such a run is row b
        of the same run under set_output_rate(rates[b]), bit for bit.  It replaces set_output_rate's rate (and that call
        replaces this); None clears it.  The following runs must have exactly len(rates) rows; the chunked entries
        (stream*, synthesize_chunked) are refused while it is set.  A refused call leaves the previous setting in place."""
        if input_rate is not None and (not isinstance(input_rate, (int, np.integer)) or input_rate <= 0):
            raise SessionError(f"input rate must be None or a positive integer (got {input_rate!r})")
        if rates is None:
            with self._locked():
                rc = self._lib.vits_set_output_rates(self._h, 0, None, 0)
                if rc != 0:
                    self._raise("vits_set_output_rates", rc)
                self.output_rates = None
            return
        rates = list(rates)
        for b, r in enumerate(rates):
            if r is not None and (not isinstance(r, (int, np.integer)) or r < 0):
                raise SessionError(f"row {b}: output rate must be None or an integer >= 0 (got {r!r})")
        if not rates:
            raise SessionError("output rates must be None or one rate per row (got none)")
        arr = np.asarray([int(r or 0) for r in rates], np.int32)
        with self._locked():
            rc = self._lib.vits_set_output_rates(self._h, int(input_rate or 0), _ffi.ptr(arr), arr.size)
            if rc != 0:
                self._raise("vits_set_output_rates", rc)
            self.output_rates = tuple(int(v) for v in arr)
            self.output_rate = None
            self.input_rate = None if input_rate is None else int(input_rate)

    def last_sample_rates(self) -> np.ndarray:
        """int32 [B]: the rate each row of the last run was delivered at (vits_last_sample_rates; host state)."""
        with self._locked(read_only=True):
            n = self._lib.vits_last_sample_rates(self._h, None, 0)
            buf = np.zeros(max(n, 0), np.int32)
            if n > 0:
                self._lib.vits_last_sample_rates(self._h, _ffi.ptr(buf), n)
            return buf

    @contextlib.contextmanager
    def _rates_for_call(self, output_rates):
        """output_rates= of one call: set for it, then what was set before is put back (None: nothing happens)"""
        if output_rates is None:
            yield
            return
        before = (self.output_rate, self.output_rates, self.input_rate)
        self.set_output_rates(output_rates, self.input_rate)
        try:
            yield
        finally:
            if before[1] is not None:
                self.set_output_rates(before[1], before[2])
            else:
                self.set_output_rate(before[0], before[2])

    def _row_ratios(self, B):
        """(L, M) per row of a run under the rates that are set - None for a row that is not resampled"""
        fi = self.input_rate or int(self.meta("sample_rate") or 22050)
        if self.output_rates is not None:
            return [None if r in (0, fi) else resample_plan(fi, r)[:2] for r in self.output_rates]
        return [resample_plan(fi, self.output_rate)[:2] if self.resampling else None] * B

    @property
    def resampling(self) -> bool:
        """An output rate is set and differs from the input rate: results are resampled."""
        if self.output_rate is None:
            return False
        fi = self.input_rate or int(self.meta("sample_rate") or 22050)
        return fi != self.output_rate

    def last_sample_counts(self) -> np.ndarray:
        """int64 [B]: the valid samples of each row of the last run at the current output rate (y_lengths * hop with the
        rate off).  From host state like last_y_lengths(): no wait, and a stream's consumer may call it."""
        with self._locked(read_only=True):
            n = self._lib.vits_last_sample_counts(self._h, None, 0)
            buf = np.zeros(max(n, 0), np.int64)
            if n > 0:
                self._lib.vits_last_sample_counts(self._h, buf.ctypes.data_as(C.POINTER(C.c_int64)), n)
            return buf

    def reserve(self, batch: int, tokens: int = 0, frames: int = 0):
        """Size the device workspaces now for requests of up to `batch` utterances x `tokens` ids rendering up to `frames`
        frames each (vits_reserve): a serving process calls this once at start-up with the largest request it admits, so that
        no request reallocates tens of GB mid-stream (a device-wide synchronisation measured at up to seconds)."""
        with self._locked():
            if self._lib.vits_reserve(self._h, int(batch), int(tokens), int(frames)) != 0:
                raise SessionError(self._err())

    def set_timing(self, on=True):
        """True / 1: stage marks + events around every conv launch; 2: stage marks only; False / 0: off."""
        self._lib.vits_set_timing(self._h, 2 if on == 2 else (1 if on else 0))

    def stats(self):
        s = _ffi.VitsStats()
        with self._locked():
            self._lib.vits_get_stats(self._h, C.byref(s))
        d = {k: getattr(s, k) for k, _ in _ffi.VitsStats._fields_}
        d["range_fallbacks"] = self.range_fallbacks
        return d

    def launch_records(self):
        """Per conv-engine launch of the last run made with set_timing(True) (call stats() first: it reads the events):
        [{"kernel", "ms", "flops", "bytes", "stage"}] in launch order."""
        n = self._lib.vits_launch_records(self._h, None, 0)
        if n <= 0:
            return []
        buf = (_ffi.VitsLaunchRecord * n)()
        self._lib.vits_launch_records(self._h, buf, n)
        return [{"kernel": r.kernel.decode(), "ms": r.ms, "flops": r.flops, "bytes": r.bytes, "stage": r.stage,
                 "cin": r.cin, "cout": r.cout, "k": r.k, "dil": r.dil, "t": r.t} for r in buf]

    def arena_bytes(self):
        return self._lib.vits_arena_bytes(self._h)

    def arena_host(self) -> np.ndarray:
        n = self.arena_bytes()
        p = self._lib.vits_arena_host(self._h)
        if not p:
            raise SessionError("this handle holds no host copy of the weight arena (opened with a device arena / layout only)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,))

    def arena_device(self) -> int:
        return self._lib.vits_arena_device(self._h) or 0

    def stream(self) -> int:
        return self._lib.vits_stream(self._h) or 0

    # device-resident run for the benchmark / sharded path: arguments are device pointers (ints)
    def run_device(self, ids_ptr, lens_ptr, B, T, scales, sid_ptr=None, noise_dp_ptr=None, noise_z_ptr=None,
                   noise_z_stride=0, seeds=None):
        """scales: host float32 [3] or [B, 3]; seeds: None or B host integers (as synthesize_batch)."""
        scales = np.ascontiguousarray(scales, np.float32)
        noise = _ffi.VitsNoise()
        noise.seed = self._seed
        noise.noise_dp = noise_dp_ptr
        noise.noise_z = noise_z_ptr
        noise.noise_z_stride = noise_z_stride
        out = _ffi.VitsOutput()
        if scales.ndim == 1 and seeds is None:
            rc = self._lib.vits_run_device(self._h, C.c_void_p(ids_ptr), C.c_void_p(lens_ptr), B, T, _ffi.ptr(scales),
                                           C.c_void_p(sid_ptr) if sid_ptr else None, C.byref(noise), C.byref(out))
        else:
            scales, seeds = _device_settings(scales, B, seeds)
            rows = _rows(scales, B)
            rc = self._lib.vits_run_device_rows(self._h, C.c_void_p(ids_ptr), C.c_void_p(lens_ptr), B, T, _ffi.ptr(rows),
                                                C.c_void_p(sid_ptr) if sid_ptr else None, C.byref(noise), _ffi.ptr(seeds),
                                                C.byref(out))
        if rc != 0:
            self._raise("vits_run_device", rc)
        dims = tuple(out.dims[i] for i in range(4))
        return {"data_ptr": C.cast(out.data, C.c_void_p).value, "dims": dims,
                "y_lengths_ptr": C.cast(out.y_lengths, C.c_void_p).value}

    def last_y_lengths(self) -> np.ndarray:
        with self._locked(read_only=True):  # (size, then contents: both of the same run; host state of the handle)
            n = self._lib.vits_last_y_lengths(self._h, None, 0)
            buf = np.zeros(max(n, 0), np.int64)
            if n > 0:
                self._lib.vits_last_y_lengths(self._h, buf.ctypes.data_as(C.POINTER(C.c_int64)), n)
            return buf

    def last_durations(self) -> np.ndarray:
        """int64 [B, T]: the frames each token of the last run occupies (w_ceil of models.py:702-704; forced runs: the
        forced values; 0 behind lens[b]); max(1, row sums) = last_y_lengths().  Answered from host state like
        last_y_lengths(): no wait, valid as soon as the run has been enqueued, and the consumer of synthesize_stream may
        call it while chunks are still rendering."""
        with self._locked(read_only=True):
            n = self._lib.vits_last_durations(self._h, None, 0)
            if n < 0:
                raise SessionError(f"vits_last_durations failed [{n}]: {self._err()}")
            B = self._lib.vits_last_y_lengths(self._h, None, 0)
            buf = np.zeros((B, n // B), np.int64)
            n = self._lib.vits_last_durations(self._h, buf.ctypes.data_as(C.POINTER(C.c_int64)), buf.size)
            if n != buf.size:
                raise SessionError(f"vits_last_durations: the run changed between two calls ({n} != {buf.size})")
            return buf

    def last_fit(self):
        """(scale float64 [G], frames int64 [G], status int32 [G]) of the last FITTED run: per group the multiplier s*, the
        frames achieved and the status (0 met, 1 floor, 2 ceiling, 3 kept).  Host state like last_durations(): valid from
        the first chunk of a stream on.  SessionError after a run that was not fitted."""
        with self._locked(read_only=True):
            G = self._lib.vits_last_fit(self._h, None, None, None, 0)
            if G < 0:
                raise SessionError(f"vits_last_fit failed [{G}]: {self._err()}")
            scale, frames, status = np.zeros(G, np.float64), np.zeros(G, np.int64), np.zeros(G, np.int32)
            if self._lib.vits_last_fit(self._h, _ffi.ptr(scale), _ffi.ptr(frames), _ffi.ptr(status), G) != G:
                raise SessionError("vits_last_fit: the run changed between two calls")
            return scale, frames, status

    def last_token_spans(self) -> np.ndarray:
        """int64 [B, T]: the output samples each token of the last WARPED run occupies (k of the warp's plan; 0 for a dropped
        token and behind lens[b]); row sums = last_sample_counts().  Host state like last_durations().  SessionError after a
        run that was not warped."""
        with self._locked(read_only=True):
            n = self._lib.vits_last_token_spans(self._h, None, 0)
            if n < 0:
                raise SessionError(f"vits_last_token_spans failed [{n}]: {self._err()}")
            B = self._lib.vits_last_y_lengths(self._h, None, 0)
            buf = np.zeros((B, n // B), np.int64)
            n = self._lib.vits_last_token_spans(self._h, buf.ctypes.data_as(C.POINTER(C.c_int64)), buf.size)
            if n != buf.size:
                raise SessionError(f"vits_last_token_spans: the run changed between two calls ({n} != {buf.size})")
            return buf

    def _token_spans(self, semitones, lens, semitones_end=None) -> np.ndarray:
        """the spans of the last run, begun with `semitones` (and the glides' end values): the warp's, or - every semitone 0,
        the run was not warped - what the identity plan gives: durations * hop"""
        live = np.arange(semitones.shape[1])[None, :] < np.asarray(lens)[:, None]
        if (live & ((semitones != 0) if semitones_end is None else ((semitones != 0) | (semitones_end != 0)))).any():
            return self.last_token_spans()
        return self.last_durations() * self.hparam("hop")

    def last_pcm16(self, normalize: bool = True, volume: float = 1.0, shape=None) -> np.ndarray:
        """int16 PCM of the last run, post-processed on the GPU exactly as TTSVoice.synthesize + AudioChunk do
        (voice.py:271-282, 88-91); [B, S], zeros past each utterance's length."""
        if shape is None:
            raise SessionError("last_pcm16 needs the [B, S] shape of the last output")
        out = np.zeros(shape, np.int16)
        with self._locked():
            rc = self._lib.vits_last_pcm16(self._h, 1 if normalize else 0, float(volume), _ffi.ptr(out), out.size)
        if rc != 0:
            raise SessionError(f"vits_last_pcm16 failed [{rc}]: {self._err()}")
        return out

    def synthesize_batch_pcm16(self, ids, lens, scales, sid=None, normalize: bool = True, volume: float = 1.0):
        """One batched run whose result leaves the GPU as 16-bit PCM only: peak-normalise / volume / clip / int16
        happen on the device (bit-identical to TTSVoice._postprocess + AudioChunk), the fp32 waveform is never
        copied to the host.  Returns (pcm int16 [B, S], y_lengths int64 [B]); with an output rate set (set_output_rate)
        (pcm int16 [B, S_out] of the resampled waveform, sample_lengths int64 [B])."""
        ids = np.ascontiguousarray(ids, np.int64)
        lens = np.ascontiguousarray(lens, np.int64)
        scales = np.ascontiguousarray(scales, np.float32)
        if ids.ndim != 2 or lens.shape != (ids.shape[0],) or scales.shape != (3,):
            raise SessionError(f"Invalid rank/shape for input: {ids.shape} / input_lengths: {lens.shape}")
        B, T = ids.shape
        if sid is not None:
            sid = np.ascontiguousarray(sid, np.int64)
        noise = _noise(self._seed)
        with self._locked():
            rc = self._lib.vits_run(self._h, _ffi.ptr(ids), _ffi.ptr(lens), B, T, _ffi.ptr(scales), _ffi.ptr(sid),
                                    C.byref(noise), None)
            if rc != 0:
                raise SessionError(f"vits_run failed [{rc}]: {self._err()}")
            if self.resampling:
                counts = self.last_sample_counts()
                return self.last_pcm16(normalize, volume, shape=(B, int(counts.max()))), counts
            ylen = self.last_y_lengths()
            S = int(ylen.max()) * self.hparam("hop")
            return self.last_pcm16(normalize, volume, shape=(B, S)), ylen

    @property
    def delivered_rate(self) -> int:
        """The sample rate results are delivered at: the output rate, or the voice's own."""
        return int(self.output_rate or self.input_rate or self.meta("sample_rate") or 22050)

    def deliver(self, segments, n_streams=None, encoding="pcm16", trims=None, return_kept=False, levels=None, sample_rate=None,
                return_levels=False, shapes=None, limits=None):
        """The last run's audio, post-processed, encoded and laid out per request on the device (vitsmi.h, "delivery"):
        segments - Segment objects, each row of the run in at most one; encoding "pcm16" / "ulaw" / "alaw" / "f32".  Returns
        one NumPy array per stream (int16 / uint8 / float32), all views into ONE buffer in stream order - page-locked memory
        from the pool when pinned_results.  The fp32 waveform stays on the device; tap / last_pcm16 / a fetch of the same run
        still work afterwards, and so does another deliver() with another plan.
        trims - one Trim or one per segment (vitsmi.h, "trimmed delivery"): every row is cut to its kept range on the device
        and followed by its tail of silence.  return_kept=True: (streams, kept_first int64 [G], kept_count int64 [G]).
        The layout of a trimmed delivery depends on the data, so its ONE buffer is sized before the scan, by the untrimmed
        layout plus the tails (one call and one scan instead of two): the views returned keep a buffer alive that is larger
        than what was delivered by what was trimmed - copy them if that matters.
        levels - one Level or one per segment (vitsmi.h, "levelled delivery"): the integrated loudness of every levelled
        segment's kept range is measured on the device and the segment delivered at its target; sample_rate - the rate the
        audio is at (default: delivered_rate; refused where it differs from a set output rate).  return_levels=True appends
        (loudness float64 [G] - NaN for an unlevelled segment, -inf below 400 ms or the gates -, gain float32 [G]).
        shapes - one Shape or one per segment (vitsmi.h, "shaped delivery"): fades at either end of what is kept of a segment
        and a piecewise-linear volume over its row, applied by the pack launch; peaks, trim scan and loudness see the
        unshaped audio, and the layout does not depend on the shapes.
        limits - one Limit or one per segment, None for a segment without one (vitsmi.h, "limited delivery"): a look-ahead
        peak limiter as the last stage in front of the clip; peaks, trim scan and loudness see the unlimited audio, and the
        layout does not depend on the limits."""
        segments = list(segments)
        code, dtype = _encoding(encoding)
        J = _n_streams(segments, n_streams)
        arr, n = _segments(segments)
        samples, offsets = np.zeros(max(J, 0), np.int64), np.zeros(max(J, 0) + 1, np.int64)
        plain = trims is None and levels is None and shapes is None and limits is None and not return_kept and not return_levels
        tarr = larr = sarr = parr = first = count = loud = gain = None  # (a plain delivery has none of them and pays for none)
        marr = _limits(limits, n)
        n_points = rate = tails = 0
        if not plain:
            tarr, larr = _trims(trims, n), _levels(levels, n)
            sarr, parr, n_points = _shapes(shapes, n)
            if levels is not None:  # (only a levelled delivery looks at the rate: 0 elsewhere, which nothing refuses)
                rate = self.delivered_rate if sample_rate is None else int(sample_rate)
                if sample_rate is None and self.output_rates is not None and segments:
                    # (a rate per row: the rate of the first segment's row - the engine refuses a levelled segment at another)
                    rates = self.last_sample_rates()
                    if 0 <= int(segments[0].row) < rates.size:
                        rate = int(rates[int(segments[0].row)])
            # (what the caller does not want back is not reported: NULL, the engine's own "none")
            if return_kept:
                first, count = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
            if return_levels:
                loud, gain = np.full(max(n, 1), np.nan, np.float64), np.ones(max(n, 1), np.float32)
            if tarr:
                tails = np.dtype(dtype).itemsize * sum(max(int(tarr[i].tail_samples), 0) for i in range(n))
        with self._locked():
            # the untrimmed layout (dst = NULL: no device work, no wait) and the tails bound the bytes: ONE delivery, one scan
            rc = self._lib.vits_deliver(self._h, arr, n, J, code, None, 0, _ffi.ptr(samples), _ffi.ptr(offsets))
            if rc != 0:
                self._raise("vits_deliver", rc)
            cap = int(offsets[-1]) + tails
            buf = _POOL.array((cap,), np.uint8) if self.pinned_results and cap else np.empty(cap, np.uint8)
            if plain:
                rc = self._lib.vits_deliver(self._h, arr, n, J, code, _ffi.ptr(buf), cap, _ffi.ptr(samples), _ffi.ptr(offsets))
            elif marr is None:  # (vits_deliver_trimmed and vits_deliver_leveled are this entry with NULLs)
                rc = self._lib.vits_deliver_shaped(self._h, arr, tarr, larr, sarr, parr, n_points, n, J, code, rate, _ffi.ptr(buf), cap,
                                                   _ffi.ptr(samples), _ffi.ptr(offsets), _ffi.ptr(first), _ffi.ptr(count),
                                                   _ffi.ptr(loud), _ffi.ptr(gain))
            else:
                rc = self._lib.vits_deliver_limited(self._h, arr, tarr, larr, sarr, parr, n_points, marr, n, J, code, rate, _ffi.ptr(buf),
                                                    cap, _ffi.ptr(samples), _ffi.ptr(offsets), _ffi.ptr(first), _ffi.ptr(count),
                                                    _ffi.ptr(loud), _ffi.ptr(gain))
            if rc != 0:
                self._raise("vits_deliver" if plain else ("vits_deliver_shaped" if marr is None else "vits_deliver_limited"), rc)
        streams = [buf[int(offsets[j]):int(offsets[j + 1])].view(dtype) for j in range(J)]
        if not (return_kept or return_levels):
            return streams
        return (streams,) + ((first[:n], count[:n]) if return_kept else ()) + ((loud[:n], gain[:n]) if return_levels else ())

    def deliver_layout(self, segments, n_streams=None, encoding="pcm16", trims=None):
        """What deliver(..., trims=) would return, without the bytes (vits_deliver_trimmed with dst = NULL: waits for the run
        and runs the scan, packs and copies nothing): {"stream_samples", "stream_offsets", "kept_first", "kept_count"}."""
        segments = list(segments)
        code, _ = _encoding(encoding)
        J = _n_streams(segments, n_streams)
        arr, n = _segments(segments)
        samples, offsets = np.zeros(max(J, 0), np.int64), np.zeros(max(J, 0) + 1, np.int64)
        first, count = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        with self._locked():
            rc = self._lib.vits_deliver_trimmed(self._h, arr, _trims(trims, n), n, J, code, None, 0, _ffi.ptr(samples),
                                                _ffi.ptr(offsets), _ffi.ptr(first), _ffi.ptr(count))
            if rc != 0:
                self._raise("vits_deliver_trimmed", rc)
        return {"stream_samples": samples, "stream_offsets": offsets, "kept_first": first[:n], "kept_count": count[:n]}

    def synthesize_delivered(self, ids, lens, scales, sid=None, *, segments=None, n_streams=None, encoding="pcm16",
                             normalize=True, volume=1.0, seeds=None, durations=None, token_rate=None, noise_dp=None,
                             noise_z=None, return_durations=False, trim=None, levels=None, shapes=None, token_gain_db=None,
                             gain_ramp=0.01, limits=None, output_rates=None, token_semitones=None, compensate=True,
                             token_semitones_end=None, fit=None):
        """One batched run and its delivery under one hold of the session lock: what leaves the GPU is the encoded audio
        of the plan and nothing else - the fp32 waveform is never copied to the host.  segments=None: one stream per row,
        with `normalize` / `volume` as scalars or [B] arrays (row b's own).  Everything in front of the delivery is
        synthesize_batch's (scales [3] or [B, 3], seeds, durations, token_rate, injected noise, the bf16x6 fallback).
        trim - one Trim or one per segment: deliver(..., trims=trim).  levels - one Level or one per segment:
        deliver(..., levels=levels); the result then holds "loudness" (float64 [G]) and "gain" (float32 [G]) too.
        shapes - one Shape or one per segment: deliver(..., shapes=shapes).  token_gain_db - [B][T], a volume in dB per token of
        every row (-inf: silent; else within [-120, 36]): between the run and the delivery it becomes breakpoints of the
        segment on that row - token_envelope over the tokens' boundaries at the delivered rate (last_durations(), the hop, the
        output-rate ratio) with gains float32(10 ** (dB / 20)) and a ramp of int(delivered_rate * gain_ramp) samples around
        every change.  No second run, no waveform on the host.  A segment with explicit points AND token gains is refused.
        With either, the result holds "shapes": the Shape every segment was delivered with.
        limits - one Limit or one per segment (None in the list: off): deliver(..., limits=limits).
        output_rates - None, or a rate per row for this call (set_output_rates; what was set before is put back afterwards).
        With row rates set, by this argument or before, `encoding` may also be one name per segment; the run is then
        delivered once per (rate, encoding) group of segments - a stream's segments must lie in one group -, every
        sample-valued field (leads, Trim, Shape, Limit) is at its row's own rate, gain_ramp is converted at each row's rate,
        and the result holds "sample_rates" (int32 [B]).
        token_semitones, compensate - as synthesize_batch: the delivery then works on the warped waveform and its counts; the
        token gains' breakpoints lie on the warp's own token spans, and with return_durations the result holds "token_spans".
        token_semitones_end - as synthesize_batch: the tokens glide ("pitch contours"); everything behind the run is the same.
        fit - as synthesize_batch ("fitted durations"): the run is fitted, everything behind it is the same, and the result
        holds "fit_scale", "fit_frames" and "fit_status".
        Returns {"streams": [array per stream], "stream_samples": int64 [J], "y_lengths": int64 [B], "sample_lengths":
        int64 [B] (each row's valid samples at the delivered rate), "kept_first" / "kept_count": int64 [G] (what each
        segment delivers of its row: all of it without a trim)[, "durations"]}."""
        ids, lens, scales, sid, noise_dp, noise_z, noise, seeds, durations, token_rate = self._run_arguments(
            ids, lens, scales, sid, noise_dp, noise_z, seeds, durations, token_rate)
        B = ids.shape[0]
        semitones, semitones_end = _contour(token_semitones, token_semitones_end, lens, B, ids.shape[1])
        cfit = _fit(fit, B, self.hparam("hop"), durations, semitones)
        if segments is None:
            try:
                nz = np.broadcast_to(np.asarray(normalize, bool), (B,))
                vol = np.broadcast_to(np.asarray(volume, np.float32), (B,))
            except ValueError:
                raise SessionError(f"normalize / volume must be scalars or [{B}] arrays") from None
            segments = [Segment(b, b, 0, 1 if nz[b] else 0, float(vol[b])) for b in range(B)]
            n_streams = B
        segments = list(segments)
        if isinstance(encoding, str):
            _encoding(encoding)
        else:
            encoding = list(encoding)
            if len(encoding) != len(segments):
                raise SessionError(f"encoding must be one name or one per segment ({len(segments)}), got {len(encoding)}")
            for e in encoding:
                _encoding(e)
            if output_rates is None and self.output_rates is None:
                raise SessionError("an encoding per segment needs a rate per row (output_rates=, set_output_rates)")
        used = None
        if shapes is not None or token_gain_db is not None:
            used = [Shape()] * len(segments) if shapes is None else ([shapes] * len(segments) if isinstance(shapes, Shape) else list(shapes))
            if len(used) != len(segments):
                raise SessionError(f"shapes must be one Shape or one per segment ({len(segments)}), got {len(used)}")
        tgains = None
        if token_gain_db is not None:
            tgains = token_gains(token_gain_db, B, ids.shape[1])
            if not (np.isfinite(gain_ramp) and gain_ramp >= 0):
                raise SessionError(f"gain_ramp must be >= 0 seconds (got {gain_ramp})")
            for i, sh in enumerate(used):
                if len(sh.points):
                    raise SessionError(f"segment {i}: token_gain_db and explicit points on the same segment")
        with self._locked(), self._rates_for_call(output_rates):
            try:
                self._begin(ids, lens, scales, sid, noise, seeds, durations, token_rate, semitones, compensate, semitones_end, cfit)
                ylen = self.last_y_lengths()
                dur = self.last_durations() if return_durations or tgains is not None else None
                fitted = self.last_fit() if cfit is not None else None
                counts = self.last_sample_counts()
                rates = self.last_sample_rates() if self.output_rates is not None else None
                spans = self._token_spans(semitones, lens, semitones_end) if semitones is not None and (return_durations or tgains is not None) else None
                loud = gain = None
                if tgains is not None:
                    used = self._token_shapes(segments, used, tgains, dur, lens, counts, gain_ramp, spans)
                if rates is not None:
                    streams, kept_first, kept_count, loud, gain = self._deliver_groups(segments, n_streams, encoding, rates, counts,
                                                                                       trim, levels, used, limits)
                elif used is None and levels is None and trim is None and limits is None:
                    streams = self.deliver(segments, n_streams, encoding)
                    kept_first = np.zeros(len(segments), np.int64)
                    kept_count = np.array([counts[int(g.row)] for g in segments], np.int64)
                else:
                    streams, kept_first, kept_count, *lv = self.deliver(segments, n_streams, encoding, trims=trim, return_kept=True,
                                                                        levels=levels, return_levels=levels is not None, shapes=used,
                                                                        limits=limits)
                    loud, gain = lv or (None, None)
            except RangeError as exc:
                self._fall_back_to_bf16x6(exc)
                return self.synthesize_delivered(ids, lens, scales, sid, segments=segments, n_streams=n_streams,
                                                 encoding=encoding, seeds=seeds, durations=durations, token_rate=token_rate,
                                                 noise_dp=noise_dp, noise_z=noise_z, return_durations=return_durations,
                                                 trim=trim, levels=levels, shapes=shapes, token_gain_db=token_gain_db,
                                                 gain_ramp=gain_ramp, limits=limits, token_semitones=token_semitones,
                                                 compensate=compensate, token_semitones_end=token_semitones_end, fit=fit)
        res = {"streams": streams, "stream_samples": np.array([a.size for a in streams], np.int64), "y_lengths": ylen,
               "sample_lengths": counts, "kept_first": kept_first, "kept_count": kept_count}
        if levels is not None:
            res["loudness"], res["gain"] = loud, gain
        if rates is not None:
            res["sample_rates"] = rates
        if used is not None:
            res["shapes"] = used
        if fitted is not None:
            res["fit_scale"], res["fit_frames"], res["fit_status"] = fitted
        if return_durations:
            res["durations"] = dur
            if spans is not None:
                res["token_spans"] = spans
        return res

    def _deliver_groups(self, segments, n_streams, encoding, rates, counts, trims, levels, shapes, limits):
        """The last run - one with a rate per row - delivered once per (rate, encoding) group of segments, in the order the
        groups first appear: a levelled delivery measures at ONE rate and a delivery has one encoding.  Returns (streams [J],
        kept_first [G], kept_count [G], loudness [G] or None, gain [G] or None) in the caller's numbering."""
        G = len(segments)
        encs = [encoding] * G if isinstance(encoding, str) else list(encoding)

        def per_segment(v, cls, name):
            if v is None:
                return None
            v = [v] * G if isinstance(v, cls) else list(v)
            if len(v) != G:
                raise SessionError(f"{name} must be one {cls.__name__} or one per segment ({G}), got {len(v)}")
            return v

        trims, levels = per_segment(trims, Trim, "trims"), per_segment(levels, Level, "levels")
        shapes, limits = per_segment(shapes, Shape, "shapes"), per_segment(limits, Limit, "limits")
        J = _n_streams(segments, n_streams)
        keys, of_stream = [], {}
        for i, g in enumerate(segments):
            if not 0 <= int(g.row) < len(rates):
                raise SessionError(f"segment {i}: row {int(g.row)} outside [0, {len(rates)})")
            if not 0 <= int(g.stream) < J:
                raise SessionError(f"segment {i}: stream {int(g.stream)} outside [0, {J})")
            keys.append((int(rates[int(g.row)]), encs[i]))
            if of_stream.setdefault(int(g.stream), keys[i]) != keys[i]:
                raise SessionError(f"segment {i}: stream {int(g.stream)} would hold audio at {keys[i][0]} Hz as {keys[i][1]} behind "
                                   f"audio at {of_stream[int(g.stream)][0]} Hz as {of_stream[int(g.stream)][1]}")
        plain = trims is None and levels is None and shapes is None and limits is None
        streams = [np.zeros(0, np.uint8)] * J
        kept_first = np.zeros(G, np.int64)
        kept_count = np.array([counts[int(g.row)] for g in segments], np.int64)
        loud = gain = None
        if levels is not None:
            loud, gain = np.full(G, np.nan, np.float64), np.ones(G, np.float32)
        for key in dict.fromkeys(keys):
            idx = [i for i in range(G) if keys[i] == key]
            local = {}
            for i in idx:
                local.setdefault(int(segments[i].stream), len(local))
            sub = [dataclasses.replace(segments[i], stream=local[int(segments[i].stream)]) for i in idx]
            pick = lambda v: None if v is None else [v[i] for i in idx]  # noqa: E731
            if plain:
                ss = self.deliver(sub, len(local), key[1])
            else:
                ss, kf, kc, *lv = self.deliver(sub, len(local), key[1], trims=pick(trims), return_kept=True, levels=pick(levels),
                                               sample_rate=key[0], return_levels=levels is not None, shapes=pick(shapes),
                                               limits=pick(limits))
                kept_first[idx], kept_count[idx] = kf, kc
                if lv:
                    loud[idx], gain[idx] = lv
            for j, k in local.items():
                streams[j] = ss[k]
        return streams, kept_first, kept_count, loud, gain

    def _token_shapes(self, segments, shapes, gains, durations, lens, counts, gain_ramp, spans=None):
        """the shapes of a delivery of the last run with every segment's points set from its row's token gains (spans: the
        token spans of a run begun with semitones - its boundaries are the warp's)"""
        hop = self.hparam("hop")
        ratios = self._row_ratios(len(lens))
        if spans is not None:
            bounds = [token_span_bounds(spans[b], counts[b]) for b in range(len(lens))]
        else:
            bounds = [token_bounds(durations[b], lens[b], hop, counts[b], ratios[b]) for b in range(len(lens))]
        if self.output_rates is None:
            return token_gain_shapes(segments, shapes, gains, bounds, int(self.delivered_rate * float(gain_ramp)))
        # (a rate per row: the ramp, given in seconds, at each row's own)
        return token_gain_shapes(segments, shapes, gains, bounds, [int(int(r) * float(gain_ramp)) for r in self.last_sample_rates()])

    def sync(self):
        with self._locked():
            rc = self._lib.vits_sync(self._h)
            if rc != 0:
                self._raise("vits_sync", rc)


class PipelinedSession:
    """A batch rendered as `parts` sub-batches on `parts` engine handles (= HIP streams) that share ONE weight
    arena.  The encoder / duration / flow stages of a sub-batch have small grids that leave most of the chip idle;
    on separate streams they overlap with another sub-batch's generator (measured on one MI355X at batch 32 x 256
    ids: +3.5 % on the LJSpeech-size voice, +9 % on the default one; more than 2 parts loses).  Utterances are
    independent, so every sub-batch is an ordinary run and results are those of `MiSession` on the same rows
    (device noise streams differ per part: seed + part index)."""

    def __init__(self, first: MiSession, parts: int = 2):
        if parts < 1:
            raise SessionError("parts must be >= 1")
        if getattr(first, "output_rate", None) is not None:
            raise SessionError("PipelinedSession runs the device-pointer entries, which do not resample: the session has an "
                               f"output rate set ({first.output_rate} Hz); call set_output_rate(None) first")
        if getattr(first, "output_rates", None) is not None:
            raise SessionError("PipelinedSession runs the device-pointer entries, which do not resample: the session has "
                               f"per-row output rates set ({list(first.output_rates)}); call set_output_rates(None) first")
        self.parts = [first]
        # `first` owns the weight arena the other handles borrow: it must never close and reopen itself under them
        # (MiSession's own fallback would free the arena while the borrowers run on it).  The fallback happens HERE,
        # for all handles together (_fall_back).
        import threading
        self._mu = threading.RLock()   # one batched call at a time per pipeline (its parts' locks are taken inside)
        self.range_fallback = first.range_fallback
        self._first_had_fallback = first.range_fallback   # handed back by close()
        first.range_fallback = False
        self.range_fallbacks = 0
        self._n_parts = parts
        self._borrow()
        self.set_seed(first._seed)

    def _borrow(self):
        """(Re)create the handles that share parts[0]'s arena (laid out for ITS arithmetic)."""
        first = self.parts[0]
        # the arithmetic the owner was opened with, as it was asked for: the layout of every split-operand conv (encoder,
        # flow, generator) follows the request, also where this voice's generator cannot use that engine
        precision = first.gen_precision
        for _ in range(self._n_parts - 1):
            self.parts.append(MiSession(first.path, device_id=first.device_id, arena_device_ptr=first.arena_device(),
                                        arena_bytes=first.arena_bytes(), gen_precision=precision, tails=first.tails))

    def _fall_back(self, exc):
        """After a RangeError on any part: every borrower is synchronised and closed, THEN the owner reopens with the
        six-product arithmetic (bf16 planes: fp32 range), then the borrowers are recreated on the new arena."""
        import logging
        first = self.parts[0]
        if not self.range_fallback or first.gen_precision == "bf16x6":
            raise exc
        logging.getLogger(__name__).warning("%s: %s - reopening all %d handles with gen_precision='bf16x6'", first.path, exc,
                                            len(self.parts))
        for s in reversed(self.parts[1:]):
            try:
                s.sync()
            except SessionError:
                pass
            s.close()
        del self.parts[1:]
        try:
            first.sync()
        except SessionError:
            pass
        seed = first._seed
        first.close()
        first._open("bf16x6")
        first.range_fallbacks += 1
        self.range_fallbacks += 1
        self._borrow()
        self.set_seed(seed)

    @classmethod
    def open(cls, path, device_id: int = 0, parts: int = 2):
        return cls(MiSession(path, device_id=device_id), parts)

    def set_seed(self, seed: int):
        for i, s in enumerate(self.parts):
            s.set_seed(int(seed) + i)

    def reserve(self, batch: int, tokens: int = 0, frames: int = 0, whole_batch: bool = True):
        """MiSession.reserve on every part.  whole_batch=True sizes every part for the WHOLE batch (run_device_steps(...,
        alternate=True) deals complete requests to the parts); False for its rows only (the split schedule)."""
        bnd = self.bounds(batch)
        for i in range(len(self.parts) if whole_batch else len(bnd) - 1):
            self.parts[i].reserve(batch if whole_batch else bnd[i + 1] - bnd[i], tokens, frames)

    def set_tails(self, tails: str):
        """"zero" / "reference" on every handle (MiSession.set_tails)."""
        with self._mu:
            for s in self.parts:
                s.set_tails(tails)

    def hparam(self, key):
        return self.parts[0].hparam(key)

    def bounds(self, B):
        n = min(len(self.parts), B)
        return [B * i // n for i in range(n + 1)]

    def run_device(self, ids_ptr, lens_ptr, B, T, scales, sid_ptr=None, seeds=None):
        """Device pointers in (rows of one [B, T] int64 tensor / [B] tensors); enqueues every sub-batch on its own
        stream and returns [(first_row, rows, MiSession.run_device result)] - the waveform of a part stays in that
        part's workspace.  Call sync() before reading.  scales (host) [3] or [B, 3] and seeds as MiSession.run_device:
        each part gets its own rows."""
        rows = seeds is not None or np.ndim(scales) == 2   # (else: every part is called exactly as before)
        if rows:
            scales, seeds = _device_settings(scales, B, seeds)
        out = []
        bnd = self.bounds(B)
        for i in range(len(bnd) - 1):
            b0, nb = bnd[i], bnd[i + 1] - bnd[i]
            sc, sd = _part(scales, seeds, b0, b0 + nb)
            r = self.parts[i].run_device(ids_ptr + b0 * T * 8, lens_ptr + b0 * 8, nb, T, sc,
                                         sid_ptr + b0 * 8 if sid_ptr else None, **({"seeds": sd} if rows else {}))
            out.append((b0, nb, r))
        return out

    def run_device_steps(self, ids_ptr, lens_ptr, B, T, scales, steps, sid_ptr=None, alternate=False, seeds=None):
        """`steps` back-to-back passes over the same device-resident batch with one host thread per part, as two
        serving workers would run: a part goes on to its next pass without waiting for the other one, and part i
        starts once part i-1 has handed its first generator to the GPU, so that the small-grid stages of one part
        keep falling under the generator of the other.  Returns the frame count of every utterance of every pass,
        int64 [steps, B]; all work has completed on return.
        alternate=False: every pass is split over the parts (rows [b0, b1) each) - a pass's latency is that of a sub-batch.
        alternate=True: WHOLE passes are dealt to the parts in turn (pass k on part k mod n: request-level pipelining, each
        worker renders complete batches) - the generator keeps the full batch's grids (a sub-batch of 11 leaves the default
        voice's 128-channel stage at 283 workgroups on 512 slots), while pass k + 1's token and frame stages still fall
        under pass k's generator on the other handle.  scales [3] or [B, 3] and seeds as run_device."""
        import threading
        rows = seeds is not None or np.ndim(scales) == 2   # (else: every part is called exactly as before)
        if rows:
            scales, seeds = _device_settings(scales, B, seeds)
        bnd = self.bounds(B)
        n = len(bnd) - 1
        out = np.zeros((steps, B), np.int64)
        stamps = self.last_pass_stamps = [0.0] * steps  # (alternate: when pass k's call returned on its worker; diagnostics)
        started = [threading.Event() for _ in range(n)]
        errors = []

        def work(i):
            try:
                if i > 0:
                    started[i - 1].wait()
                if alternate:
                    for k in range(i, steps, n):
                        self.parts[i].run_device(ids_ptr, lens_ptr, B, T, scales, sid_ptr, **({"seeds": seeds} if rows else {}))
                        started[i].set()
                        out[k, :] = self.parts[i].last_y_lengths()
                        stamps[k] = time.perf_counter()
                    self.parts[i].sync()
                    return
                b0, nb = bnd[i], bnd[i + 1] - bnd[i]
                sc, sd = _part(scales, seeds, b0, b0 + nb)
                for k in range(steps):
                    self.parts[i].run_device(ids_ptr + b0 * T * 8, lens_ptr + b0 * 8, nb, T, sc,
                                             sid_ptr + b0 * 8 if sid_ptr else None, **({"seeds": sd} if rows else {}))
                    started[i].set()
                    out[k, b0:b0 + nb] = self.parts[i].last_y_lengths()
                self.parts[i].sync()
            except Exception as e:  # noqa: BLE001 - re-raised on the caller's thread
                errors.append(e)
            finally:
                started[i].set()

        if n == 1:
            work(0)
        else:
            th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        if errors:
            raise errors[0]
        return out

    def last_y_lengths(self, B) -> np.ndarray:
        n = len(self.bounds(B)) - 1
        return np.concatenate([self.parts[i].last_y_lengths() for i in range(n)])

    def last_durations(self, B) -> np.ndarray:
        """int64 [B, T] of the last B-utterance batch: the parts' MiSession.last_durations() in request order."""
        n = len(self.bounds(B)) - 1
        return np.concatenate([self.parts[i].last_durations() for i in range(n)])

    def synthesize_batch(self, ids, lens, scales, sid=None, seeds=None, durations=None, token_rate=None,
                         return_durations=False, noise_dp=None, noise_z=None, token_semitones=None, compensate=True,
                         token_semitones_end=None, fit=None):
        """Host arrays in, host arrays out, like MiSession.synthesize_batch (scales [3] or [B, 3], seeds, durations [B, T],
        token_rate [B, T], injected noise_dp [B, 2, T] / noise_z [B, inter, >= F]: each part gets its own rows of all of
        them; return_durations adds "durations" [B, T], the parts' rows in request order).  One worker thread per sub-batch (the C
        calls release the GIL): each enqueues its part (vits_run_async), learns its frame counts, meets the others at a
        barrier where the ONE [B,1,1,S_max] result array (pinned host memory) is sized, then waits for its own render
        and lets the DMA engine write its rows straight into that array (vits_fetch_output) - the copy-out of a part
        that finishes early runs under the render of the others, and no byte is copied twice on the host."""
        import threading
        if token_semitones is not None:
            # (the parts' warped rows have lengths of their own behind the barrier that sizes the one result: not a pass-through)
            raise SessionError("Unexpected input: 'token_semitones' / 'compensate' are not covered by PipelinedSession "
                               "(MiSession.synthesize_batch takes them)")
        if fit is not None:  # (a group may span the parts, and each part is a run of its own)
            raise SessionError("Unexpected input: 'fit' is not covered by PipelinedSession (MiSession.synthesize_batch takes it)")
        if token_semitones_end is not None:  # (for the same reason)
            raise SessionError("Unexpected input: 'token_semitones_end' is not covered by PipelinedSession "
                               "(MiSession.synthesize_batch takes it)")
        ids = np.ascontiguousarray(ids)
        lens = np.ascontiguousarray(lens)
        if ids.dtype != np.int64 or lens.dtype != np.int64 or ids.ndim != 2 or lens.shape != (ids.shape[0],):
            raise SessionError("Unexpected input: 'input' int64 [B,T], 'input_lengths' int64 [B]")
        B = ids.shape[0]
        scales, seeds = _settings(scales, B, seeds)
        durations, token_rate = _timing(durations, token_rate, lens, B, ids.shape[1])
        if sid is not None:
            sid = np.ascontiguousarray(sid)
            if sid.dtype != np.int64 or sid.shape != (B,):
                raise SessionError("Unexpected input: 'sid' must be int64 of shape [batch_size]")
        if noise_dp is not None:
            noise_dp = np.ascontiguousarray(noise_dp, np.float32)
            if noise_dp.shape != (B, 2, ids.shape[1]):
                raise SessionError(f"noise_dp must be [B,2,T], got {noise_dp.shape}")
        if noise_z is not None:
            noise_z = np.ascontiguousarray(noise_z, np.float32)
            if noise_z.ndim != 3 or noise_z.shape[0] != B or noise_z.shape[1] != self.hparam("inter"):
                raise SessionError(f"noise_z must be [B,inter,F], got {noise_z.shape}")
        with self._mu:
            return self._synthesize_batch_locked(ids, lens, scales, sid, B, seeds, durations, token_rate, return_durations,
                                                 noise_dp, noise_z)

    def _synthesize_batch_locked(self, ids, lens, scales, sid, B, seeds=None, durations=None, token_rate=None,
                                 return_durations=False, noise_dp=None, noise_z=None):
        import threading
        dur = np.zeros(ids.shape, np.int64) if return_durations else None
        bnd = self.bounds(B)
        n = len(bnd) - 1
        hop = self.hparam("hop")
        ylen = np.zeros(B, np.int64)
        box = {}
        pinned = self.parts[0].pinned_results

        def size_output():  # (barrier action: runs once, in one thread, when every part knows its frame counts)
            shape = (B, 1, 1, int(ylen.max()) * hop)
            box["out"] = _POOL.array(shape) if pinned else np.empty(shape, np.float32)

        bar = threading.Barrier(n, action=size_output)
        errors = []

        def work(i):
            b0, b1 = bnd[i], bnd[i + 1]
            p = self.parts[i]
            try:
                # (this part's rows of the injected noise: contiguous slices, alive until _begin has copied them)
                noise = _noise(p._seed, None if noise_dp is None else noise_dp[b0:b1], None if noise_z is None else noise_z[b0:b1])
                with p._mu:  # (a part may also be used on its own, e.g. bench.py's measure(): same per-session lock)
                    sc, sd = _part(scales, seeds, b0, b1)
                    p._begin(ids[b0:b1], lens[b0:b1], sc, None if sid is None else sid[b0:b1], noise, sd,
                             None if durations is None else durations[b0:b1],
                             None if token_rate is None else token_rate[b0:b1])
                    ylen[b0:b1] = p.last_y_lengths()
                    if dur is not None:
                        dur[b0:b1] = p.last_durations()
                    bar.wait()
                    p._fetch(box["out"], b0, b1 - b0)
            except threading.BrokenBarrierError:
                pass  # another part failed; its error is reported
            except Exception as e:  # noqa: BLE001 - re-raised on the caller's thread
                errors.append(e)
                bar.abort()

        if n == 1:
            work(0)
        else:
            th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        if errors:
            rng = [e for e in errors if isinstance(e, RangeError)]
            if rng:
                self._fall_back(rng[0])
                return self.synthesize_batch(ids, lens, scales, sid, seeds=seeds, durations=durations, token_rate=token_rate,
                                             return_durations=return_durations, noise_dp=noise_dp, noise_z=noise_z)
            raise errors[0]
        res = {"output": box["out"], "y_lengths": ylen}
        if dur is not None:
            res["durations"] = dur
        return res

    def sync(self):
        for s in self.parts:
            s.sync()

    def close(self, close_first: bool = True):
        """Closes the borrowed handles and (close_first) the arena owner.  close_first=False hands the first session back
        to its caller as it was given: open, with its own range fallback restored."""
        for s in reversed(self.parts[1:]):  # the first handle owns the arena the others borrow
            s.close()
        first = self.parts[0]
        del self.parts[1:]
        first.range_fallback = self._first_had_fallback
        if close_first:
            first.close()


# kernel-level hooks (tests)
def test_conv1d(x, w, bias=None, dil=1, pad_l=0, lrelu_slope=None, relu=False, device_id=0, hint=0):
    """hint: tile-size class as chosen at pack time (0 generator, 1 flow, 2 token domain)."""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    out = np.empty((B, Cout, T), np.float32)
    flags = (1 if lrelu_slope is not None else 0) | (2 if relu else 0) | ((hint & 3) << 8)
    rc = lib.vits_test_conv1d(device_id, _ffi.ptr(x), B, Cin, T, _ffi.ptr(w), _ffi.ptr(b), Cout, K, dil, pad_l, flags,
                              float(lrelu_slope or 0.0), _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_conv1d_sx(x, w, bias=None, dil=1, pad_l=0, planes_slope=None, residual=False, in_slope=None, device_id=0,
                   precision="f32", planes_only=False, small=False):
    """The split-operand engine (Cin % 16 == 0, Cout % 32 == 0).  planes_slope: read the result back from
    the 16-bit output planes, which carry leaky_relu(conv, planes_slope); residual: out = conv(x) + x;
    in_slope: out = conv(leaky_relu(x, in_slope)) [+ x] - Cin <= 64 (the raw-input kernels), or precision "f16", whose
    input plane then holds leaky_relu(x) and whose residual is recovered from that plane.
    precision: "f32" = six exact bf16 plane products; "f16x3" = two fp16 planes, three products (fp32-grade); "f16" = one
    fp16 plane, one product, fp16 storage (the reduced-precision vocoder of BASELINE config 4).
    planes_only: the planes are the launch's only output (the specialised plane epilogues); needs planes_slope.
    small: the short-launch kernel (conv_sx_small.hip.hpp, f16x3 on plane inputs, Cin % 32 == 0) with the same epilogue."""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    out = np.empty((B, Cout, T), np.float32)
    flags = (1 if planes_slope is not None else 0) | (4 if residual else 0) | (8 if in_slope is not None else 0)
    flags |= {"f32": 0, "f16": 2, "f16x3": 3}[precision] << 4
    flags |= 128 if planes_only else 0
    flags |= 256 if small else 0
    if in_slope is not None and planes_slope is not None and in_slope != planes_slope:
        raise ValueError("the hook takes one slope value")
    if in_slope is not None and Cin > 64 and precision != "f16":
        raise ValueError("in_slope needs a raw-input conv (Cin <= 64) or the single-plane arithmetic")
    slope = planes_slope if planes_slope is not None else in_slope
    rc = lib.vits_test_conv1d_sx(device_id, _ffi.ptr(x), B, Cin, T, _ffi.ptr(w), _ffi.ptr(b), Cout, K, dil, pad_l,
                                 flags, float(slope or 0.0), _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_conv1d_sx_planar(x, w, bias=None, dil=1, lens=None, old=None, row_split=None, pl_rows=0, relu=False, mask=False,
                          residual=False, accumulate=False, coupling=False, store2=False, planes_of2=False, device_id=0,
                          small=False):
    """The split-operand engine's planar epilogue (f16x3, "same" padding): o = old + act(conv(x) + bias) * mask, rows
    [0, row_split) in a first tensor, the rest in a second (see include/vitsmi.h).  small=True: through the short-launch
    kernel (conv_sx_small.hip.hpp) instead of the engine's.  Returns (out [B, Cout, T], planes [B, pl_rows, T] or None)."""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    B, Cin, T = x.shape
    Cout, _, K = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
    od = None if old is None else np.ascontiguousarray(old, np.float32)
    out = np.empty((B, Cout, T), np.float32)
    pl = np.empty((B, pl_rows, T), np.float32) if pl_rows else None
    flags = (1 if relu else 0) | (2 if mask else 0) | (4 if residual else 0) | (8 if accumulate else 0) | \
            (16 if coupling else 0) | (32 if store2 else 0) | (64 if planes_of2 else 0) | (128 if small else 0)
    rc = lib.vits_test_conv1d_sx_planar(device_id, _ffi.ptr(x), B, Cin, T, _ffi.ptr(w), _ffi.ptr(b), Cout, K, dil, flags,
                                        _ffi.ptr(ln), _ffi.ptr(od), Cout if row_split is None else row_split, pl_rows,
                                        _ffi.ptr(out), _ffi.ptr(pl))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out, pl


# the f32 engine's flags by name (conv_engine.hip.hpp; include/vitsmi.h VITS_CONV_*)
CONV_FLAGS = {"pro_lrelu": 1, "pro_mask": 2, "relu": 4, "mask": 8, "res": 16, "acc": 32, "div": 64, "coupling": 128, "wn": 256,
              "wn_first": 512}
CONV_EPI_SENTINEL = -1234.5678  # what the hook puts where it was given no old contents, and into every pitch column


def test_conv1d_epi(x, w, bias=None, flags=(), dil=1, pad_l=None, stride=1, hint=0, cfg=None, ck=None, lens=None, bias_b=None,
                    res=None, old_out=None, old_out2=None, out2=False, slope=0.1, div=1.0, oslope=1.0, oslope2=1.0, wn_split=0,
                    x_cstride=0, out_cstride=0, out_rows=0, out_row0=0, pl_rows=0, device_id=0):
    """The f32 conv engine with the argument set the pipeline's conv() gives it (include/vitsmi.h vits_test_conv1d_epi).
    flags: names of CONV_FLAGS.  stride > 1: ConvTranspose1d, w [Cin, Cout, K].  cfg / ck: an explicit tile and chunk,
    else the choice by `hint`.  old_out / old_out2 [B, out_rows, T * stride]: previous contents of the outputs; without
    them, and in every pitch column, the outputs start as CONV_EPI_SENTINEL.  out2: second output wanted (implied by
    old_out2).  Returns a dict: out / out2 [B, out_rows, out pitch] whole, planes [B, pl_rows, T] or None, kernel (the
    instantiation launched), cfg, ck."""
    lib = _ffi.load()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, w, bias, bias_b, res, old_out, old_out2 = (f32(a) for a in (x, w, bias, bias_b, res, old_out, old_out2))
    B, Cin, T = x.shape
    Cout, K = (w.shape[1] if stride > 1 else w.shape[0]), w.shape[2]
    ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
    rows, pitch = out_rows or Cout, out_cstride or T * stride
    # (the hook reads these by the shapes it derives: whatever disagrees is refused here)
    for name, arr, shape in (("w", w, (Cin, Cout, K) if stride > 1 else (Cout, Cin, K)), ("bias", bias, (Cout,)),
                             ("res", res, (B, Cout, pitch)), ("old_out", old_out, (B, rows, T * stride)),
                             ("old_out2", old_out2, (B, rows, T * stride)), ("lens", ln, (B,))):
        if arr is not None and arr.shape != shape:
            raise ValueError(f"{name} has shape {arr.shape}, the launch needs {shape}")
    if bias_b is not None and (bias_b.ndim != 2 or bias_b.shape[0] != B):
        raise ValueError(f"bias_b has shape {bias_b.shape}, the launch needs ({B}, stride)")
    out = np.empty((B, rows, pitch), np.float32)
    o2 = np.empty((B, rows, pitch), np.float32) if (out2 or old_out2 is not None) else None
    pl = np.empty((B, pl_rows, T), np.float32) if pl_rows > 0 else None
    a = _ffi.VitsTestConvEpiArgs()
    a.B, a.Cin, a.T, a.Cout, a.K, a.dil, a.stride, a.hint = B, Cin, T, Cout, K, dil, stride, hint
    a.pad_l = dil * (K - 1) // 2 if pad_l is None else pad_l
    a.cfg, a.ck = (-1 if cfg is None else cfg), (-1 if ck is None else ck)
    a.flags = sum(CONV_FLAGS[f] for f in flags)
    a.slope, a.div, a.oslope, a.oslope2, a.wn_split = slope, div, oslope, oslope2, wn_split
    a.x, a.w, a.bias, a.lens, a.bias_b, a.res = (_ffi.ptr(v) for v in (x, w, bias, ln, bias_b, res))
    a.bias_b_stride = 0 if bias_b is None else bias_b.shape[1]
    a.x_cstride, a.out_cstride, a.out_rows, a.out_row0 = x_cstride, out_cstride, out_rows, out_row0
    a.old_out, a.old_out2, a.sentinel = _ffi.ptr(old_out), _ffi.ptr(old_out2), CONV_EPI_SENTINEL
    a.out, a.out2, a.pl_rows, a.planes_out = _ffi.ptr(out), _ffi.ptr(o2), pl_rows, _ffi.ptr(pl)
    rc = lib.vits_test_conv1d_epi(device_id, C.byref(a))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"out": out, "out2": o2, "planes": pl, "kernel": a.kernel.decode(), "cfg": a.cfg_used, "ck": a.ck_used}


# the split-operand engine's epilogue flags and arithmetics by name (include/vitsmi.h VITS_SX_*)
SX_EPI_FLAGS = {"res": 1, "acc": 2, "div": 4, "no_raw_store": 8}
SX_PRECISIONS = {"bf16x6": 0, "f16x3": 1, "f16": 2}


def test_conv1d_sx_epi(x, w, bias=None, flags=(), precision="f16x3", dil=1, pad_l=None, stride=1, force16=False, no_s16=False,
                       min_cfg=0, run_cfg=-1, res=None, res_is_x=False, res_planes=False, res_slope=1.0, old_out=None,
                       bias_b=None, div=1.0, oslope=1.0, oslope2=1.0, islope=1.0, raw=True, planes=False, lens=None,
                       rag_add=0, rag_mul=1, sentinel=CONV_EPI_SENTINEL, device_id=0):
    """The split-operand conv engine with the argument set the pipeline's conv_sx() gives a generator-form launch
    (include/vitsmi.h vits_test_conv1d_sx_epi).  flags: names of SX_EPI_FLAGS.  stride > 1: ConvTranspose1d, w [Cin, Cout, K].
    res: fp32 [B, Cout, T * stride], or with res_planes the same tensor uploaded as operand planes of leaky_relu(res,
    res_slope); res_is_x: the raw input's own device tensor.  raw / planes: which outputs exist; both start as `sentinel`
    (raw: as old_out where given).  Returns a dict: out, planes [B, Cout, T * stride] or None, res_seen (what the residual
    planes hold, or None), kernel (the instantiation launched), pack_cfg, run_cfg, rawin, s16, ck, peak."""
    lib = _ffi.load()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, w, bias, bias_b, res, old_out = (f32(a) for a in (x, w, bias, bias_b, res, old_out))
    B, Cin, T = x.shape
    Cout, K = (w.shape[1] if stride > 1 else w.shape[0]), w.shape[2]
    To = T * stride
    ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
    # (the hook reads these by the shapes it derives: whatever disagrees is refused here)
    for name, arr, shape in (("w", w, (Cin, Cout, K) if stride > 1 else (Cout, Cin, K)), ("bias", bias, (Cout,)),
                             ("res", res, (B, Cout, To)), ("old_out", old_out, (B, Cout, To)), ("lens", ln, (B,))):
        if arr is not None and arr.shape != shape:
            raise ValueError(f"{name} has shape {arr.shape}, the launch needs {shape}")
    if bias_b is not None and (bias_b.ndim != 2 or bias_b.shape[0] != B):
        raise ValueError(f"bias_b has shape {bias_b.shape}, the launch needs ({B}, stride)")
    out = np.empty((B, Cout, To), np.float32) if raw else None
    pl = np.empty((B, Cout, To), np.float32) if planes else None
    seen = np.empty((B, Cout, To), np.float32) if (res_planes and res is not None) else None
    a = _ffi.VitsTestConvSxEpiArgs()
    a.B, a.Cin, a.T, a.Cout, a.K, a.dil, a.stride = B, Cin, T, Cout, K, dil, stride
    a.pad_l = dil * (K - 1) // 2 if pad_l is None else pad_l
    a.precision, a.force16, a.no_s16, a.min_cfg, a.run_cfg = SX_PRECISIONS[precision], int(force16), int(no_s16), min_cfg, run_cfg
    a.flags = sum(SX_EPI_FLAGS[f] for f in flags)
    a.x, a.w, a.bias, a.res, a.old_out, a.bias_b, a.lens = (_ffi.ptr(v) for v in (x, w, bias, res, old_out, bias_b, ln))
    a.res_is_x, a.res_planes, a.res_slope = int(res_is_x), int(res_planes), res_slope
    a.bias_b_stride = 0 if bias_b is None else bias_b.shape[1]
    a.div, a.oslope, a.oslope2, a.islope = div, oslope, oslope2, islope
    a.rag_add, a.rag_mul, a.sentinel = rag_add, rag_mul, sentinel
    a.out, a.planes_out, a.res_seen = _ffi.ptr(out), _ffi.ptr(pl), _ffi.ptr(seen)
    rc = lib.vits_test_conv1d_sx_epi(device_id, C.byref(a))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"out": out, "planes": pl, "res_seen": seen, "kernel": a.kernel.decode(), "pack_cfg": a.pack_cfg, "run_cfg": a.run_cfg_used,
            "rawin": bool(a.rawin), "s16": bool(a.s16), "ck": a.ck, "peak": float(a.peak)}


def test_wn_gate(a, blocked=False, device_id=0):
    """tanh(a[:, :H]) * sigmoid(a[:, H:]) of a [B, 2H, T]: wn_gate_kernel, or (blocked) wn_gate_blocked_kernel on the same
    values in the raw cell layout.  -> [B, H, T]"""
    lib = _ffi.load()
    a = np.ascontiguousarray(a, np.float32)
    B, C2, T = a.shape
    if C2 % 2:
        raise ValueError("a holds the tanh rows and as many sigmoid rows")
    out = np.empty((B, C2 // 2, T), np.float32)
    rc = lib.vits_test_wn_gate(device_id, _ffi.ptr(a), B, C2 // 2, T, 1 if blocked else 0, _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_cond_matvec(emb_g, sid, W, bias=None, device_id=0):
    """out[b] = bias + W @ emb_g[clamp(sid[b])] (cond_matvec_kernel); emb_g [n_speakers, gin], W [rows, gin] -> [B, rows]"""
    lib = _ffi.load()
    emb_g = np.ascontiguousarray(emb_g, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    sid = np.ascontiguousarray(sid, np.int64)
    if emb_g.ndim != 2 or W.ndim != 2 or W.shape[1] != emb_g.shape[1] or sid.ndim != 1 or (b is not None and b.shape != W.shape[:1]):
        raise ValueError("emb_g [n_speakers, gin], W [rows, gin], bias [rows], sid [B]")
    out = np.empty((len(sid), W.shape[0]), np.float32)
    rc = lib.vits_test_cond_matvec(device_id, _ffi.ptr(emb_g), emb_g.shape[0], emb_g.shape[1], _ffi.ptr(sid), len(sid),
                                   _ffi.ptr(W), _ffi.ptr(b), W.shape[0], _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_conv1d_sx_gate(x, w, bias, g, dil=1, small=False, planes=False, device_id=0):
    """The flow's WN in-layer with its gate epilogue: acts = tanh(a + g_a) * sigmoid(b + g_b) where (a | b) = conv(x) + bias
    ("same" padding), w [2H, Cin, K], bias [2H], g [B, 2H] in the module's channel order (modules.py:195-203,
    commons.py:99-106).  The hook wants the rows pair-interleaved the way the packer lays them out; that permutation is
    applied here.  small: the short-launch kernel; planes: the result through the fp16 operand planes.  -> [B, H, T]"""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    B, Cin, T = x.shape
    C2, _, K = w.shape
    H = C2 // 2
    perm = np.concatenate([np.concatenate([np.arange(p, p + 32), H + np.arange(p, p + 32)]) for p in range(0, H, 32)])
    wp = np.ascontiguousarray(np.asarray(w, np.float32)[perm])
    bp = np.ascontiguousarray(np.asarray(bias, np.float32)[perm])
    gg = np.ascontiguousarray(g, np.float32)
    out = np.empty((B, H, T), np.float32)
    rc = lib.vits_test_conv1d_sx_gate(device_id, _ffi.ptr(x), B, Cin, T, _ffi.ptr(wp), _ffi.ptr(bp), _ffi.ptr(gg), C2, K, dil,
                                      (1 if small else 0) | (2 if planes else 0), _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_conv_pair_sx(x, w1, b1, w2, b2, dil1=1, dil2=1, chain=False, slope=0.1, device_id=0, timed=False, kernel="pair",
                      from_plane=False):
    """Two dependent convs in ONE fused launch (32- / 64-channel stage of the generator):
    chain=False (ResBlock1 step): out = c2(lrelu(c1(lrelu(x)))) + x
    chain=True (two ResBlock2 steps): x1 = c1(lrelu(x)) + x; out = c2(lrelu(x1)) + x1.    timed=True -> (out, ms).
    kernel: "pair" = conv_sx_pair_kernel (32x32x16 loop, f16x3), "pair16" = conv_sx_pair16_kernel (16x16x32 loop) in f16x3,
    "pair16_f16" = the same in the single-plane arithmetic (fp16 plane in; from_plane: the result read back from the output
    plane, leaky_relu(out, slope) as fp16)."""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    w1 = np.ascontiguousarray(w1, np.float32)
    w2 = np.ascontiguousarray(w2, np.float32)
    B, Cc, T = x.shape
    K = w1.shape[2]
    if w1.shape != (Cc, Cc, K) or w2.shape != (Cc, Cc, K):
        raise ValueError("both convs are C -> C with the same kernel size")
    b1 = None if b1 is None else np.ascontiguousarray(b1, np.float32)
    b2 = None if b2 is None else np.ascontiguousarray(b2, np.float32)
    out = np.empty_like(x)
    ms = C.c_float(0.0)
    rc = lib.vits_test_conv_pair_sx(device_id, _ffi.ptr(x), B, Cc, T, _ffi.ptr(w1), _ffi.ptr(b1), _ffi.ptr(w2),
                                    _ffi.ptr(b2), K, dil1, dil2,
                                    (1 if chain else 0) | ({"pair": 0, "pair16": 1, "pair16_f16": 2}[kernel] << 1) | (8 if from_plane else 0),
                                    float(slope), _ffi.ptr(out),
                                    C.byref(ms) if timed else None)
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return (out, float(ms.value)) if timed else out


# the fused ResBlock step's launch flags by name (include/vitsmi.h VITS_P16_EPI_*)
P16_EPI_FLAGS = {"acc": 1, "div": 2, "raw": 4, "planes": 8}


def test_conv_pair16_epi(x, w1, b1, w2, b2, flags=("raw",), dil1=1, dil2=1, chain=False, slope=0.1, precision="f16x3", div=1.0,
                         old_out=None, lens=None, rag_add=0, rag_mul=1, x_tail=None, sentinel=CONV_EPI_SENTINEL, device_id=0):
    """conv_sx_pair16_kernel with the argument set the generator's conv_sx_pair16() gives it (include/vitsmi.h
    vits_test_conv_pair16_epi): one launch.  flags: names of P16_EPI_FLAGS.  The raw tensor starts as old_out, else as
    `sentinel`; the planes start as the sentinel's split.  x_tail [B, C, T]: what the input planes hold behind each utterance's
    end instead of x.  Returns a dict: out (the raw tensor after the launch), planes (read back from the output planes; None
    without the planes flag), x_seen (x as the kernel recovers it from its input planes), kernel, BN, BNo, ovl, peak, guard_ok."""
    lib = _ffi.load()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, w1, b1, w2, b2, old_out, x_tail = (f32(a) for a in (x, w1, b1, w2, b2, old_out, x_tail))
    B, Cc, T = x.shape
    K = w1.shape[2]
    ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
    # (the hook reads these by the shapes it derives: whatever disagrees is refused here)
    for name, arr, shape in (("w1", w1, (Cc, Cc, K)), ("w2", w2, (Cc, Cc, K)), ("b1", b1, (Cc,)), ("b2", b2, (Cc,)),
                             ("old_out", old_out, (B, Cc, T)), ("x_tail", x_tail, (B, Cc, T)), ("lens", ln, (B,))):
        if arr is not None and arr.shape != shape:
            raise ValueError(f"{name} has shape {arr.shape}, the launch needs {shape}")
    out = np.empty((B, Cc, T), np.float32)
    pl = np.empty((B, Cc, T), np.float32) if "planes" in flags else None
    seen = np.empty((B, Cc, T), np.float32)
    a = _ffi.VitsTestConvPair16EpiArgs()
    a.B, a.C, a.T, a.K, a.dil1, a.dil2, a.chain = B, Cc, T, K, dil1, dil2, int(bool(chain))
    a.precision, a.flags = SX_PRECISIONS[precision], sum(P16_EPI_FLAGS[f] for f in flags)
    a.slope, a.div, a.sentinel = slope, div, sentinel
    a.x, a.w1, a.b1, a.w2, a.b2, a.old_out, a.x_tail, a.lens = (_ffi.ptr(v) for v in (x, w1, b1, w2, b2, old_out, x_tail, ln))
    a.rag_add, a.rag_mul = rag_add, rag_mul
    a.out, a.planes_out, a.x_seen = _ffi.ptr(out), _ffi.ptr(pl), _ffi.ptr(seen)
    rc = lib.vits_test_conv_pair16_epi(device_id, C.byref(a))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"out": out, "planes": pl, "x_seen": seen, "kernel": a.kernel.decode(), "BN": a.BN, "BNo": a.BNo, "ovl": bool(a.ovl),
            "peak": float(a.peak), "guard_ok": bool(a.guard_ok)}


def test_split_forms(x, slope=0.1, form="pair", device_id=0):
    """The activation -> operand-plane helpers on an array (include/vitsmi.h vits_test_split_forms): x [n], n even.
    form: "engine" = split2h_pair_pk, "pair" = what conv_sx_pair_kernel uses.  Returns a dict: h0, h1 (float16 views of the
    planes' bits), pk [n / 2], rec [n]."""
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 1 or x.size < 2 or x.size % 2:
        raise ValueError("x: one dimension, an even number of values")
    n = x.size
    h0, h1 = np.empty(n, np.uint16), np.empty(n, np.uint16)
    pk, rec = np.empty(n // 2, np.float32), np.empty(n, np.float32)
    rc = lib.vits_test_split_forms(device_id, _ffi.ptr(x), n, float(slope), {"engine": 0, "pair": 1}[form], _ffi.ptr(h0), _ffi.ptr(h1),
                                   _ffi.ptr(pk), _ffi.ptr(rec))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"h0": h0.view(np.float16), "h1": h1.view(np.float16), "pk": pk, "rec": rec}


# conv_sx_pair_kernel's launch flags by name (include/vitsmi.h VITS_PAIR_EPI_*)
PAIR_EPI_FLAGS = {"acc": 1, "div": 2}


def test_conv_pair_sx_epi(x, w1, b1, w2, b2, flags=(), dil1=1, dil2=1, chain=False, slope=0.1, div=1.0, out_init=None, lens=None,
                          device_id=0):
    """conv_sx_pair_kernel with the argument set the generator's conv_sx_pair() gives it (include/vitsmi.h
    vits_test_conv_pair_sx_epi): one launch.  flags: names of PAIR_EPI_FLAGS.  lens [B]: utterance b's tensors end at lens[b]
    columns.  The raw tensor starts as out_init, else as zeros.  Returns a dict: out (the raw tensor after the launch), kernel,
    BNo."""
    lib = _ffi.load()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, w1, b1, w2, b2, out_init = (f32(a) for a in (x, w1, b1, w2, b2, out_init))
    B, Cc, T = x.shape
    K = w1.shape[2]
    ln = None if lens is None else np.ascontiguousarray(lens, np.int64)
    for name, arr, shape in (("w1", w1, (Cc, Cc, K)), ("w2", w2, (Cc, Cc, K)), ("b1", b1, (Cc,)), ("b2", b2, (Cc,)),
                             ("out_init", out_init, (B, Cc, T)), ("lens", ln, (B,))):
        if arr is not None and arr.shape != shape:
            raise ValueError(f"{name} has shape {arr.shape}, the launch needs {shape}")
    out = np.empty((B, Cc, T), np.float32)
    a = _ffi.VitsTestConvPairSxEpiArgs()
    a.B, a.C, a.T, a.K, a.dil1, a.dil2, a.chain = B, Cc, T, K, dil1, dil2, int(bool(chain))
    a.flags = sum(PAIR_EPI_FLAGS[f] for f in flags)
    a.slope, a.div = slope, div
    a.x, a.w1, a.b1, a.w2, a.b2, a.lens, a.out_init, a.out = (_ffi.ptr(v) for v in (x, w1, b1, w2, b2, ln, out_init, out))
    rc = lib.vits_test_conv_pair_sx_epi(device_id, C.byref(a))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"out": out, "kernel": a.kernel.decode(), "BNo": a.BNo}


def bench_conv1d_sx(B, Cin, Cout, T, K, dil=1, dbg=0, iters=20, device_id=0):
    """Average launch time (ms) of one conv shape on the split-exact engine -> (ms, tile config)."""
    lib = _ffi.load()
    res = np.zeros(8, np.float32)
    rc = lib.vits_bench_conv1d_sx(device_id, B, Cin, Cout, T, K, dil, dbg, iters,
                                  res.ctypes.data_as(_ffi.C.POINTER(_ffi.C.c_float)))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    if dbg & 16:
        return float(res[0]), int(res[1]), [float(v) for v in res[3:8]] + [float(res[2])]
    return float(res[0]), int(res[1])


def test_conv_transpose1d(x, w, bias, stride, device_id=0, sx=False):
    lib = _ffi.load()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    B, Cin, T = x.shape
    _, Cout, K = w.shape
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    out = np.empty((B, Cout, T * stride), np.float32)
    fn = lib.vits_test_conv_transpose1d_sx if sx else lib.vits_test_conv_transpose1d
    # sx="f16": the split-exact engine in its fp16 two-plane mode (the hook takes it as a negative stride)
    rc = fn(device_id, _ffi.ptr(x), B, Cin, T, _ffi.ptr(w), _ffi.ptr(b), Cout, K, -stride if sx == "f16" else stride,
            _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def test_attention16(qkv, n_heads, rel_k, rel_v, lens, device_id=0, kernel=1, planes=False, reps=0):
    """attention16.hip.hpp (kernel=1) or the fp32-MFMA kernel (0) on q|k|v planar fp32 [B, 3C, T]; returns out [B, C, T],
    plus the output's operand planes (uint16 [B, 3, C/8, T, 8]) when planes=True, plus ms per launch when reps > 0."""
    lib = _ffi.load()
    qkv = np.ascontiguousarray(qkv, np.float32)
    B, C3, T = qkv.shape
    Cc = C3 // 3
    rel_k = np.ascontiguousarray(rel_k, np.float32)
    rel_v = np.ascontiguousarray(rel_v, np.float32)
    window = (rel_k.shape[0] - 1) // 2
    lens = np.ascontiguousarray(lens, np.int64)
    out = np.empty((B, Cc, T), np.float32)
    opl = np.empty((B, 3, Cc // 8, T, 8), np.uint16) if planes else None
    ms = (C.c_float * 1)()
    rc = lib.vits_test_attention16(device_id, _ffi.ptr(qkv), B, Cc, T, n_heads, _ffi.ptr(rel_k), _ffi.ptr(rel_v), window,
                                   _ffi.ptr(lens), _ffi.ptr(out), _ffi.ptr(opl) if planes else None, int(kernel), int(reps), ms)
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    res = (out,)
    if planes:
        res += (opl,)
    if reps > 0:
        res += (float(ms[0]),)
    return res[0] if len(res) == 1 else res


def test_attention_form(qkv, n_heads, rel_k, rel_v, lens, kernel=16, want_out=True, want_planes=True, ns=0, qt=0, kh=0,
                        qkv_planes=None, device_id=0):
    """One attention launch in the form and instantiation named (include/vitsmi.h vits_test_attention_form): kernel 16
    (attention16.hip.hpp) or 32 (the fp32-MFMA kernel); want_out / want_planes: which outputs the launch writes; ns, qt
    (kernel 16) and kh (kernel 32): the instantiation, 0 = the launcher's choice; qkv_planes (kernel 16): the q|k|v operand
    planes uint16 [B, 3, 3C/8, T, 8] used as they are instead of the split of qkv.  qkv is fp32 [B, 3C, T].  Returns a dict: out
    [B, C, T] and planes uint16 [B, 3, C/8, T, 8] - the device buffers as the launch left them, 0xff bytes where it wrote nothing
    (planes is None when C % 8) -, peak (the range guard's), kernel (the instantiation started)."""
    lib = _ffi.load()
    qkv = np.ascontiguousarray(qkv, np.float32)
    B, C3, T = qkv.shape
    Cc = C3 // 3
    rel_k = np.ascontiguousarray(rel_k, np.float32)
    rel_v = np.ascontiguousarray(rel_v, np.float32)
    window = (rel_k.shape[0] - 1) // 2
    lens = np.ascontiguousarray(lens, np.int64)
    if C3 != 3 * Cc or n_heads <= 0 or Cc % n_heads or lens.shape != (B,):
        raise ValueError(f"q|k|v {qkv.shape} with {n_heads} heads and lens {lens.shape}")
    dk = Cc // n_heads
    if rel_k.shape != (2 * window + 1, dk) or rel_v.shape != rel_k.shape:
        raise ValueError(f"relative embeddings {rel_k.shape} / {rel_v.shape}, head width {dk}")
    qp = None
    if qkv_planes is not None:
        qp = np.ascontiguousarray(qkv_planes, np.uint16)
        if C3 % 8 or qp.shape != (B, 3, C3 // 8, T, 8):
            raise ValueError(f"q|k|v planes {qp.shape}, the launch needs {(B, 3, C3 // 8, T, 8)}")
    out = np.empty((B, Cc, T), np.float32)
    opl = np.empty((B, 3, Cc // 8, T, 8), np.uint16) if Cc % 8 == 0 else None
    a = _ffi.VitsTestAttentionFormArgs()
    a.kernel, a.qkv, a.qkv_planes = int(kernel), _ffi.ptr(qkv), _ffi.ptr(qp)
    a.B, a.C, a.T, a.n_heads, a.window = B, Cc, T, n_heads, window
    a.rel_k, a.rel_v, a.lens = _ffi.ptr(rel_k), _ffi.ptr(rel_v), _ffi.ptr(lens)
    a.want_out, a.want_planes, a.ns, a.qt, a.kh = int(bool(want_out)), int(bool(want_planes)), int(ns), int(qt), int(kh)
    a.out, a.out_planes = _ffi.ptr(out), _ffi.ptr(opl)
    rc = lib.vits_test_attention_form(device_id, C.byref(a))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return {"out": out, "planes": opl, "peak": float(a.peak), "kernel": a.kernel_name.decode()}


def test_attention(qkv, n_heads, rel_k, rel_v, lens, device_id=0):
    lib = _ffi.load()
    qkv = np.ascontiguousarray(qkv, np.float32)
    B, C3, T = qkv.shape
    Cc = C3 // 3
    rel_k = np.ascontiguousarray(rel_k, np.float32)
    rel_v = np.ascontiguousarray(rel_v, np.float32)
    window = (rel_k.shape[0] - 1) // 2
    lens = np.ascontiguousarray(lens, np.int64)
    out = np.empty((B, Cc, T), np.float32)
    rc = lib.vits_test_attention(device_id, _ffi.ptr(qkv), B, Cc, T, n_heads, _ffi.ptr(rel_k), _ffi.ptr(rel_v), window,
                                 _ffi.ptr(lens), _ffi.ptr(out))
    if rc != 0:
        raise SessionError(_ffi.last_error(None))
    return out


def _resample_test_args(x, lens, in_rate, out_rate):
    x = np.ascontiguousarray(x, np.float32)
    lens = np.ascontiguousarray(lens, np.int64)
    if x.ndim != 2 or lens.shape != (x.shape[0],):
        raise SessionError(f"x must be [B, S] and lens [B], got {x.shape} / {lens.shape}")
    L, M, _ = resample_plan(in_rate, out_rate)
    return x, lens, L, M


def test_resample(x, lens, in_rate, out_rate, device_id=0):
    """The output-rate resampler by value (vits_test_resample): x float32 [B, S], lens [B] valid samples per row ->
    (y float32 [B, S_out], counts int64 [B]) with counts = ceil(lens * L / M) and S_out = max(1, counts.max())."""
    x, lens, L, M = _resample_test_args(x, lens, in_rate, out_rate)
    B, S = x.shape
    counts = -(-np.clip(lens, 0, S) * L // M)
    y = np.full((B, max(1, int(counts.max()))), np.nan, np.float32)
    rc = _ffi.load().vits_test_resample(device_id, _ffi.ptr(x), _ffi.ptr(lens), B, S, int(in_rate), int(out_rate), _ffi.ptr(y),
                                        y.shape[1])
    if rc != 0:
        raise SessionError(f"vits_test_resample failed [{rc}]: {_ffi.last_error(None)}")
    return y, counts


def test_resample_rows(x, lens, in_rate, out_rates, device_id=0):
    """The rows entry of the resampler by value (vits_test_resample_rows): x float32 [B, S], lens [B], out_rates [B] (None, 0
    or in_rate: a native row) -> (y float32 [B, S_out], counts int64 [B]) with S_out = counts.max() (at least 1)."""
    x = np.ascontiguousarray(x, np.float32)
    lens = np.ascontiguousarray(lens, np.int64)
    rates = np.asarray([int(r or 0) for r in out_rates], np.int32)
    if x.ndim != 2 or lens.shape != (x.shape[0],) or rates.shape != lens.shape:
        raise SessionError(f"x must be [B, S], lens and out_rates [B], got {x.shape} / {lens.shape} / {rates.shape}")
    B, S = x.shape
    # (the engine validates the rates and reports the counts: the buffer is sized by a bound that needs no plan)
    cap = -(-S * max(int(rates.max()), int(in_rate)) // max(int(in_rate), 1)) + 1
    buf = np.full(B * cap, np.nan, np.float32)
    counts = np.zeros(B, np.int64)
    rc = _ffi.load().vits_test_resample_rows(device_id, _ffi.ptr(x), _ffi.ptr(lens), B, S, int(in_rate), _ffi.ptr(rates), _ffi.ptr(buf),
                                             buf.size, _ffi.ptr(counts))
    if rc != 0:
        raise SessionError(f"vits_test_resample_rows failed [{rc}]: {_ffi.last_error(None)}")
    S_out = int(counts.max())
    if S_out == 0:  # (nothing was written: one column of zeros, as the single-rate hook gives)
        return np.zeros((B, 1), np.float32), counts
    return buf[:B * S_out].reshape(B, S_out).copy(), counts


def warp_token(semitones):
    """(step, c, half_taps) of a token at `semitones` (vits_warp_token: pure host code)"""
    step, c, Kh = C.c_int64(), C.c_int64(), C.c_int32()
    rc = _ffi.load().vits_warp_token(float(semitones), C.byref(step), C.byref(c), C.byref(Kh))
    if rc != 0:
        raise SessionError(f"vits_warp_token failed [{rc}]: {_ffi.last_error(None)}")
    return step.value, c.value, Kh.value


def warp_plan(durations, semitones, hop):
    """One row's plan (vits_warp_plan: pure host code): durations [T] in frames, semitones [T] or None ->
    (segments: a ctypes array of _ffi.VitsWarpSeg, spans int64 [T], N)."""
    D = np.ascontiguousarray(durations, np.int64)
    st = None if semitones is None else np.ascontiguousarray(semitones, np.float32)
    if D.ndim != 1 or (st is not None and st.shape != D.shape):
        raise SessionError(f"durations must be [T] and semitones [T] or None, got {D.shape} / {None if st is None else st.shape}")
    segs = (_ffi.VitsWarpSeg * max(len(D), 1))()
    spans = np.zeros(len(D), np.int64)
    n = C.c_int64()
    count = _ffi.load().vits_warp_plan(_ffi.ptr(D), _ffi.ptr(st), len(D), int(hop), segs, _ffi.ptr(spans), C.byref(n))
    if count < 0:
        raise SessionError(f"vits_warp_plan failed [{count}]: {_ffi.last_error(None)}")
    return (_ffi.VitsWarpSeg * count)(*segs[:count]), spans, n.value


def test_warp(x, counts, row_segs, device_id=0):
    """The time warp by value (vits_test_warp): x float32 [B, S], counts [B] the rows' valid samples, row_segs - per row a
    sequence of _ffi.VitsWarpSeg (warp_plan's) -> y float32 [B, S_w], S_w = max(1, max_b N_b); every column is written."""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    if x.ndim != 2 or counts.shape != (x.shape[0],) or len(row_segs) != x.shape[0]:
        raise SessionError(f"x must be [B, S], counts [B] and row_segs B sequences, got {x.shape} / {counts.shape} / {len(row_segs)}")
    B, S = x.shape
    flat = [g for row in row_segs for g in row]
    first = np.cumsum([0] + [len(row) for row in row_segs]).astype(np.int32)
    segs = (_ffi.VitsWarpSeg * max(len(flat), 1))(*flat)
    n_out = [int(row[-1].n0 + row[-1].k) if len(row) else int(min(max(counts[b], 0), S)) for b, row in enumerate(row_segs)]
    S_w = max(1, max(n_out))
    y = np.full((B, S_w), np.nan, np.float32)
    rc = _ffi.load().vits_test_warp(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, segs, _ffi.ptr(first), _ffi.ptr(y), S_w)
    if rc != 0:
        raise SessionError(f"vits_test_warp failed [{rc}]: {_ffi.last_error(None)}")
    return y


def glide_token(st0, st1):
    """(step0, step1, rate) of a token gliding from st0 to st1 semitones (vits_glide_token: pure host code); rate is the
    float32 factor its duration takes under compensate"""
    a, b, r = C.c_int64(), C.c_int64(), C.c_float()
    rc = _ffi.load().vits_glide_token(float(st0), float(st1), C.byref(a), C.byref(b), C.byref(r))
    if rc != 0:
        raise SessionError(f"vits_glide_token failed [{rc}]: {_ffi.last_error(None)}")
    return a.value, b.value, np.float32(r.value)


def glide_cutoff(step):
    """(c, half_taps) of an output sample whose speed is `step` (vits_glide_cutoff: pure host code)"""
    c, Kh = C.c_int64(), C.c_int32()
    rc = _ffi.load().vits_glide_cutoff(int(step), C.byref(c), C.byref(Kh))
    if rc != 0:
        raise SessionError(f"vits_glide_cutoff failed [{rc}]: {_ffi.last_error(None)}")
    return c.value, Kh.value


def glide_plan(durations, st0, st1, hop):
    """One row's plan with glides (vits_glide_plan: pure host code): durations [T] in frames, st0 / st1 [T] or None ->
    (segments: a ctypes array of _ffi.VitsGlideSeg, spans int64 [T], N)."""
    D = np.ascontiguousarray(durations, np.int64)
    a = None if st0 is None else np.ascontiguousarray(st0, np.float32)
    b = None if st1 is None else np.ascontiguousarray(st1, np.float32)
    if D.ndim != 1 or any(v is not None and v.shape != D.shape for v in (a, b)):
        raise SessionError(f"durations must be [T] and st0 / st1 [T] or None, got {D.shape}")
    segs = (_ffi.VitsGlideSeg * max(len(D), 1))()
    spans = np.zeros(len(D), np.int64)
    n = C.c_int64()
    count = _ffi.load().vits_glide_plan(_ffi.ptr(D), _ffi.ptr(a), _ffi.ptr(b), len(D), int(hop), segs, _ffi.ptr(spans), C.byref(n))
    if count < 0:
        raise SessionError(f"vits_glide_plan failed [{count}]: {_ffi.last_error(None)}")
    return (_ffi.VitsGlideSeg * count)(*segs[:count]), spans, n.value


def test_glide(x, counts, row_segs, device_id=0):
    """The glide by value (vits_test_glide): test_warp over rows of _ffi.VitsGlideSeg (glide_plan's)."""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    if x.ndim != 2 or counts.shape != (x.shape[0],) or len(row_segs) != x.shape[0]:
        raise SessionError(f"x must be [B, S], counts [B] and row_segs B sequences, got {x.shape} / {counts.shape} / {len(row_segs)}")
    B, S = x.shape
    flat = [g for row in row_segs for g in row]
    first = np.cumsum([0] + [len(row) for row in row_segs]).astype(np.int32)
    segs = (_ffi.VitsGlideSeg * max(len(flat), 1))(*flat)
    n_out = [int(row[-1].n0 + row[-1].k) if len(row) else int(min(max(counts[b], 0), S)) for b, row in enumerate(row_segs)]
    S_w = max(1, max(n_out))
    y = np.full((B, S_w), np.nan, np.float32)
    rc = _ffi.load().vits_test_glide(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, segs, _ffi.ptr(first), _ffi.ptr(y), S_w)
    if rc != 0:
        raise SessionError(f"vits_test_glide failed [{rc}]: {_ffi.last_error(None)}")
    return y


def _pitched_spans(durations, st0, st1, hop, ratio):
    """the token spans of one row of a pitched run, in delivered samples: the plan without a rate, or - ratio (L, M) - the folded
    one, whose unpitched rows follow the resampler's rule over the row's n_b = y_len * hop valid samples, y_len = max(sum of the
    durations, 1) as the engine counts it"""
    if ratio is None:
        return warp_plan(durations, st0, hop)[1] if st1 is None else glide_plan(durations, st0, st1, hop)[1]
    L, M = ratio
    if not np.any(st0) and (st1 is None or not np.any(st1)):
        return rate_identity_spans(durations, hop, L, M, max(int(np.sum(durations)), 1) * hop)[0]
    return warp_plan_rate(durations, st0, hop, L, M)[1] if st1 is None else glide_plan_rate(durations, st0, st1, hop, L, M)[1]


def warp_token_rate(semitones, L, M):
    """(step, c, half_taps) of a token at `semitones` delivered at fi * L / M (vits_warp_token_rate: pure host code)"""
    step, c, Kh = C.c_int64(), C.c_int64(), C.c_int32()
    rc = _ffi.load().vits_warp_token_rate(float(semitones), int(L), int(M), C.byref(step), C.byref(c), C.byref(Kh))
    if rc != 0:
        raise SessionError(f"vits_warp_token_rate failed [{rc}]: {_ffi.last_error(None)}")
    return step.value, c.value, Kh.value


def warp_plan_rate(durations, semitones, hop, L, M):
    """warp_plan with the output rate fi * L / M folded into the steps (vits_warp_plan_rate: pure host code): n0, k and N are
    delivered samples."""
    D = np.ascontiguousarray(durations, np.int64)
    st = None if semitones is None else np.ascontiguousarray(semitones, np.float32)
    if D.ndim != 1 or (st is not None and st.shape != D.shape):
        raise SessionError(f"durations must be [T] and semitones [T] or None, got {D.shape} / {None if st is None else st.shape}")
    segs = (_ffi.VitsWarpSeg * max(len(D), 1))()
    spans = np.zeros(len(D), np.int64)
    n = C.c_int64()
    count = _ffi.load().vits_warp_plan_rate(_ffi.ptr(D), _ffi.ptr(st), len(D), int(hop), int(L), int(M), segs, _ffi.ptr(spans), C.byref(n))
    if count < 0:
        raise SessionError(f"vits_warp_plan_rate failed [{count}]: {_ffi.last_error(None)}")
    return (_ffi.VitsWarpSeg * count)(*segs[:count]), spans, n.value


def glide_plan_rate(durations, st0, st1, hop, L, M):
    """glide_plan with the output rate fi * L / M folded into the steps (vits_glide_plan_rate: pure host code)"""
    D = np.ascontiguousarray(durations, np.int64)
    a = None if st0 is None else np.ascontiguousarray(st0, np.float32)
    b = None if st1 is None else np.ascontiguousarray(st1, np.float32)
    if D.ndim != 1 or any(v is not None and v.shape != D.shape for v in (a, b)):
        raise SessionError(f"durations must be [T] and st0 / st1 [T] or None, got {D.shape}")
    segs = (_ffi.VitsGlideSeg * max(len(D), 1))()
    spans = np.zeros(len(D), np.int64)
    n = C.c_int64()
    count = _ffi.load().vits_glide_plan_rate(_ffi.ptr(D), _ffi.ptr(a), _ffi.ptr(b), len(D), int(hop), int(L), int(M), segs, _ffi.ptr(spans),
                                             C.byref(n))
    if count < 0:
        raise SessionError(f"vits_glide_plan_rate failed [{count}]: {_ffi.last_error(None)}")
    return (_ffi.VitsGlideSeg * count)(*segs[:count]), spans, n.value


def glide_cutoff_rate(step):
    """glide_cutoff over the steps a folded plan admits, [ONE / 8, 8 ONE] (vits_glide_cutoff_rate: pure host code)"""
    c, Kh = C.c_int64(), C.c_int32()
    rc = _ffi.load().vits_glide_cutoff_rate(int(step), C.byref(c), C.byref(Kh))
    if rc != 0:
        raise SessionError(f"vits_glide_cutoff_rate failed [{rc}]: {_ffi.last_error(None)}")
    return c.value, Kh.value


def rate_identity_spans(durations, hop, L, M, n_in):
    """(spans int64 [T], N) of an identity row - every token at 0 semitones - delivered at fi * L / M: the resampler's rule
    (vits_rate_identity_spans: pure host code)"""
    D = np.ascontiguousarray(durations, np.int64)
    spans = np.zeros(len(D), np.int64)
    n = C.c_int64()
    rc = _ffi.load().vits_rate_identity_spans(_ffi.ptr(D), len(D), int(hop), int(L), int(M), int(n_in), _ffi.ptr(spans), C.byref(n))
    if rc != 0:
        raise SessionError(f"vits_rate_identity_spans failed [{rc}]: {_ffi.last_error(None)}")
    return spans, n.value


def _test_rate(fn, seg_type, x, counts, row_segs, in_rates, out_rates, window, device_id):
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B = len(counts)
    fis = np.full(B, int(in_rates), np.int32) if np.ndim(in_rates) == 0 else np.ascontiguousarray(in_rates, np.int32)
    fos = np.asarray([int(r or 0) for r in out_rates], np.int32)
    if x.ndim != 2 or counts.shape != (x.shape[0],) or len(row_segs) != B or fis.shape != counts.shape or fos.shape != counts.shape:
        raise SessionError(f"x must be [B, S], counts, in_rates and out_rates [B] and row_segs B sequences, got {x.shape} / {counts.shape} / "
                           f"{fis.shape} / {fos.shape} / {len(row_segs)}")
    S = x.shape[1]
    flat = [g for row in row_segs for g in row]
    first = np.cumsum([0] + [len(row) for row in row_segs]).astype(np.int32)
    segs = (seg_type * max(len(flat), 1))(*flat)
    n_out = []
    for b, row in enumerate(row_segs):
        if len(row):
            n_out.append(int(row[-1].n0 + row[-1].k))
        else:  # an identity row: ceil(n_b * L / M)
            n = int(min(max(counts[b], 0), S))
            fi, fo = int(fis[b]), int(fos[b]) or int(fis[b])
            g = int(np.gcd(fi, fo))
            n_out.append(-(-n * (fo // g) // (fi // g)))
    n_lo, n_hi = window if window is not None else (0, max(1, max(n_out)))
    y = np.full((B, n_hi - n_lo), np.nan, np.float32)
    rc = getattr(_ffi.load(), fn)(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, segs, _ffi.ptr(first), _ffi.ptr(fis), _ffi.ptr(fos),
                                  int(n_lo), int(n_hi), _ffi.ptr(y))
    if rc != 0:
        raise SessionError(f"{fn} failed [{rc}]: {_ffi.last_error(None)}")
    return y, np.asarray(n_out, np.int64)


def test_warp_rate(x, counts, row_segs, in_rates, out_rates, window=None, device_id=0):
    """The wide warp by value (vits_test_warp_rate; vitsmi.h, "pitch at an output rate"): x float32 [B, S], counts [B], row_segs -
    per row the _ffi.VitsWarpSeg records of warp_plan_rate at the row's rates, none for an identity row -, in_rates one rate or
    [B], out_rates [B] (None, 0 or the row's in_rate: native).  window (n_lo, n_hi): the output samples rendered; None: [0, max(1, max_b N_b)).
    -> (y float32 [B, n_hi - n_lo], N int64 [B])."""
    return _test_rate("vits_test_warp_rate", _ffi.VitsWarpSeg, x, counts, row_segs, in_rates, out_rates, window, device_id)


def test_glide_rate(x, counts, row_segs, in_rates, out_rates, window=None, device_id=0):
    """test_warp_rate over rows of _ffi.VitsGlideSeg (glide_plan_rate's)"""
    return _test_rate("vits_test_glide_rate", _ffi.VitsGlideSeg, x, counts, row_segs, in_rates, out_rates, window, device_id)


def warp_emit_end_rate(segs, n_in, n_out, X, half):
    """warp_emit_end / glide_emit_end over the records of a folded plan whose largest Kh is `half` (vits_warp_emit_end_rate /
    vits_glide_emit_end_rate: pure host code)"""
    fn = "vits_glide_emit_end_rate" if isinstance(segs[0], _ffi.VitsGlideSeg) else "vits_warp_emit_end_rate"
    ready = C.c_int64()
    rc = getattr(_ffi.load(), fn)(segs, len(segs), int(n_in), int(n_out), int(X), int(half), C.byref(ready))
    if rc != 0:
        raise SessionError(f"{fn} failed [{rc}]: {_ffi.last_error(None)}")
    return ready.value


def identity_emit_end_rate(L, M, K, n_in, X):
    """the emit rule of an identity row of a folded plan: the resampler's (vits_identity_emit_end_rate: pure host code)"""
    ready = C.c_int64()
    rc = _ffi.load().vits_identity_emit_end_rate(int(L), int(M), int(K), int(n_in), int(X), C.byref(ready))
    if rc != 0:
        raise SessionError(f"vits_identity_emit_end_rate failed [{rc}]: {_ffi.last_error(None)}")
    return ready.value


def warp_stream_cap_rate(piece_samples, S_w, min_step, half):
    """n_cap of a streamed run with a folded plan: its least step and largest Kh (vits_warp_stream_cap_rate)"""
    cap = _ffi.load().vits_warp_stream_cap_rate(int(piece_samples), int(S_w), int(min_step), int(half))
    if cap < 0:
        raise SessionError(f"vits_warp_stream_cap_rate failed [{cap}]: {_ffi.last_error(None)}")
    return int(cap)


def _test_rate_pieces(fn, seg_type, x, counts, row_segs, in_rate, out_rate, piece_bounds, device_id):
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    bounds = np.ascontiguousarray(piece_bounds, np.int64)
    if x.ndim != 2 or counts.shape != (x.shape[0],) or len(row_segs) != x.shape[0] or bounds.ndim != 1 or not len(bounds):
        raise SessionError(f"x must be [B, S], counts [B], row_segs B sequences and piece_bounds [P], got {x.shape} / {counts.shape} / "
                           f"{len(row_segs)} / {bounds.shape}")
    B, S = x.shape
    flat = [g for row in row_segs for g in row]
    first = np.cumsum([0] + [len(row) for row in row_segs]).astype(np.int32)
    segs = (seg_type * max(len(flat), 1))(*flat)
    fo = int(out_rate or in_rate)
    g = int(np.gcd(int(in_rate), fo))
    L, M = fo // g, int(in_rate) // g
    n_out = [int(row[-1].n0 + row[-1].k) if len(row) else -(-int(min(max(counts[b], 0), S)) * L // M) for b, row in enumerate(row_segs)]
    S_w = max(1, max(n_out))
    y = np.full((B, S_w), np.nan, np.float32)
    cap = len(bounds) + S_w + 2  # (more windows than any schedule has)
    ranges = np.zeros((cap, 2), np.int64)
    rc = getattr(_ffi.load(), fn)(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, segs, _ffi.ptr(first), int(in_rate), fo, _ffi.ptr(bounds),
                                  len(bounds), _ffi.ptr(y), S_w, _ffi.ptr(ranges), cap)
    if rc < 0:
        raise SessionError(f"{fn} failed [{rc}]: {_ffi.last_error(None)}")
    return y, ranges[:rc]


def test_warp_rate_pieces(x, counts, row_segs, in_rate, out_rate, piece_bounds, device_id=0):
    """The wide streamed stage by value (vits_test_warp_rate_pieces): test_warp_pieces over a folded plan at one pair of rates"""
    return _test_rate_pieces("vits_test_warp_rate_pieces", _ffi.VitsWarpSeg, x, counts, row_segs, in_rate, out_rate, piece_bounds, device_id)


def test_glide_rate_pieces(x, counts, row_segs, in_rate, out_rate, piece_bounds, device_id=0):
    """test_warp_rate_pieces over rows of _ffi.VitsGlideSeg (glide_plan_rate's)"""
    return _test_rate_pieces("vits_test_glide_rate_pieces", _ffi.VitsGlideSeg, x, counts, row_segs, in_rate, out_rate, piece_bounds, device_id)


def _emit_end(fn, segs, n_in, n_out, X):
    ready = C.c_int64()
    rc = getattr(_ffi.load(), fn)(segs, len(segs), int(n_in), int(n_out), int(X), C.byref(ready))
    if rc != 0:
        raise SessionError(f"{fn} failed [{rc}]: {_ffi.last_error(None)}")
    return ready.value


def warp_emit_end(segs, n_in, n_out, X):
    """The emit rule of one row (vits_warp_emit_end: pure host code; vitsmi.h, "streamed pitch"): segs a ctypes array of
    _ffi.VitsWarpSeg (warp_plan's), n_in / n_out the row's valid input and output samples -> how many output samples exist
    once input samples [0, X) do (n_out where X >= n_in)."""
    return _emit_end("vits_warp_emit_end", segs, n_in, n_out, X)


def glide_emit_end(segs, n_in, n_out, X):
    """warp_emit_end over _ffi.VitsGlideSeg records (glide_plan's)"""
    return _emit_end("vits_glide_emit_end", segs, n_in, n_out, X)


def warp_stream_cap(piece_samples, S_w):
    """n_cap: the output samples one delivery of a streamed run with pitch holds at most (vits_warp_stream_cap)"""
    cap = _ffi.load().vits_warp_stream_cap(int(piece_samples), int(S_w))
    if cap < 0:
        raise SessionError(f"vits_warp_stream_cap failed [{cap}]: {_ffi.last_error(None)}")
    return int(cap)


def _test_pieces(fn, seg_type, x, counts, row_segs, piece_bounds, device_id):
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    bounds = np.ascontiguousarray(piece_bounds, np.int64)
    if x.ndim != 2 or counts.shape != (x.shape[0],) or len(row_segs) != x.shape[0] or bounds.ndim != 1 or not len(bounds):
        raise SessionError(f"x must be [B, S], counts [B], row_segs B sequences and piece_bounds [P], got {x.shape} / {counts.shape} / "
                           f"{len(row_segs)} / {bounds.shape}")
    B, S = x.shape
    flat = [g for row in row_segs for g in row]
    first = np.cumsum([0] + [len(row) for row in row_segs]).astype(np.int32)
    segs = (seg_type * max(len(flat), 1))(*flat)
    n_out = [int(row[-1].n0 + row[-1].k) if len(row) else int(min(max(counts[b], 0), S)) for b, row in enumerate(row_segs)]
    S_w = max(1, max(n_out))
    y = np.full((B, S_w), np.nan, np.float32)
    cap = len(bounds) + S_w + 2  # (more windows than any schedule has)
    ranges = np.zeros((cap, 2), np.int64)
    rc = getattr(_ffi.load(), fn)(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, segs, _ffi.ptr(first), _ffi.ptr(bounds), len(bounds),
                                  _ffi.ptr(y), S_w, _ffi.ptr(ranges), cap)
    if rc < 0:
        raise SessionError(f"{fn} failed [{rc}]: {_ffi.last_error(None)}")
    return y, ranges[:rc]


def test_warp_pieces(x, counts, row_segs, piece_bounds, device_id=0):
    """The streamed warp by value (vits_test_warp_pieces): test_warp's arguments with the input cut at piece_bounds (ascending
    piece ends, the last one S) and sent through the pipeline's stage -> (y float32 [B, S_w]: the windows joined, ranges
    int64 [calls, 2]: {first, n} of every window in order)."""
    return _test_pieces("vits_test_warp_pieces", _ffi.VitsWarpSeg, x, counts, row_segs, piece_bounds, device_id)


def test_glide_pieces(x, counts, row_segs, piece_bounds, device_id=0):
    """test_warp_pieces over rows of _ffi.VitsGlideSeg (glide_plan's)"""
    return _test_pieces("vits_test_glide_pieces", _ffi.VitsGlideSeg, x, counts, row_segs, piece_bounds, device_id)


def test_resample_pieces(x, lens, in_rate, out_rate, piece_samples, device_id=0):
    """The same input through the chunked entry, `piece_samples` input samples at a time (vits_test_resample_pieces):
    (y float32 [B, ceil(S * L / M)], [(first_sample, n_samples) of every delivery])."""
    x, lens, L, M = _resample_test_args(x, lens, in_rate, out_rate)
    B, S = x.shape
    y = np.full((B, -(-S * L // M)), np.nan, np.float32)
    max_ranges = -(-S // int(piece_samples)) + 1
    ranges = np.zeros((max_ranges, 2), np.int64)
    n = _ffi.load().vits_test_resample_pieces(device_id, _ffi.ptr(x), _ffi.ptr(lens), B, S, int(in_rate), int(out_rate),
                                              int(piece_samples), _ffi.ptr(y), y.shape[1], _ffi.ptr(ranges), max_ranges)
    if n < 0:
        raise SessionError(f"vits_test_resample_pieces failed [{n}]: {_ffi.last_error(None)}")
    return y, [(int(a), int(b)) for a, b in ranges[:n]]


def test_stream_pack(x, counts, piece_samples, encoding="pcm16", ref_peak=None, volume=None, device_id=0):
    """vits_test_stream_pack: x [B, S] float32 and the rows' valid samples through the encoded stream's kernel, `piece_samples`
    columns at a time -> one EncodedChunk per piece, with `data` the whole pitched block as uint8 [B, pitch] (pad bytes
    included: they are part of what the kernel writes)."""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B, S = x.shape
    fmt, dtype = _stream_format(encoding, ref_peak, volume, B)
    w, piece = np.dtype(dtype).itemsize, int(piece_samples)
    if piece < 1:
        raise SessionError(f"piece_samples = {piece} is not positive")
    sizes = [min(piece, S - f0) for f0 in range(0, S, piece)]
    pitch = [-(-w * n // 16) * 16 for n in sizes]
    out = np.full(B * sum(pitch), 0xA5, np.uint8)
    pitches = np.zeros(len(sizes), np.int64)
    valid = np.full((len(sizes), B), -1, np.int32)
    peaks = np.full((len(sizes), B), np.nan, np.float32)
    n = _ffi.load().vits_test_stream_pack(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, piece, C.byref(fmt), _ffi.ptr(out),
                                          out.nbytes, _ffi.ptr(pitches), _ffi.ptr(valid), _ffi.ptr(peaks), len(sizes))
    if n < 0:
        raise SessionError(f"vits_test_stream_pack failed [{n}]: {_ffi.last_error(None)}")
    chunks, off = [], 0
    for k in range(n):
        p = int(pitches[k])
        chunks.append(EncodedChunk(k * piece, out[off:off + B * p].reshape(B, p), valid[k], peaks[k], S))
        off += B * p
    return chunks


def test_stream_pack_shaped(x, counts, piece_samples, encoding="pcm16", ref_peak=None, volume=None, shapes=None, limit=None,
                            device_id=0):
    """vits_test_stream_pack_shaped: test_stream_pack through the shaped stream's kernels (shapes / limit as
    MiSession.synthesize_stream_encoded, or RawShapes / RawStreamLimit) -> (one EncodedChunk per piece that delivered
    something - first_sample and `data` [B, pitch] of the DELIVERED range -, [(first, n) delivered by every piece])."""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B, S = x.shape
    fmt, dtype = _stream_format(encoding, ref_peak, volume, B)
    shaping = _stream_shaping(shapes, limit, B)
    w, piece = np.dtype(dtype).itemsize, int(piece_samples)
    if piece < 1:
        raise SessionError(f"piece_samples = {piece} is not positive")
    n_pieces = -(-S // piece)
    out = np.full(B * (-(-w * S // 16) * 16 + 16 * n_pieces), 0xA5, np.uint8)
    pitches = np.zeros(n_pieces, np.int64)
    firsts, ns = np.full(n_pieces, -1, np.int64), np.full(n_pieces, -1, np.int64)
    valid = np.full((n_pieces, B), -1, np.int32)
    peaks = np.full((n_pieces, B), np.nan, np.float32)
    n = _ffi.load().vits_test_stream_pack_shaped(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, piece, C.byref(fmt),
                                                 None if shaping is None else C.byref(shaping), _ffi.ptr(out), out.nbytes,
                                                 _ffi.ptr(pitches), _ffi.ptr(valid), _ffi.ptr(peaks), _ffi.ptr(firsts), _ffi.ptr(ns),
                                                 n_pieces)
    if n < 0:
        raise SessionError(f"vits_test_stream_pack_shaped failed [{n}]: {_ffi.last_error(None)}")
    chunks, off = [], 0
    for k in range(n):
        p = int(pitches[k])
        if ns[k] > 0:
            chunks.append(EncodedChunk(int(firsts[k]), out[off:off + B * p].reshape(B, p), valid[k], peaks[k], S))
        off += B * p
    return chunks, [(int(f), int(c)) for f, c in zip(firsts[:n], ns[:n])]


def test_stream_pack_trimmed(x, counts, piece_samples, encoding="pcm16", ref_peak=None, volume=None, shapes=None, limit=None,
                             onsets=None, device_id=0):
    """vits_test_stream_pack_trimmed: test_stream_pack_shaped with onsets (as MiSession.synthesize_stream_encoded, or
    RawOnset) -> (chunks - each with its `skip` -, [(first, n) delivered by every piece], start int32 [B]: the rows' final
    a_b, INT32_MAX where a trimmed row has no onset)."""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B, S = x.shape
    fmt, dtype = _stream_format(encoding, ref_peak, volume, B)
    shaping = _stream_shaping(shapes, limit, B)
    trim = _stream_onsets(onsets, B)
    w, piece = np.dtype(dtype).itemsize, int(piece_samples)
    if piece < 1:
        raise SessionError(f"piece_samples = {piece} is not positive")
    n_pieces = -(-S // piece)
    out = np.full(B * (-(-w * S // 16) * 16 + 16 * n_pieces), 0xA5, np.uint8)
    pitches = np.zeros(n_pieces, np.int64)
    firsts, ns = np.full(n_pieces, -1, np.int64), np.full(n_pieces, -1, np.int64)
    valid, skip = np.full((n_pieces, B), -1, np.int32), np.full((n_pieces, B), -1, np.int32)
    peaks = np.full((n_pieces, B), np.nan, np.float32)
    start = np.full(B, -1, np.int32)
    n = _ffi.load().vits_test_stream_pack_trimmed(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, piece, C.byref(fmt),
                                                  None if shaping is None else C.byref(shaping), trim, _ffi.ptr(out), out.nbytes,
                                                  _ffi.ptr(pitches), _ffi.ptr(valid), _ffi.ptr(skip), _ffi.ptr(peaks), _ffi.ptr(firsts),
                                                  _ffi.ptr(ns), _ffi.ptr(start), n_pieces)
    if n < 0:
        raise SessionError(f"vits_test_stream_pack_trimmed failed [{n}]: {_ffi.last_error(None)}")
    chunks, off = [], 0
    for k in range(n):
        p = int(pitches[k])
        if ns[k] > 0:
            chunks.append(EncodedChunk(int(firsts[k]), out[off:off + B * p].reshape(B, p), valid[k], peaks[k], S, skip[k]))
        off += B * p
    return chunks, [(int(f), int(c)) for f, c in zip(firsts[:n], ns[:n])], start


# ---- the token-to-frame and frame-to-sample kernels by value (include/vitsmi.h: vits_test_durations ...) ----------------

def _test_deliver(stage, x, counts, segments, n_streams, encoding, device_id, dst=None, layout_only=False, trims=None, levels=None,
                  sample_rate=0, shapes=None, limits=None):
    """What the test_deliver* helpers share.  stage 0 .. 4: vits_test_deliver, _trimmed, _leveled, _shaped, _limited - each entry
    takes what the one before it takes and its own arrays.  -> the dict of test_deliver_leveled."""
    name = ("vits_test_deliver", "vits_test_deliver_trimmed", "vits_test_deliver_leveled", "vits_test_deliver_shaped",
            "vits_test_deliver_limited")[stage]
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B, S = x.shape
    segments = list(segments)
    code, dtype = _encoding(encoding)
    J = _n_streams(segments, n_streams)
    arr, n = _segments(segments)
    tarr, larr = _trims(trims, n), _levels(levels, n)
    sarr, parr, n_points = _shapes(shapes, n)
    if dst is None and not layout_only:
        dst = np.empty(delivery_plan(counts, segments, J, encoding, trims=trims)["total_bytes"], np.uint8)
    samples, offsets = np.zeros(max(J, 0), np.int64), np.zeros(max(J, 0) + 1, np.int64)
    first, count = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    loud, gain = np.full(max(n, 1), np.nan, np.float64), np.ones(max(n, 1), np.float32)
    args = [arr, tarr, larr, sarr, parr, n_points, _limits(limits, n)][:(1, 2, 3, 6, 7)[stage]] + [n, J, code] + [int(sample_rate)] * (stage >= 2)
    args += [None if layout_only else _ffi.ptr(dst), 0 if layout_only else dst.nbytes, _ffi.ptr(samples), _ffi.ptr(offsets)]
    args += [_ffi.ptr(first), _ffi.ptr(count), _ffi.ptr(loud), _ffi.ptr(gain)][:(0, 2, 4, 4, 4)[stage]]
    rc = getattr(_ffi.load(), name)(device_id, _ffi.ptr(x), _ffi.ptr(counts), B, S, *args)
    if rc != 0:
        raise SessionError(f"{name} failed [{rc}]: {_ffi.last_error(None)}")
    streams = None if layout_only else [dst[int(offsets[j]):int(offsets[j + 1])].view(dtype) for j in range(J)]
    return {"streams": streams, "stream_samples": samples, "stream_offsets": offsets, "kept_first": first[:n], "kept_count": count[:n],
            "loudness": loud[:n], "gain": gain[:n]}


def test_deliver(x, counts, segments, n_streams=None, encoding="pcm16", device_id=0, dst=None):
    """vits_test_deliver: x [B, S] float32 and the rows' valid samples through the delivery kernels -> one array per stream,
    views into `dst` (uint8; default: a buffer of exactly the plan's size, sized by delivery_plan).  A refusal raises
    SessionError and leaves a `dst` passed in untouched."""
    return _test_deliver(0, x, counts, segments, n_streams, encoding, device_id, dst)["streams"]


def test_deliver_trimmed(x, counts, segments, trims=None, n_streams=None, encoding="pcm16", device_id=0, dst=None, layout_only=False):
    """vits_test_deliver_trimmed: test_deliver with trims (one Trim, one per segment, or None) -> {"streams": one array per
    stream, views into `dst` (uint8; default: a buffer of the untrimmed plan's size with the tails), "stream_samples",
    "stream_offsets", "kept_first", "kept_count"}.  layout_only: dst = NULL - the scan runs, nothing is packed ("streams" is
    None).  A refusal raises SessionError and leaves a `dst` passed in untouched."""
    r = _test_deliver(1, x, counts, segments, n_streams, encoding, device_id, dst, layout_only, trims)
    return {k: v for k, v in r.items() if k not in ("loudness", "gain")}


def test_deliver_leveled(x, counts, segments, levels, sample_rate, trims=None, n_streams=None, encoding="pcm16", device_id=0,
                         layout_only=False):
    """vits_test_deliver_leveled: test_deliver_trimmed with levels (one Level, one per segment, or None) at sample_rate; the
    result holds "loudness" (float64 [G]) and "gain" (float32 [G]) too."""
    return _test_deliver(2, x, counts, segments, n_streams, encoding, device_id, None, layout_only, trims, levels, sample_rate)


def test_deliver_shaped(x, counts, segments, shapes, trims=None, levels=None, sample_rate=22050, n_streams=None, encoding="pcm16",
                        device_id=0, dst=None, layout_only=False):
    """vits_test_deliver_shaped: test_deliver_leveled with shapes (one Shape, one per segment, or None); `dst` as in
    test_deliver_trimmed: a refusal raises SessionError and leaves a `dst` passed in untouched."""
    return _test_deliver(3, x, counts, segments, n_streams, encoding, device_id, dst, layout_only, trims, levels, sample_rate, shapes)


def test_deliver_limited(x, counts, segments, limits, shapes=None, trims=None, levels=None, sample_rate=22050, n_streams=None,
                         encoding="pcm16", device_id=0, dst=None, layout_only=False):
    """vits_test_deliver_limited: test_deliver_shaped with limits (one Limit, one per segment - None in the list: off -, or
    None); `dst` as in test_deliver_trimmed: a refusal raises SessionError and leaves a `dst` passed in untouched."""
    return _test_deliver(4, x, counts, segments, n_streams, encoding, device_id, dst, layout_only, trims, levels, sample_rate, shapes,
                         limits)


def test_loudness_blocks(x, counts, sample_rate, firsts=None, device_id=0):
    """vits_test_loudness_blocks: x [B, S] float32, row b's kept range x[b, firsts[b] : firsts[b] + counts[b]] through the
    loudness kernels in one set of launches -> (one float32 array of sub-block energies per row, the compiled chunk Lc)"""
    x = np.ascontiguousarray(x, np.float32)
    counts = np.ascontiguousarray(counts, np.int64)
    B, S = x.shape
    firsts = np.zeros(B, np.int64) if firsts is None else np.ascontiguousarray(firsts, np.int64)
    hop = (int(sample_rate) + 5) // 10
    e = np.full(int(np.sum(np.maximum(counts, 0) // max(hop, 1))) + 1, np.nan, np.float32)
    n_sub, chunk = np.zeros(B, np.int32), C.c_int32()
    rc = _ffi.load().vits_test_loudness_blocks(device_id, _ffi.ptr(x), _ffi.ptr(counts), _ffi.ptr(firsts), B, S, int(sample_rate),
                                               _ffi.ptr(e), e.size, _ffi.ptr(n_sub), C.byref(chunk))
    if rc != 0:
        raise SessionError(f"vits_test_loudness_blocks failed [{rc}]: {_ffi.last_error(None)}")
    ends = np.cumsum(n_sub)
    return [e[int(b - n):int(b)].copy() for b, n in zip(ends, n_sub)], chunk.value


def loudness_chunk():
    """the compiled Lc of the loudness kernels (no device needed: the hook reports it before it looks at its arguments)"""
    chunk = C.c_int32()
    _ffi.load().vits_test_loudness_blocks(0, None, None, None, 0, 0, 0, None, 0, None, C.byref(chunk))
    return chunk.value


def _glue_check(rc, name):
    if rc != 0:
        raise SessionError(f"{name} failed [{rc}]: {_ffi.last_error(None)}")


def _rows3(rows, B):
    if rows is None:
        return None
    rows = np.ascontiguousarray(rows, np.float32)
    if rows.shape != (B, 3):
        raise SessionError(f"rows must be [B, 3] = [{B}, 3], got {rows.shape}")
    return rows


def test_durations(logw=None, dur=None, lens=None, length_scale=1.0, rows=None, token_rate=None, device_id=0):
    """duration_kernel (logw float32 [B, T]) or forced_duration_kernel (dur int64 [B, T]) -> (w_ceil float32 [B, T],
    cum int32 [B, T], y_len int32 [B]); rows [B, 3] (column 1: length_scale per utterance), token_rate [B, T]."""
    if (logw is None) == (dur is None):
        raise SessionError("one of logw and dur is needed")
    src = np.ascontiguousarray(logw, np.float32) if dur is None else np.ascontiguousarray(dur, np.int64)
    lens = np.ascontiguousarray(lens, np.int64)
    if src.ndim != 2 or lens.shape != (src.shape[0],):
        raise SessionError(f"logw / dur must be [B, T] and lens [B], got {src.shape} / {lens.shape}")
    B, T = src.shape
    rows = _rows3(rows, B)
    if token_rate is not None:
        token_rate = np.ascontiguousarray(token_rate, np.float32)
        if token_rate.shape != (B, T):
            raise SessionError(f"token_rate must be [B, T], got {token_rate.shape}")
    w_ceil = np.full((B, T), np.nan, np.float32)
    cum, y_len = np.full((B, T), -1, np.int32), np.full(B, -1, np.int32)
    rc = _ffi.load().vits_test_durations(device_id, _ffi.ptr(src) if dur is None else None, None if dur is None else _ffi.ptr(src),
                                         _ffi.ptr(lens), B, T, float(length_scale), _ffi.ptr(rows), _ffi.ptr(token_rate),
                                         _ffi.ptr(w_ceil), _ffi.ptr(cum), _ffi.ptr(y_len))
    _glue_check(rc, "vits_test_durations")
    return w_ceil, cum, y_len


def test_fit_durations(w, lens, fit, w_ceil=None, cum=None, y_len=None, device_id=0):
    """fit_duration_kernel by value (vits_test_fit_durations): weights float32 [B, T], lens [B], a Fit; w_ceil / cum / y_len -
    what rows of no group hold before the launch (default: a canary of -1s).  Returns (w_ceil float32 [B, T], cum int32
    [B, T], y_len int32 [B], scale float64 [G], frames int64 [G], status int32 [G])."""
    w = np.ascontiguousarray(w, np.float32)
    lens = np.ascontiguousarray(lens, np.int64)
    B, T = w.shape
    g32, t64 = np.ascontiguousarray(fit.groups, np.int32), np.ascontiguousarray(fit.target_frames, np.int64)
    m32 = np.array([int(v) for v in fit.modes], np.int32)
    G = len(t64)
    if g32.shape != (B,) or len(m32) != G:
        raise SessionError(f"test_fit_durations: groups {g32.shape} for {B} rows, {len(m32)} modes for {G} groups")
    c = _ffi.VitsFit(g32.ctypes.data, G, t64.ctypes.data, m32.ctypes.data)
    wc = np.full((B, T), -1, np.float32) if w_ceil is None else np.array(w_ceil, np.float32).reshape(B, T)
    cm = np.full((B, T), -1, np.int32) if cum is None else np.array(cum, np.int32).reshape(B, T)
    yl = np.full(B, -1, np.int32) if y_len is None else np.array(y_len, np.int32).reshape(B)
    scale, frames, status = np.zeros(G, np.float64), np.zeros(G, np.int64), np.zeros(G, np.int32)
    _glue_check(_ffi.load().vits_test_fit_durations(device_id, _ffi.ptr(w), _ffi.ptr(lens), B, T, C.byref(c), _ffi.ptr(wc), _ffi.ptr(cm),
                                                    _ffi.ptr(yl), _ffi.ptr(scale), _ffi.ptr(frames), _ffi.ptr(status)),
                "vits_test_fit_durations")
    return wc, cm, yl, scale, frames, status


def test_expand_prior(m_logs, cum, lens, y_len, F, noise=None, noise_scale=0.667, rows=None, seeds=None, noise_frames=None,
                      device_id=0):
    """expand_prior_strided_kernel: m_logs float32 [B, 2C, T] (m_p | logs_p), cum int32 [B, T], lens [B], y_len [B] -> z_p
    [B, C, F].  noise [B, C, Fn] (Fn < F reads as 0 behind Fn; noise_frames: how many of the Fn the kernel may read, Fn when
    None), else seeds uint64 [B]; rows [B, 3] (column 0: noise_scale per utterance)."""
    m_logs = np.ascontiguousarray(m_logs, np.float32)
    if m_logs.ndim != 3 or m_logs.shape[1] % 2:
        raise SessionError(f"m_logs must be [B, 2C, T], got {m_logs.shape}")
    B, C2, T = m_logs.shape
    Cc = C2 // 2
    cum = np.ascontiguousarray(cum, np.int32)
    lens = np.ascontiguousarray(lens, np.int64)
    y_len = np.ascontiguousarray(y_len, np.int32)
    if cum.shape != (B, T) or lens.shape != (B,) or y_len.shape != (B,):
        raise SessionError(f"cum must be [B, T], lens and y_len [B], got {cum.shape} / {lens.shape} / {y_len.shape}")
    rows = _rows3(rows, B)
    stride = 0
    if noise is not None:
        noise = np.ascontiguousarray(noise, np.float32)
        if noise.ndim != 3 or noise.shape[:2] != (B, Cc):
            raise SessionError(f"noise must be [B, C, Fn] = [{B}, {Cc}, Fn], got {noise.shape}")
        stride = noise.shape[2]
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, np.uint64)
        if seeds.shape != (B,):
            raise SessionError(f"seeds must be [B], got {seeds.shape}")
    F = int(F)
    z_p = np.full((B, Cc, max(F, 0)), np.nan, np.float32)
    rc = _ffi.load().vits_test_expand_prior(device_id, _ffi.ptr(m_logs), B, Cc, T, _ffi.ptr(cum), _ffi.ptr(lens), _ffi.ptr(y_len), F,
                                            _ffi.ptr(noise), stride, int(stride if noise_frames is None else noise_frames),
                                            float(noise_scale), _ffi.ptr(rows), _ffi.ptr(seeds), _ffi.ptr(z_p))
    _glue_check(rc, "vits_test_expand_prior")
    return z_p


def test_fill_normal(n, seed, stream_id, device_id=0):
    """fill_normal_kernel: the flat stream `stream_id` of `seed`, float32 [n]"""
    n = int(n)
    out = np.full(max(n, 0), np.nan, np.float32)
    rc = _ffi.load().vits_test_fill_normal(device_id, n, int(seed), int(stream_id), _ffi.ptr(out))
    _glue_check(rc, "vits_test_fill_normal")
    return out


def test_fill_normal_rows(T, channels, seeds, stream, rows, col, device_id=0):
    """fill_normal_rows_kernel: float32 [B, channels, T], utterance b's stream `stream` of seeds[b] times rows[b, col]"""
    seeds = np.ascontiguousarray(seeds, np.uint64)
    if seeds.ndim != 1:
        raise SessionError(f"seeds must be [B], got {seeds.shape}")
    B = seeds.shape[0]
    rows = _rows3(rows, B)
    T, channels = int(T), int(channels)
    out = np.full((B, max(channels, 0), max(T, 0)), np.nan, np.float32)
    rc = _ffi.load().vits_test_fill_normal_rows(device_id, B, channels, T, _ffi.ptr(seeds), int(stream), _ffi.ptr(rows), int(col),
                                                _ffi.ptr(out))
    _glue_check(rc, "vits_test_fill_normal_rows")
    return out


_POST_CONV_KERNELS = {"planar": 0, "blocked": 1, "blocked_generic": 2}


def test_post_conv(x, w, slope, vlen=None, hop=1, kernel="planar", device_id=0):
    """The vocoder's tail: x float32 [B, C, T], w [C, K] -> out [B, T] = tanh(conv_post(leaky_relu(x, slope))), zeros at and
    behind vlen[b] * hop.  kernel: "planar" (post_conv_tanh_kernel), "blocked" (post_conv_tanh_blocked_kernel, <7> when
    K == 7, else <0>) or "blocked_generic" (always <0>); for the blocked ones x is laid out as [C/8][T][8] here."""
    if kernel not in _POST_CONV_KERNELS:
        raise SessionError(f"unknown kernel {kernel!r}")
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    if x.ndim != 3 or w.ndim != 2 or w.shape[0] != x.shape[1]:
        raise SessionError(f"x must be [B, C, T] and w [C, K], got {x.shape} / {w.shape}")
    B, Cc, T = x.shape
    K = w.shape[1]
    if kernel != "planar":
        if Cc % 8:
            raise SessionError(f"the blocked layout holds 8 channels per cell: C={Cc}")
        x = np.ascontiguousarray(x.reshape(B, Cc // 8, 8, T).transpose(0, 1, 3, 2))
    if vlen is not None:
        vlen = np.ascontiguousarray(vlen, np.int64)
        if vlen.shape != (B,):
            raise SessionError(f"vlen must be [B], got {vlen.shape}")
    out = np.full((B, T), np.nan, np.float32)
    rc = _ffi.load().vits_test_post_conv(device_id, _ffi.ptr(x), B, Cc, T, _ffi.ptr(w), K, float(slope), _ffi.ptr(vlen), int(hop),
                                         _POST_CONV_KERNELS[kernel], _ffi.ptr(out))
    _glue_check(rc, "vits_test_post_conv")
    return out


# ---- the text-side kernels of the encoder and the stochastic duration predictor, by value.  Every wrapper returns the
# tensor AND the guard row behind it as the device left it (0xff bytes, NaN, where nothing wrote).

LN_GELU, LN_ACCUM, LN_MASK, LN_RELU_IN = 1, 2, 4, 8
_LN_FORMS = {"tile16": 0, "tile32": 1, "column": 2}


def _f32(a, shape, name):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape != tuple(shape):
        raise SessionError(f"{name} must be {list(shape)}, got {list(a.shape)}")
    return a


def _lens_or_none(lens, B):
    if lens is None:
        return None
    lens = np.ascontiguousarray(lens, np.int64)
    if lens.shape != (B,):
        raise SessionError(f"lens must be [B] = [{B}], got {lens.shape}")
    return lens


def _guarded(n, T):
    return np.zeros(n + T, np.float32)


def test_layernorm(x, gamma, beta, lens=None, flags=0, form="tile16", out_init=None, in_place=False, dw_w=None, dw_b=None,
                   dil=1, planes=False, device_id=0):
    """LayerNorm over channels of x float32 [B, C, T] through launch_layernorm (form: "tile16", "tile32", "column"), or -
    dw_w [C, K], dw_b [C] - depthwise conv + LN + GELU through launch_dw_ln.  flags: LN_GELU | LN_ACCUM | LN_MASK | LN_RELU_IN;
    out_init: the initial content of out (LN_ACCUM), in_place: x is.  Returns (out [B, C, T], guard [T]) and, with planes=True,
    also (planes uint16 [B, 3, C/8, T, 8], plane guard [T, 8])."""
    if form not in _LN_FORMS:
        raise SessionError(f"unknown form {form!r}")
    x = np.ascontiguousarray(x, np.float32)
    if x.ndim != 3:
        raise SessionError(f"x must be [B, C, T], got {x.shape}")
    B, Cc, T = x.shape
    gamma, beta = _f32(gamma, (Cc,), "gamma"), _f32(beta, (Cc,), "beta")
    lens = _lens_or_none(lens, B)
    if out_init is not None:
        out_init = _f32(out_init, x.shape, "out_init")
    K = 1
    if dw_w is not None:
        dw_w = np.ascontiguousarray(dw_w, np.float32)
        if dw_w.ndim != 2 or dw_w.shape[0] != Cc:
            raise SessionError(f"dw_w must be [C, K], got {dw_w.shape}")
        K = dw_w.shape[1]
        dw_b = _f32(dw_b, (Cc,), "dw_b")
    n = B * Cc * T
    out = _guarded(n, T)
    pl = np.zeros(n * 3 + T * 8, np.uint16) if planes else None
    rc = _ffi.load().vits_test_layernorm(device_id, _ffi.ptr(x), _ffi.ptr(out_init), B, Cc, T, _ffi.ptr(gamma), _ffi.ptr(beta),
                                         _ffi.ptr(lens), int(flags), _LN_FORMS[form], int(bool(in_place)), _ffi.ptr(dw_w),
                                         _ffi.ptr(dw_b), int(K), int(dil), _ffi.ptr(out), _ffi.ptr(pl))
    _glue_check(rc, "vits_test_layernorm")
    res = (out[:n].reshape(B, Cc, T), out[n:])
    if planes:
        res += (pl[:n * 3].reshape(B, 3, Cc // 8, T, 8), pl[n * 3:].reshape(T, 8))
    return res


def test_dds(x, lens, layers, form=16, mask_out=True, head=None, tail=None, device_id=0):
    """A stack of fused DDSConv layers on x float32 [B, C, T]: form 16 (dds_layer16_kernel) or 32 (dds_layer_kernel); layers =
    a list of dicts with dw_w [C, 3], dw_b, ln1_g, ln1_b, pw_w [C, C], pw_b, ln2_g, ln2_b, dil.  mask_out=False: one layer with
    its mask off.  head = dict(cond [B, C, T], z [B, 2, T], ch, pre_w [C], pre_b [C]) (form 16; x may be None), tail =
    dict(w [R, C], b [R] or None) (form 16).  Returns (the stack's result [B, C, T] - or tail_out [B, R, T] - and guard [T])."""
    lens = np.ascontiguousarray(lens, np.int64)
    src = head["cond"] if x is None and head is not None else x
    src = np.ascontiguousarray(src, np.float32)
    if src.ndim != 3 or lens.shape != (src.shape[0],):
        raise SessionError(f"x must be [B, C, T] and lens [B], got {src.shape} / {lens.shape}")
    B, Cc, T = src.shape
    x = None if x is None else src
    keep = []
    arr = (_ffi.VitsTestDdsLayer * len(layers))()
    for i, L in enumerate(layers):
        for name, shape in (("dw_w", (Cc, 3)), ("dw_b", (Cc,)), ("ln1_g", (Cc,)), ("ln1_b", (Cc,)), ("pw_w", (Cc, Cc)),
                            ("pw_b", (Cc,)), ("ln2_g", (Cc,)), ("ln2_b", (Cc,))):
            a = _f32(L[name], shape, f"layers[{i}].{name}")
            keep.append(a)
            setattr(arr[i], name, a.ctypes.data)
        arr[i].dil = int(L["dil"])
    hc = hz = hw = hb = tw = tb = None
    hch, R = 0, 0
    if head is not None:
        hc, hz = _f32(head["cond"], (B, Cc, T), "head.cond"), _f32(head["z"], (B, 2, T), "head.z")
        hw, hb = _f32(head["pre_w"], (Cc,), "head.pre_w"), _f32(head["pre_b"], (Cc,), "head.pre_b")
        hch = int(head["ch"])
    if tail is not None:
        tw = np.ascontiguousarray(tail["w"], np.float32)
        if tw.ndim != 2 or tw.shape[1] != Cc:
            raise SessionError(f"tail.w must be [R, C], got {tw.shape}")
        R = tw.shape[0]
        tb = None if tail.get("b") is None else _f32(tail["b"], (R,), "tail.b")
    rows = R if tail is not None else Cc
    out = _guarded(B * rows * T, T)
    rc = _ffi.load().vits_test_dds(device_id, int(form), _ffi.ptr(x), B, Cc, T, _ffi.ptr(lens), len(layers), arr, int(bool(mask_out)),
                                   _ffi.ptr(hc), _ffi.ptr(hz), hch, _ffi.ptr(hw), _ffi.ptr(hb), _ffi.ptr(tw), _ffi.ptr(tb), R,
                                   _ffi.ptr(out))
    _glue_check(rc, "vits_test_dds")
    del keep
    return out[:B * rows * T].reshape(B, rows, T), out[B * rows * T:]


def test_cf_pre(z, ch, w, bias, cond, device_id=0):
    """cf_pre_kernel: out = w[c] * z[b, ch, t] + bias[c] + cond[b, c, t]; z [B, 2, T], cond [B, C, T] -> (out, guard [T])"""
    cond = np.ascontiguousarray(cond, np.float32)
    if cond.ndim != 3:
        raise SessionError(f"cond must be [B, C, T], got {cond.shape}")
    B, Cc, T = cond.shape
    z, w, bias = _f32(z, (B, 2, T), "z"), _f32(w, (Cc,), "w"), _f32(bias, (Cc,), "bias")
    out = _guarded(B * Cc * T, T)
    rc = _ffi.load().vits_test_cf_pre(device_id, _ffi.ptr(z), int(ch), _ffi.ptr(w), _ffi.ptr(bias), _ffi.ptr(cond), B, Cc, T, _ffi.ptr(out))
    _glue_check(rc, "vits_test_cf_pre")
    return out[:B * Cc * T].reshape(B, Cc, T), out[B * Cc * T:]


def test_rqs_inverse(pr, z, lens, ch0, nb, sqrt_c, device_id=0):
    """rqs_inverse_kernel (<10> for nb <= 10, else <16>): z float32 [B, 2, T] with channel ch0 passing through and channel
    ch0 ^ 1 transformed by the spline of pr [B, 3 nb - 1, T] -> (z [B, 2, T], guard [T])"""
    z = np.ascontiguousarray(z, np.float32)
    if z.ndim != 3 or z.shape[1] != 2:
        raise SessionError(f"z must be [B, 2, T], got {z.shape}")
    B, _, T = z.shape
    nb = int(nb)
    pr = _f32(pr, (B, 3 * nb - 1, T), "pr")
    lens = _lens_or_none(lens, B)
    out = _guarded(B * 2 * T, T)
    rc = _ffi.load().vits_test_rqs_inverse(device_id, _ffi.ptr(pr), _ffi.ptr(z), B, T, _ffi.ptr(lens), int(ch0), nb, float(sqrt_c),
                                           _ffi.ptr(out))
    _glue_check(rc, "vits_test_rqs_inverse")
    return out[:B * 2 * T].reshape(B, 2, T), out[B * 2 * T:]


def test_ea_logw(z, ch, m0, logs0, lens, device_id=0):
    """ea_logw_kernel: logw = (z[b, ch, t] - m0) * exp(-logs0) * mask -> (logw [B, T], guard [T])"""
    z = np.ascontiguousarray(z, np.float32)
    if z.ndim != 3 or z.shape[1] != 2:
        raise SessionError(f"z must be [B, 2, T], got {z.shape}")
    B, _, T = z.shape
    lens = _lens_or_none(lens, B)
    out = _guarded(B * T, T)
    rc = _ffi.load().vits_test_ea_logw(device_id, _ffi.ptr(z), int(ch), float(m0), float(logs0), _ffi.ptr(lens), B, T, _ffi.ptr(out))
    _glue_check(rc, "vits_test_ea_logw")
    return out[:B * T].reshape(B, T), out[B * T:]
