"""Fitted durations (include/vitsmi.h, "fitted durations") restated in NumPy: the cleaning, the count, the largest
multiplier of [2^-4, 2^4] whose count stays within the target, and the hand-out of the remaining frames.  Everything behind
the fp32 weight is IEEE double and int64, so the engine's results are compared with these by exact equality."""
import numpy as np

MET, FLOOR, CEIL, KEPT = 0, 1, 2, 3
LO_BITS = int(np.float64(2.0 ** -4).view(np.uint64))
ONE_BITS = int(np.float64(1.0).view(np.uint64))
HI_BITS = int(np.float64(2.0 ** 4).view(np.uint64))


def clean(w):
    w = np.asarray(w, np.float32)
    ok = np.isfinite(w) & (w > 0)
    return np.minimum(np.where(ok, w, np.float32(0)), np.float32(2.0 ** 24)).astype(np.float32)


def scale_of(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def terms(wc, s):
    """(int64) ceil((double) w * s) per token: one double product"""
    return np.ceil(wc.astype(np.float64) * np.float64(s)).astype(np.int64)


def fit_group(wc, F, mode):
    """wc: the group's cleaned weights in (row, t) order -> (durations int64, s*, frames, status)"""
    def count(bits):
        return int(terms(wc, scale_of(bits)).sum())

    def done(bits, status):
        d = terms(wc, scale_of(bits))
        return d, scale_of(bits), int(d.sum()), status

    hi = HI_BITS
    if mode == 2:
        if count(ONE_BITS) <= F:
            return done(ONE_BITS, KEPT)
        hi = ONE_BITS
    if count(LO_BITS) > F:
        return done(LO_BITS, FLOOR)
    lo = LO_BITS
    if count(hi) <= F:  # (mode 1 only: in mode 2 count(1.0) > F is known)
        return done(hi, CEIL if count(hi) < F else MET)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= F:
            lo = mid
        else:
            hi = mid
    d = terms(wc, scale_of(lo))
    R = F - int(d.sum())
    cand = np.flatnonzero(terms(wc, scale_of(lo + 1)) > d)
    assert len(cand) >= R, (len(cand), R)
    d[cand[:R]] += 1
    return d, scale_of(lo), int(d.sum()), MET


def fit(w, lens, groups, targets, modes):
    """w [B][T] fp32, lens [B], groups [B] in [-1, G), targets / modes [G] ->
    (durations int64 [B][T] with -1 in the rows of no group, scale float64 [G], frames int64 [G], status int32 [G])"""
    w = np.asarray(w, np.float32)
    B, T = w.shape
    G = len(targets)
    dur = np.full((B, T), -1, np.int64)
    scale, frames, status = np.zeros(G, np.float64), np.zeros(G, np.int64), np.zeros(G, np.int32)
    for g in range(G):
        rows = [b for b in range(B) if groups[b] == g]
        wc = clean(np.concatenate([w[b, :int(lens[b])] for b in rows]) if rows else np.zeros(0, np.float32))
        d, scale[g], frames[g], status[g] = fit_group(wc, int(targets[g]), int(modes[g]))
        at = 0
        for b in rows:
            L = int(lens[b])
            dur[b] = 0
            dur[b, :L] = d[at:at + L]
            at += L
    return dur, scale, frames, status


def per_row(dur, lens):
    """what the engine leaves per row of durations int64 [B][T]: (w_ceil float32, cum int32, y_len int32)"""
    d = np.asarray(dur, np.int64)
    return d.astype(np.float32), np.cumsum(d, axis=1).astype(np.int32), np.maximum(d.sum(axis=1), 1).astype(np.int32)
