// warp.hpp — the plan of the per-token time warp (include/vitsmi.h, "Intonation"): a token's step, cutoff and half-taps,
// a row's segments and output count, and the prototype table G, computed in double on the host and rounded once to fp32.
// Host-side C++17, no HIP types: the plan is a pure function of the durations and the semitones, answered without a handle
// or a device.  All position arithmetic is int64 (Q16 input positions).
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"
#include "resample.hpp"

namespace vitsmi {

constexpr int kWarpZ = kResampleZ;         // zero crossings on either side, as the resampler
constexpr int kWarpR = 512;                // table entries per zero crossing
constexpr int kWarpFB = 16;                // fractional bits of an input position
constexpr int64_t kWarpOne = int64_t(1) << kWarpFB;
constexpr int kWarpTable = kWarpZ * kWarpR + 2;  // G[0 .. Z*R + 1]; the last two are 0
constexpr float kWarpMaxSemitones = 12.f;
constexpr int64_t kWarpMinStep = kWarpOne / 2, kWarpMaxStep = kWarpOne * 2;  // -12 and +12 semitones
constexpr int kWarpMaxHalf = 38;           // half-taps at +12 semitones: the most a token has

constexpr int64_t kGlideMaxSpan = int64_t(1) << 23;  // output samples a gliding token has at most: |b - a| * j * (j - 1) stays in int64

static_assert(sizeof(vits_warp_seg) == 40, "vits_warp_seg is a 40-byte record");
static_assert(sizeof(vits_glide_seg) == sizeof(vits_warp_seg), "carve_warp carves the plan block of either record");

#if defined(__HIPCC__)
#define VITSMI_HD __host__ __device__
#else
#define VITSMI_HD
#endif

// a row of a launch: its segment records, its valid input samples, its output samples
struct WarpRow {
    int32_t seg0, n_segs;  // records [seg0, seg0 + n_segs) of the launch's segment array
    int32_t n_in, n_out;
    int32_t identity;      // a masked copy: no segment, or every step the unit step
};

// G[i] = (float)g(i / R), g(u) = sinc(u) * kaiser(u / Z) for 0 <= u < Z, else 0
inline void warp_table(float *G) {
    const double kPi = 3.14159265358979323846;
    const double i0b = resample_i0(kResampleBeta);
    for (int i = 0; i < kWarpTable; i++) {
        const double u = (double)i / kWarpR;
        double g = 0.0;
        if (u < (double)kWarpZ) {
            const double a = kPi * u, t = u / kWarpZ;
            g = (a == 0.0 ? 1.0 : std::sin(a) / a) * resample_i0(kResampleBeta * std::sqrt(1.0 - t * t)) / i0b;
        }
        G[i] = (float)g;
    }
}

// step, cutoff c and half-taps Kh of a token at `semitones`; false: not a finite value within [-12, 12]
inline bool warp_token(float semitones, int64_t &step, int64_t &c, int32_t &Kh) {
    if (!std::isfinite(semitones) || std::fabs(semitones) > kWarpMaxSemitones) return false;
    const double r = std::exp2((double)semitones / 12.0);
    step = std::llrint(r * (double)kWarpOne);
    const double q = (double)kWarpOne / (double)step;
    const double s = kResampleRolloff * (q < 1.0 ? q : 1.0);
    c = std::llrint(s * (double)kWarpOne);
    Kh = (int32_t)(((int64_t)kWarpZ * kWarpOne + c - 1) / c);
    return true;
}

// The plan of one row: tokens [0, len) with rendered durations D_t (frames) and semitones st_t.  segs == nullptr: counts
// only.  spans[t] (nullable): k of token t, 0 for a dropped one.  Returns "" or what is wrong, naming the token.
inline std::string warp_plan(const int64_t *durations, const float *semitones, int len, int hop, vits_warp_seg *segs, int64_t *spans,
                             int64_t &n_segs, int64_t &n_out) {
    char buf[200];
    int64_t pos = 0, n = 0, cum = 0;
    n_segs = 0;
    for (int t = 0; t < len; t++) {
        if (spans) spans[t] = 0;
        const int64_t D = durations[t];
        if (D < 0) {
            std::snprintf(buf, sizeof buf, "token %d: duration %lld is negative", t, (long long)D);
            return buf;
        }
        if (D == 0) continue;
        int64_t step, c;
        int32_t Kh;
        if (!warp_token(semitones ? semitones[t] : 0.f, step, c, Kh)) {
            std::snprintf(buf, sizeof buf, "token %d: semitones %g is not a finite value within [-12, 12]", t, (double)semitones[t]);
            return buf;
        }
        cum += D;
        if (cum > (INT64_MAX >> (kWarpFB + 2)) / hop) {
            std::snprintf(buf, sizeof buf, "token %d: %lld frames of %d samples leave the range of a position", t, (long long)cum, hop);
            return buf;
        }
        const int64_t P = (cum * hop) << kWarpFB;
        const int64_t k = P <= pos ? 0 : (P - pos + step - 1) / step;
        if (segs) segs[n_segs] = vits_warp_seg{n, pos, k, (int32_t)step, (int32_t)c, Kh, 0};
        if (spans) spans[t] = k;
        n_segs++;
        n += k;
        pos += k * step;
        if (n > INT_MAX) {
            std::snprintf(buf, sizeof buf, "token %d: the row reaches %lld output samples, more than a row admits (%d)", t, (long long)n, INT_MAX);
            return buf;
        }
    }
    n_out = n;
    return "";
}

// every step of the row is the unit step: a masked copy (a row without a segment too)
inline bool warp_identity(const vits_warp_seg *segs, int64_t n_segs) {
    for (int64_t j = 0; j < n_segs; j++)
        if (segs[j].step != kWarpOne) return false;
    return true;
}

// ---- pitch contours (include/vitsmi.h, "pitch contours"): the speed moves linearly from step0 to step1 across a token

// THE cutoff of an output sample whose speed is `step` (Q16, within [kWarpMinStep, kWarpMaxStep]), in integers: for every such
// step the c and Kh warp_token derives in double.  Host plan, hooks and glide_kernel call this one function.
VITSMI_HD inline void glide_cutoff(int64_t step, int32_t &c, int32_t &Kh) {
    c = step <= kWarpOne ? 55706 : (int32_t)(((uint64_t(17) << 32) + 10u * (uint64_t)step) / (20u * (uint64_t)step));
    Kh = (int32_t)(((uint32_t)kWarpZ * (uint32_t)kWarpOne + (uint32_t)c - 1u) / (uint32_t)c);
}

// Q16 input position of sample j (0 <= j <= k; j == k: where the next token starts) of the record {pos0, k, a, b}:
// pos0 + j * a + sgn * floor(|b - a| * j * (j - 1) / (2 k)).  The numerator is below 2^17 * 2^23 * 2^23.
VITSMI_HD inline int64_t glide_pos(int64_t pos0, int64_t k, int32_t a, int32_t b, int64_t j) {
    const uint64_t d = (uint64_t)(b >= a ? b - a : a - b);
    if (d == 0 || j < 2) return pos0 + j * a;
    const int64_t q = (int64_t)(d * (uint64_t)j * (uint64_t)(j - 1) / (2u * (uint64_t)k));
    return pos0 + j * a + (b >= a ? q : -q);
}

// the speed of that sample: a + sgn * floor(|b - a| * j / k)
VITSMI_HD inline int64_t glide_step(int64_t k, int32_t a, int32_t b, int64_t j) {
    const uint64_t d = (uint64_t)(b >= a ? b - a : a - b);
    if (d == 0 || j == 0) return a;
    const int64_t q = (int64_t)(d * (uint64_t)j / (uint64_t)k);
    return b >= a ? a + q : a - q;
}

// the two steps of a token and the factor its duration takes under compensate: (float)((r0 + r1) / 2); false: a value is
// not finite within [-12, 12] (*bad: 0 the start value, 1 the end value)
inline bool glide_token(float st0, float st1, int64_t &a, int64_t &b, float &rate, int *bad = nullptr) {
    int64_t c;
    int32_t Kh;
    if (!warp_token(st0, a, c, Kh)) {
        if (bad) *bad = 0;
        return false;
    }
    if (!warp_token(st1, b, c, Kh)) {
        if (bad) *bad = 1;
        return false;
    }
    rate = (float)((std::exp2((double)st0 / 12.0) + std::exp2((double)st1 / 12.0)) * 0.5);
    return true;
}

// warp_plan's sibling: token t glides from st0[t] to st1[t] (st0 == nullptr: zeros; st1 == nullptr: = st0)
inline std::string glide_plan(const int64_t *durations, const float *st0, const float *st1, int len, int hop, vits_glide_seg *segs,
                              int64_t *spans, int64_t &n_segs, int64_t &n_out) {
    char buf[200];
    int64_t pos = 0, n = 0, cum = 0;
    n_segs = 0;
    for (int t = 0; t < len; t++) {
        if (spans) spans[t] = 0;
        const int64_t D = durations[t];
        if (D < 0) {
            std::snprintf(buf, sizeof buf, "token %d: duration %lld is negative", t, (long long)D);
            return buf;
        }
        if (D == 0) continue;
        const float v0 = st0 ? st0[t] : 0.f, v1 = st1 ? st1[t] : v0;
        int64_t a, b;
        float rate;
        int bad = 0;
        if (!glide_token(v0, v1, a, b, rate, &bad)) {
            std::snprintf(buf, sizeof buf, "token %d: semitones %g is not a finite value within [-12, 12]", t, (double)(bad ? v1 : v0));
            return buf;
        }
        cum += D;
        if (cum > (INT64_MAX >> (kWarpFB + 2)) / hop) {
            std::snprintf(buf, sizeof buf, "token %d: %lld frames of %d samples leave the range of a position", t, (long long)cum, hop);
            return buf;
        }
        const int64_t P = (cum * hop) << kWarpFB;
        const int64_t k = P <= pos ? 0 : (2 * (P - pos) + (a + b) - 1) / (a + b);
        if (k > kGlideMaxSpan) {
            std::snprintf(buf, sizeof buf, "token %d: %lld output samples, more than a gliding token admits (%lld)", t, (long long)k,
                          (long long)kGlideMaxSpan);
            return buf;
        }
        if (segs) segs[n_segs] = vits_glide_seg{n, pos, k, (int32_t)a, (int32_t)b, {0, 0}};
        if (spans) spans[t] = k;
        n_segs++;
        n += k;
        pos = glide_pos(pos, k, (int32_t)a, (int32_t)b, k);
        if (n > INT_MAX) {
            std::snprintf(buf, sizeof buf, "token %d: the row reaches %lld output samples, more than a row admits (%d)", t, (long long)n, INT_MAX);
            return buf;
        }
    }
    n_out = n;
    return "";
}

// every token of the row keeps the unit step: a masked copy (a row without a segment too)
inline bool warp_identity(const vits_glide_seg *segs, int64_t n_segs) {
    for (int64_t j = 0; j < n_segs; j++)
        if (segs[j].step0 != kWarpOne || segs[j].step1 != kWarpOne) return false;
    return true;
}

// the rows' records of a launch from each row's segments [seg_first[b], seg_first[b + 1]) and valid input samples
// (a row without a segment: N_b = n_b); returns S_w = max(1, max_b N_b)
template <class Seg>
inline int64_t warp_rows(const Seg *segs, const int32_t *seg_first, const int64_t *n_in, int B, std::vector<WarpRow> &rows) {
    rows.resize((size_t)B);
    int64_t S_w = 1;
    for (int b = 0; b < B; b++) {
        const int32_t s0 = seg_first[b], ns = seg_first[b + 1] - s0;
        const int64_t N = ns > 0 ? segs[s0 + ns - 1].n0 + segs[s0 + ns - 1].k : n_in[b];
        rows[(size_t)b] = WarpRow{s0, ns, (int32_t)n_in[b], (int32_t)N, warp_identity(segs + s0, ns) ? 1 : 0};
        S_w = N > S_w ? N : S_w;
    }
    return S_w;
}

// "" or what keeps a row's segment records from being rendered: each within the limits a token has, each starting where the
// one before it ends - in output samples and in input position -, so that positions never decrease along the row
inline std::string warp_segs_fault(const vits_warp_seg *segs, int64_t n_segs) {
    char buf[200];
    int64_t n = 0, pos = 0;
    for (int64_t j = 0; j < n_segs; j++) {
        const vits_warp_seg &g = segs[j];
        const bool first = j == 0;
        if (g.step < kWarpMinStep || g.step > kWarpMaxStep || g.c < 1 || g.c > kWarpOne || g.half_taps < 1 || g.half_taps > kWarpMaxHalf ||
            (int64_t)g.half_taps * g.c < (int64_t)kWarpZ * kWarpOne || g.k < 0 || g.k > INT_MAX || g.n0 != n ||
            (first ? g.pos0 != 0 : g.pos0 != pos)) {
            std::snprintf(buf, sizeof buf, "segment %lld {n0 %lld, pos0 %lld, k %lld, step %d, c %d, half_taps %d} does not continue the row at "
                                           "output %lld, position %lld within the limits of a token",
                          (long long)j, (long long)g.n0, (long long)g.pos0, (long long)g.k, g.step, g.c, g.half_taps, (long long)n, (long long)pos);
            return buf;
        }
        n += g.k;
        pos = g.pos0 + g.k * (int64_t)g.step;
        if (n > INT_MAX) {
            std::snprintf(buf, sizeof buf, "segment %lld: the row reaches %lld output samples, more than a row admits (%d)", (long long)j, (long long)n, INT_MAX);
            return buf;
        }
    }
    return "";
}

// warp_segs_fault's sibling: each record within the limits of a gliding token, each starting where the closed form
// (glide_pos at j = k) ends the one before it
inline std::string glide_segs_fault(const vits_glide_seg *segs, int64_t n_segs) {
    char buf[240];
    int64_t n = 0, pos = 0;
    for (int64_t j = 0; j < n_segs; j++) {
        const vits_glide_seg &g = segs[j];
        if (g.step0 < kWarpMinStep || g.step0 > kWarpMaxStep || g.step1 < kWarpMinStep || g.step1 > kWarpMaxStep || g.k < 0 ||
            g.k > kGlideMaxSpan || g.n0 != n || g.pos0 != pos) {
            std::snprintf(buf, sizeof buf, "segment %lld {n0 %lld, pos0 %lld, k %lld, step0 %d, step1 %d} does not continue the row at "
                                           "output %lld, position %lld within the limits of a token",
                          (long long)j, (long long)g.n0, (long long)g.pos0, (long long)g.k, g.step0, g.step1, (long long)n, (long long)pos);
            return buf;
        }
        n += g.k;
        pos = glide_pos(g.pos0, g.k, g.step0, g.step1, g.k);
        if (n > INT_MAX) {
            std::snprintf(buf, sizeof buf, "segment %lld: the row reaches %lld output samples, more than a row admits (%d)", (long long)j, (long long)n, INT_MAX);
            return buf;
        }
    }
    return "";
}

// ---- streamed pitch (include/vitsmi.h, "streamed pitch"): which output samples exist once input samples [0, X) do

// Q16 input position of sample j of a record, by the closed form of its family
VITSMI_HD inline int64_t warp_seg_pos(const vits_warp_seg &g, int64_t j) { return g.pos0 + j * (int64_t)g.step; }
VITSMI_HD inline int64_t warp_seg_pos(const vits_glide_seg &g, int64_t j) { return glide_pos(g.pos0, g.k, g.step0, g.step1, j); }

// Q16 input position of output sample n (0 <= n < N) of a row; a row without a record is the masked copy: n itself
template <class Seg>
inline int64_t warp_row_pos(const Seg *segs, int64_t n_segs, int64_t n) {
    if (n_segs <= 0) return n << kWarpFB;
    int64_t lo = 0, hi = n_segs - 1;  // the last record whose n0 <= n, as warp_find on the device
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].n0 <= n) lo = mid;
        else hi = mid - 1;
    }
    return warp_seg_pos(segs[lo], n - segs[lo].n0);
}

// ready_b(X): how many n < N have (pos_n >> FB) + kWarpMaxHalf < X - every input a tile stages for them exists.  Positions never
// decrease along a row, so it is a prefix count: bisection over n.
template <class Seg>
inline int64_t warp_ready(const Seg *segs, int64_t n_segs, int64_t N, int64_t X) {
    int64_t lo = 0, hi = N;  // samples [0, lo) are ready, sample hi (if any) is not
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((warp_row_pos(segs, n_segs, mid) >> kWarpFB) + kWarpMaxHalf < X) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ... and what the row admits: a row whose n_in valid inputs all exist (X >= n_in) is complete - N
template <class Seg>
inline int64_t warp_emit_row(const Seg *segs, int64_t n_segs, int64_t n_in, int64_t N, int64_t X) {
    return X >= n_in ? N : warp_ready(segs, n_segs, N, X);
}

// e(X) of a launch's rows: the least ready count among the rows still short of input; S_w without one, or on the last piece
template <class Seg>
inline int64_t warp_emit_end(const Seg *segs, const std::vector<WarpRow> &rows, int64_t S_w, int64_t X, bool is_last) {
    int64_t e = S_w;
    if (is_last) return e;
    for (const WarpRow &r : rows) {
        if (X >= r.n_in) continue;
        const int64_t q = warp_ready(segs + r.seg0, r.n_segs, r.n_out, X);
        e = q < e ? q : e;
    }
    return e;
}

// n_cap: output samples one delivery of a streamed run holds at most.  A piece of `piece_in` input samples moves every position's
// bound by that much, which at the least step ONE / 2 completes 2 * piece_in outputs, and the uniform kWarpMaxHalf of the rule may
// fall on either side of it: 2 * (piece_in + kWarpMaxHalf).  Longer ranges - a slow row's end releasing the others - are cut.
inline int64_t warp_stream_cap(int64_t piece_in, int64_t S_w) {
    const int64_t cap = 2 * (piece_in + kWarpMaxHalf);
    return cap < S_w ? cap : S_w;
}

// The plans of a batch from the durations [B][T] (any arithmetic type: frames) and the rows' valid input samples: plan_row plans
// one row into its records.  segs / first / spans [B][T] / rows are filled; returns "" or "row b, ..." - what is wrong.
template <class Seg, class Dur, class PlanRow>
inline std::string warp_plan_rows(const Dur *durations, const int64_t *lens, const int64_t *n_in, int B, int T, int hop, PlanRow plan_row,
                                  std::vector<Seg> &segs, std::vector<int32_t> &first, std::vector<int64_t> &spans, std::vector<WarpRow> &rows,
                                  int64_t &S_w) {
    segs.clear();
    first.assign((size_t)B + 1, 0);
    spans.assign((size_t)B * T, 0);
    std::vector<int64_t> dur((size_t)T);
    for (int b = 0; b < B; b++) {
        const int L = (int)lens[b];
        for (int t = 0; t < L; t++) dur[t] = (int64_t)durations[(size_t)b * T + t];
        const size_t at = segs.size();
        segs.resize(at + (size_t)L);
        int64_t ns = 0, N = 0;
        const std::string e = plan_row(b, dur.data(), L, hop, segs.data() + at, spans.data() + (size_t)b * T, ns, N);
        if (!e.empty()) return "row " + std::to_string(b) + ", " + e;
        segs.resize(at + (size_t)ns);
        first[(size_t)b + 1] = (int32_t)segs.size();
    }
    S_w = warp_rows(segs.data(), first.data(), n_in, B, rows);
    return "";
}

}  // namespace vitsmi
