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
template <class Token>
inline std::string warp_plan_as(Token token, const int64_t *durations, const float *semitones, int len, int hop, vits_warp_seg *segs,
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
        int64_t step, c;
        int32_t Kh;
        if (!token(semitones ? semitones[t] : 0.f, step, c, Kh)) {
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

inline std::string warp_plan(const int64_t *durations, const float *semitones, int len, int hop, vits_warp_seg *segs, int64_t *spans,
                             int64_t &n_segs, int64_t &n_out) {
    return warp_plan_as(warp_token, durations, semitones, len, hop, segs, spans, n_segs, n_out);
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
template <class Token>
inline std::string glide_plan_as(Token token, int64_t max_span, const int64_t *durations, const float *st0, const float *st1, int len, int hop,
                                 vits_glide_seg *segs, int64_t *spans, int64_t &n_segs, int64_t &n_out) {
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
        if (!token(v0, v1, a, b, rate, &bad)) {
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
        if (k > max_span) {
            std::snprintf(buf, sizeof buf, "token %d: %lld output samples, more than a gliding token admits (%lld)", t, (long long)k,
                          (long long)max_span);
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

inline std::string glide_plan(const int64_t *durations, const float *st0, const float *st1, int len, int hop, vits_glide_seg *segs,
                              int64_t *spans, int64_t &n_segs, int64_t &n_out) {
    return glide_plan_as([](float v0, float v1, int64_t &a, int64_t &b, float &rate, int *bad) { return glide_token(v0, v1, a, b, rate, bad); },
                         kGlideMaxSpan, durations, st0, st1, len, hop, segs, spans, n_segs, n_out);
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
inline std::string warp_segs_fault_in(const vits_warp_seg *segs, int64_t n_segs, int64_t min_step, int64_t max_step, int max_half) {
    char buf[200];
    int64_t n = 0, pos = 0;
    for (int64_t j = 0; j < n_segs; j++) {
        const vits_warp_seg &g = segs[j];
        const bool first = j == 0;
        if (g.step < min_step || g.step > max_step || g.c < 1 || g.c > kWarpOne || g.half_taps < 1 || g.half_taps > max_half ||
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

inline std::string warp_segs_fault(const vits_warp_seg *segs, int64_t n_segs) {
    return warp_segs_fault_in(segs, n_segs, kWarpMinStep, kWarpMaxStep, kWarpMaxHalf);
}

// warp_segs_fault's sibling: each record within the limits of a gliding token, each starting where the closed form
// (glide_pos at j = k) ends the one before it
inline std::string glide_segs_fault_in(const vits_glide_seg *segs, int64_t n_segs, int64_t min_step, int64_t max_step, int64_t max_span) {
    char buf[240];
    int64_t n = 0, pos = 0;
    for (int64_t j = 0; j < n_segs; j++) {
        const vits_glide_seg &g = segs[j];
        if (g.step0 < min_step || g.step0 > max_step || g.step1 < min_step || g.step1 > max_step || g.k < 0 || g.k > max_span || g.n0 != n ||
            g.pos0 != pos) {
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

inline std::string glide_segs_fault(const vits_glide_seg *segs, int64_t n_segs) {
    return glide_segs_fault_in(segs, n_segs, kWarpMinStep, kWarpMaxStep, kGlideMaxSpan);
}

// the records of a folded plan ("pitch at an output rate", below): the same checks within the wider limits
inline std::string warp_rate_segs_fault(const vits_warp_seg *segs, int64_t n_segs) {
    return warp_segs_fault_in(segs, n_segs, kWarpOne / 8, kWarpOne * 8, 151);
}
inline std::string glide_rate_segs_fault(const vits_glide_seg *segs, int64_t n_segs) {
    return glide_segs_fault_in(segs, n_segs, kWarpOne / 8, kWarpOne * 8, int64_t(1) << 22);
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

// ready_b(X): how many n < N have (pos_n >> FB) + half < X - every input a tile stages for them exists; half is the plan's
// largest Kh bound: kWarpMaxHalf, or what a folded plan ("pitch at an output rate") counts with.  Positions never decrease
// along a row, so it is a prefix count: bisection over n.
template <class Seg>
inline int64_t warp_ready(const Seg *segs, int64_t n_segs, int64_t N, int64_t X, int64_t half = kWarpMaxHalf) {
    int64_t lo = 0, hi = N;  // samples [0, lo) are ready, sample hi (if any) is not
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((warp_row_pos(segs, n_segs, mid) >> kWarpFB) + half < X) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ... and what the row admits: a row whose n_in valid inputs all exist (X >= n_in) is complete - N
template <class Seg>
inline int64_t warp_emit_row(const Seg *segs, int64_t n_segs, int64_t n_in, int64_t N, int64_t X, int64_t half = kWarpMaxHalf) {
    return X >= n_in ? N : warp_ready(segs, n_segs, N, X, half);
}

// e(X) of a launch's rows: the least ready count among the rows still short of input; S_w without one, or on the last piece
template <class Seg>
inline int64_t warp_emit_end(const Seg *segs, const std::vector<WarpRow> &rows, int64_t S_w, int64_t X, bool is_last, int64_t half = kWarpMaxHalf) {
    int64_t e = S_w;
    if (is_last) return e;
    for (const WarpRow &r : rows) {
        if (X >= r.n_in) continue;
        const int64_t q = warp_ready(segs + r.seg0, r.n_segs, r.n_out, X, half);
        e = q < e ? q : e;
    }
    return e;
}

// the largest Kh and the least step a plan's emit rule and cap count with: an unfolded plan's are the family's
template <class Seg>
inline void warp_plan_extent(const Seg *, const std::vector<WarpRow> &, int64_t &half, int64_t &min_step) {
    half = kWarpMaxHalf;
    min_step = kWarpMinStep;
}

// n_cap: output samples one delivery of a streamed run holds at most.  A piece of `piece_in` input samples moves every position's
// bound by that much, which at the least step ONE / 2 completes 2 * piece_in outputs, and the uniform kWarpMaxHalf of the rule may
// fall on either side of it: 2 * (piece_in + kWarpMaxHalf).  Longer ranges - a slow row's end releasing the others - are cut.
// A folded plan counts with its own least step and largest Kh: ceil((piece_in + half) * ONE / min_step) - the same figure at
// ONE / 2 and kWarpMaxHalf.
inline int64_t warp_stream_cap(int64_t piece_in, int64_t S_w, int64_t min_step = kWarpMinStep, int64_t half = kWarpMaxHalf) {
    const int64_t cap = ((piece_in + half) * kWarpOne + min_step - 1) / min_step;
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

// ---- pitch at an output rate (include/vitsmi.h, "pitch at an output rate"): the output rate fo = fi * L / M folded into the step
//
// A token at st semitones delivered at fo is the record with step = 2^(st / 12) * M / L: one filter pass, and n0 / k / N_b are
// delivered samples.  P stays a native input position, so the row plans above serve unchanged given the steps.  Admitted:
// 1/4 <= M / L <= 4, hence steps within [ONE / 8, 8 ONE] and Kh <= 151 (c = 6963 at 8 ONE: ceil(16 * 65536 / 6963)).

constexpr int64_t kWarpRateMinStep = kWarpOne / 8, kWarpRateMaxStep = kWarpOne * 8;
constexpr int kWarpRateMaxHalf = 151;
// Output samples a gliding token of a folded plan has at most.  glide_pos's numerator is |b - a| * j * (j - 1) with j <= k:
// |b - a| <= 8 ONE - ONE / 8 < 2^19, and k <= 2^22 gives j * (j - 1) < 2^44, so the product stays below 2^63 - inside uint64 and,
// divided by 2k, inside int64.  At kGlideMaxSpan = 2^23 it would reach 2^65.  glide_step's numerator |b - a| * j is below 2^41.
constexpr int64_t kGlideRateMaxSpan = int64_t(1) << 22;

// the ratio a pitched row admits
inline bool warp_rate_ok(int64_t L, int64_t M) { return L >= 1 && M >= 1 && M <= 4 * L && L <= 4 * M; }

// warp_token with the rate folded in: step = llrint(2^(st / 12) * M / L * ONE), c and Kh from the step by warp_token's rule
inline bool warp_token_rate(float semitones, int64_t L, int64_t M, int64_t &step, int64_t &c, int32_t &Kh) {
    if (!std::isfinite(semitones) || std::fabs(semitones) > kWarpMaxSemitones) return false;
    const double r = std::exp2((double)semitones / 12.0) * (double)M / (double)L;
    step = std::llrint(r * (double)kWarpOne);
    const double q = (double)kWarpOne / (double)step;
    const double s = kResampleRolloff * (q < 1.0 ? q : 1.0);
    c = std::llrint(s * (double)kWarpOne);
    Kh = (int32_t)(((int64_t)kWarpZ * kWarpOne + c - 1) / c);
    return true;
}

// glide_token with the rate folded into both steps; the factor under compensate is glide_token's - durations are native frames
inline bool glide_token_rate(float st0, float st1, int64_t L, int64_t M, int64_t &a, int64_t &b, float &rate, int *bad = nullptr) {
    int64_t c;
    int32_t Kh;
    if (!warp_token_rate(st0, L, M, a, c, Kh)) {
        if (bad) *bad = 0;
        return false;
    }
    if (!warp_token_rate(st1, L, M, b, c, Kh)) {
        if (bad) *bad = 1;
        return false;
    }
    rate = (float)((std::exp2((double)st0 / 12.0) + std::exp2((double)st1 / 12.0)) * 0.5);
    return true;
}

// warp_plan / glide_plan of a row delivered at fi * L / M (L == M: the plans above, record by record)
inline std::string warp_plan_rate(const int64_t *durations, const float *semitones, int len, int hop, int64_t L, int64_t M, vits_warp_seg *segs,
                                  int64_t *spans, int64_t &n_segs, int64_t &n_out) {
    if (!warp_rate_ok(L, M)) return "rate ratio " + std::to_string(L) + " / " + std::to_string(M) + " outside [1/4, 4]";
    return warp_plan_as([L, M](float st, int64_t &step, int64_t &c, int32_t &Kh) { return warp_token_rate(st, L, M, step, c, Kh); }, durations,
                        semitones, len, hop, segs, spans, n_segs, n_out);
}
inline std::string glide_plan_rate(const int64_t *durations, const float *st0, const float *st1, int len, int hop, int64_t L, int64_t M,
                                   vits_glide_seg *segs, int64_t *spans, int64_t &n_segs, int64_t &n_out) {
    if (!warp_rate_ok(L, M)) return "rate ratio " + std::to_string(L) + " / " + std::to_string(M) + " outside [1/4, 4]";
    return glide_plan_as([L, M](float v0, float v1, int64_t &a, int64_t &b, float &rate, int *bad) { return glide_token_rate(v0, v1, L, M, a, b, rate, bad); },
                         kGlideRateMaxSpan, durations, st0, st1, len, hop, segs, spans, n_segs, n_out);
}

// every token of the row (of the `len` it has) at 0 semitones, both ends: the row is NOT rendered by the folded plan
inline bool warp_rate_unpitched(const float *st0, const float *st1, int len) {
    for (int t = 0; t < len; t++)
        if ((st0 && st0[t] != 0.f) || (st1 ? st1[t] != 0.f : false)) return false;
    return true;
}

// ... but by the resampler's rule, so that an unpitched request does not change because it was batched with a pitched one:
// N = ceil(n_in * L / M), token t's span the difference of ceil(cum_t * hop * L / M) clamped to N.  spans nullable.
inline int64_t warp_rate_identity(const int64_t *durations, int len, int hop, int64_t L, int64_t M, int64_t n_in, int64_t *spans) {
    const int64_t N = (n_in * L + M - 1) / M;
    int64_t cum = 0, prev = 0;
    for (int t = 0; t < len && spans; t++) {
        cum += durations[t] > 0 ? durations[t] : 0;
        int64_t e = (cum * hop * L + M - 1) / M;
        e = e > N ? N : e;
        spans[t] = e - prev;
        prev = e;
    }
    return N;
}

// A row of a folded launch: WarpRow, the largest Kh among its samples (what a tile stages on either side) and the resampler's
// plan of the row, as ResampleRowPlan has it - what an identity row is rendered by (table == nullptr: a masked copy, L == M).
struct WarpRateRow {
    int32_t seg0, n_segs;
    int32_t n_in, n_out;
    int32_t identity;
    int32_t half_max;
    int32_t Kp, K;
    int64_t L, M;
    const float *table;
};

// the largest Kh and the least step among a row's records (no record: 1 and kWarpRateMaxStep)
inline void warp_rate_extent(const vits_warp_seg *segs, int64_t n_segs, int32_t &half, int64_t &min_step) {
    half = 1;
    min_step = kWarpRateMaxStep;
    for (int64_t j = 0; j < n_segs; j++) {
        half = segs[j].half_taps > half ? segs[j].half_taps : half;
        min_step = segs[j].step < min_step ? segs[j].step : min_step;
    }
}
inline void warp_rate_extent(const vits_glide_seg *segs, int64_t n_segs, int32_t &half, int64_t &min_step) {
    half = 1;
    min_step = kWarpRateMaxStep;
    for (int64_t j = 0; j < n_segs; j++) {
        int32_t c, Kh;
        glide_cutoff(segs[j].step0 > segs[j].step1 ? segs[j].step0 : segs[j].step1, c, Kh);  // (Kh grows with the step)
        half = Kh > half ? Kh : half;
        const int64_t lo = segs[j].step0 < segs[j].step1 ? segs[j].step0 : segs[j].step1;
        min_step = lo < min_step ? lo : min_step;
    }
}

// The rows' records of a folded launch.  A row without a segment is an identity row: N_b = ceil(n_b * L_b / M_b), rendered by
// plan[b] (whose table the caller fills in); every other row is rendered by its records, even at unit steps.  Returns S_w.
template <class Seg>
inline int64_t warp_rate_rows(const Seg *segs, const int32_t *seg_first, const int64_t *n_in, const int64_t *L, const int64_t *M, int B,
                              std::vector<WarpRateRow> &rows) {
    rows.resize((size_t)B);
    int64_t S_w = 1;
    for (int b = 0; b < B; b++) {
        const int32_t s0 = seg_first[b], ns = seg_first[b + 1] - s0;
        const int64_t N = ns > 0 ? segs[s0 + ns - 1].n0 + segs[s0 + ns - 1].k : (n_in[b] * L[b] + M[b] - 1) / M[b];
        int32_t half = 1;
        int64_t lo = 0;
        warp_rate_extent(segs + s0, ns, half, lo);
        rows[(size_t)b] = WarpRateRow{s0, ns, (int32_t)n_in[b], (int32_t)N, ns > 0 ? 0 : 1, half, 0, 0, L[b], M[b], nullptr};
        S_w = N > S_w ? N : S_w;
    }
    return S_w;
}

// Streams of a folded plan.  The emit rule counts with the plan's largest Kh (`half`) in place of kWarpMaxHalf, the cap with
// its least step in place of ONE / 2; an identity row is the resampler's and is ready by the resampler's own rule. An identity
// row advances by M / L input samples an output: its step, rounded down, joins the least.  (A native identity row - a masked
// copy - has K == 0: sample n is ready once input n exists.)
template <class Seg>
inline void warp_plan_extent(const Seg *segs, const std::vector<WarpRateRow> &rows, int64_t &half, int64_t &min_step) {
    half = 1;
    min_step = kWarpRateMaxStep;
    for (const WarpRateRow &r : rows) {
        int32_t h = 1;
        int64_t s = r.M * kWarpOne / r.L;
        if (!r.identity) warp_rate_extent(segs + r.seg0, r.n_segs, h, s);
        half = h > half ? h : half;
        min_step = s < min_step ? s : min_step;
    }
}

// ready count of an identity row once input samples [0, X) exist: ResamplePlan::complete, clipped to the row
inline int64_t warp_rate_identity_ready(const WarpRateRow &r, int64_t X) {
    ResamplePlan p;
    p.L = r.L;
    p.M = r.M;
    p.K = r.K;
    const int64_t q = p.complete(X);
    return q < r.n_out ? q : (int64_t)r.n_out;
}

// warp_emit_end over the rows of a folded plan
template <class Seg>
inline int64_t warp_emit_end(const Seg *segs, const std::vector<WarpRateRow> &rows, int64_t S_w, int64_t X, bool is_last, int64_t half) {
    int64_t e = S_w;
    if (is_last) return e;
    for (const WarpRateRow &r : rows) {
        if (X >= r.n_in) continue;
        const int64_t q = r.identity ? warp_rate_identity_ready(r, X) : warp_ready(segs + r.seg0, r.n_segs, r.n_out, X, half);
        e = q < e ? q : e;
    }
    return e;
}

}  // namespace vitsmi
