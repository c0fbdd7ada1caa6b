// fit.hpp — fitted durations (include/vitsmi.h, "fitted durations"): the cleaning of a weight, a token's frames at a
// multiplier, the search for the multiplier s* and the plan of one group.  Host-side C++17, no HIP types; the pieces the
// kernel shares (fit.hip.hpp) are VITSMI_HD, so the arithmetic is stated once.  Everything behind the fp32 weight is IEEE
// double and integers: host, device and a NumPy restatement agree on every bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"

#ifndef VITSMI_HD
#if defined(__HIPCC__)
#define VITSMI_HD __host__ __device__
#else
#define VITSMI_HD
#endif
#endif

namespace vitsmi {

// S = the doubles of [2^-4, 2^4]; positive doubles order like their bit patterns, so the search walks the patterns
constexpr uint64_t kFitLoBits = 0x3FB0000000000000ull;   // 2^-4
constexpr uint64_t kFitOneBits = 0x3FF0000000000000ull;  // 1.0
constexpr uint64_t kFitHiBits = 0x4030000000000000ull;   // 2^4
constexpr float kFitMaxWeight = 16777216.f;              // 2^24

// what the device leaves per group in the readback block
struct FitResult {
    double scale;
    int64_t frames;
    int32_t status;
    int32_t pad_;
};
static_assert(sizeof(FitResult) == 24, "FitResult is a 24-byte record");

// floats of the readback block [w_ceil B*T | y_len B | fit]: the records sit at the next 8-byte boundary, one per row at most
// (no group is empty, so there are never more groups than rows)
inline size_t fit_block_offset(size_t nBT, int B) { return (nBT + (size_t)B + 1) & ~size_t(1); }
inline size_t fit_block_floats(size_t nBT, int B, int G) { return fit_block_offset(nBT, B) + (size_t)G * (sizeof(FitResult) / sizeof(float)); }

// the cleaned weight: not finite or not > 0 counts as 0, above 2^24 as 2^24
VITSMI_HD inline float fit_clean(float w) {
    if (!(w > 0.f) || !(w <= 3.402823466e+38f)) return 0.f;
    return w > kFitMaxWeight ? kFitMaxWeight : w;
}

VITSMI_HD inline double fit_scale(uint64_t bits) {
    double s;
    __builtin_memcpy(&s, &bits, sizeof s);
    return s;
}

// a token's frames at multiplier s: one double product (nothing to fuse it with), ceil, int64.  With w <= 2^24 and s <= 2^4
// (fit_scale(bits + 1) of 2^4 included) the value is at most 2^28 + 1, so the conversion goes through int - one instruction
// on the device where double -> int64 is a sequence - and gives the same integer.
VITSMI_HD inline int64_t fit_term(float w_clean, double s) { return (int64_t)(int32_t)ceil((double)w_clean * s); }

// The search.  count(bits) is the group's frame count at the multiplier with that bit pattern, non-decreasing in it; on the
// device every thread of the workgroup calls it with the same argument and receives the same value, so the control flow
// here is uniform.  Leaves s* (as bits), count(s*) and the status; a bisection over the patterns, 55 counts at the most.
template <class Count>
VITSMI_HD inline void fit_search(Count &count, int64_t F, int mode, uint64_t &bits, int64_t &cnt, int32_t &status) {
    uint64_t hi = kFitHiBits;
    if (mode == 2) {
        const int64_t c1 = count(kFitOneBits);
        if (c1 <= F) {
            bits = kFitOneBits, cnt = c1, status = VITS_FIT_KEPT;
            return;
        }
        hi = kFitOneBits;  // count(1.0) > F: s* lies below
    }
    uint64_t lo = kFitLoBits;
    int64_t clo = count(lo);
    if (clo > F) {
        bits = lo, cnt = clo, status = VITS_FIT_FLOOR;
        return;
    }
    if (mode != 2) {
        const int64_t chi = count(hi);
        if (chi <= F) {
            bits = hi, cnt = chi, status = chi < F ? VITS_FIT_CEIL : VITS_FIT_MET;
            return;
        }
    }
    while (hi - lo > 1) {  // count(lo) <= F < count(hi)
        const uint64_t mid = lo + (hi - lo) / 2;
        const int64_t cm = count(mid);
        if (cm <= F) lo = mid, clo = cm;
        else hi = mid;
    }
    bits = lo, cnt = clo, status = VITS_FIT_MET;
}

// a vits_fit against a batch of B rows: "" or the refusal.  max_frames: what a group's target admits.
inline std::string fit_fault(const vits_fit *fit, int B, int64_t max_frames) {
    char m[200];
    if (!fit) return "";
    const int G = fit->n_groups;
    if (G < 0) {
        std::snprintf(m, sizeof m, "fit n_groups = %d is negative", G);
        return m;
    }
    if (G > 0 && (!fit->group || !fit->target_frames || !fit->mode)) return "fit with groups needs group, target_frames and mode";
    std::vector<int> rows((size_t)G, 0);
    for (int b = 0; b < B && fit->group; b++) {
        const int32_t g = fit->group[b];
        if (g < -1 || g >= G) {
            std::snprintf(m, sizeof m, "fit group[%d]=%d outside [-1,%d)", b, (int)g, G);
            return m;
        }
        if (g >= 0) rows[g]++;
    }
    for (int g = 0; g < G; g++) {
        const int64_t F = fit->target_frames[g];
        if (F < 1 || F > max_frames) {
            std::snprintf(m, sizeof m, "fit target_frames[%d]=%lld outside [1,%lld] (VITS_MAX_FORCED_FRAMES, INT_MAX / hop)", g, (long long)F,
                          (long long)max_frames);
            return m;
        }
        if (fit->mode[g] != 1 && fit->mode[g] != 2) {
            std::snprintf(m, sizeof m, "fit mode[%d]=%d is neither 1 (exact) nor 2 (at most)", g, (int)fit->mode[g]);
            return m;
        }
        if (rows[g] == 0) {
            std::snprintf(m, sizeof m, "fit group %d has no rows", g);
            return m;
        }
    }
    return "";
}

// some row belongs to a group: otherwise the call is the entry without a fit
inline bool fit_on(const vits_fit *fit, int B) {
    if (!fit || fit->n_groups <= 0 || !fit->group) return false;
    for (int b = 0; b < B; b++)
        if (fit->group[b] >= 0) return true;
    return false;
}

// The plan of group g over weights [B][T] (rows b with group[b] == g, tokens t < lens[b]): durations [B][T] of its rows
// (0 behind lens[b]; other rows are not written), s*, the achieved frames and the status.
inline void fit_plan_group(const float *w, const int64_t *lens, const int32_t *group, int B, int T, int g, int64_t F, int mode,
                           int64_t *dur, double &scale, int64_t &frames, int32_t &status) {
    std::vector<float> wc;
    std::vector<size_t> at;
    for (int b = 0; b < B; b++) {
        if (group[b] != g) continue;
        for (int t = 0; t < T; t++) dur[(size_t)b * T + t] = 0;
        for (int t = 0; t < (int)lens[b]; t++) {
            wc.push_back(fit_clean(w[(size_t)b * T + t]));
            at.push_back((size_t)b * T + t);
        }
    }
    auto count = [&](uint64_t bits) {
        const double s = fit_scale(bits);
        int64_t c = 0;
        for (float v : wc) c += fit_term(v, s);
        return c;
    };
    uint64_t bits;
    int64_t cnt;
    fit_search(count, F, mode, bits, cnt, status);
    const double s = fit_scale(bits), s_next = fit_scale(bits + 1);
    int64_t R = status == VITS_FIT_MET ? F - cnt : 0;
    frames = 0;
    for (size_t i = 0; i < wc.size(); i++) {  // (b, t) ascending: the first R candidates take one more frame
        int64_t d = fit_term(wc[i], s);
        if (R > 0 && fit_term(wc[i], s_next) > d) d++, R--;
        dur[at[i]] = d;
        frames += d;
    }
    scale = s;
}

}  // namespace vitsmi
