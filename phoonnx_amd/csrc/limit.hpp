// limit.hpp — the plan of a limited delivery (include/vitsmi.h, "limited delivery"): the validation of the limits, the scalar
// rule of one segment's gains, and what the limiter's kernels read: a record per segment.
// Host-side C++17, no HIP types, answered without a handle or a device - like shape.hpp.
//
// Everything in front of the final division is integer arithmetic, so the order in which a parallel scheme forms the
// minima and the sums cannot show.  The three floating-point operations of the rule - the quotient ceiling / |u|, its product
// with 2^16, and S / ((L + 1) * 2^16) - are shape.hpp's contraction-off shape_div / shape_mul: under a HIP compiler limit_q
// and limit_g are host and device functions, and the kernels (limit.hip.hpp) call the very same ones.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"
#include "shape.hpp"

namespace vitsmi {

constexpr int32_t kLimitUnity = 65536;     // q of a sample that needs no gain reduction: 2^16
constexpr float kLimitMaxVolume = 1024.f;  // |volume| of a limited segment

// one segment as the limiter's kernels read it (16 bytes; parallel to the DeliverySeg table, in dst order)
struct LimitSeg {
    float ceiling;
    int32_t L;   // the look-ahead in samples
    int32_t on;  // 0: the segment is not limited (g = 1.0f, no clamp)
    int32_t pad;
};

// q: the gain sample value u would need on its own, in units of 2^-16.  (A NaN is not above the ceiling: 65536.)
SHAPE_FN int32_t limit_q(float u, float ceiling) {
    const float m = fabsf(u);
    if (!(m > ceiling)) return kLimitUnity;
    return (int32_t)floorf(shape_mul(shape_div(ceiling, m), 65536.0f));
}

// g of a window sum S over a box of L + 1
SHAPE_FN float limit_g(int32_t S, int32_t L) { return shape_div((float)S, (float)((L + 1) * kLimitUnity)); }

// the limited sample: one rounded product, then the clamp that absorbs its rounding
SHAPE_FN float limit_apply(float u, float g, float ceiling) { return fminf(fmaxf(shape_mul(u, g), -ceiling), ceiling); }

inline bool any_limit(const vits_limit *limits, int n_segs) {
    for (int g = 0; g < n_segs && limits; g++)
        if (limits[g].mode != 0) return true;
    return false;
}

// "" or what is wrong with the limits of a call, naming the segment and the value.  limits == nullptr: "".  Ceiling and
// lookahead are read of a limited segment only (mode 1): an all-zero vits_limit is "off".  segs (nullable): the volume of
// a limited segment is checked where they are given.
inline std::string limit_fault(const vits_limit *limits, const vits_segment *segs, int n_segs) {
    if (!limits) return "";
    char buf[200];
    for (int g = 0; g < n_segs; g++) {
        const vits_limit &l = limits[g];
        buf[0] = 0;
        if (l.mode < 0 || l.mode > 1) std::snprintf(buf, sizeof buf, "segment %d: limit mode %d outside 0..1", g, l.mode);
        else if (l.reserved != 0) std::snprintf(buf, sizeof buf, "segment %d: limit reserved %d is not 0", g, l.reserved);
        else if (l.mode == 1 && !(std::isfinite(l.ceiling) && l.ceiling > 0.f && l.ceiling <= 1.f))
            std::snprintf(buf, sizeof buf, "segment %d: limit ceiling %g is not finite and within (0, 1]", g, (double)l.ceiling);
        else if (l.mode == 1 && (l.lookahead < 1 || l.lookahead > VITS_LIMIT_MAX_LOOKAHEAD))
            std::snprintf(buf, sizeof buf, "segment %d: lookahead %d outside [1, %d]", g, l.lookahead, VITS_LIMIT_MAX_LOOKAHEAD);
        else if (l.mode == 1 && segs && !(fabsf(segs[g].volume) <= kLimitMaxVolume))
            std::snprintf(buf, sizeof buf, "segment %d: volume %g of a limited segment: |volume| is at most %g", g, (double)segs[g].volume,
                          (double)kLimitMaxVolume);
        if (buf[0]) return buf;
    }
    return "";
}

// The rule for one segment, written for clarity: u [c] the unlimited values of the kept range, g [c] the gains.
//   q[k] = limit_q(u[k]) inside [0, c), 65536 outside;  M[j] = min q[j .. j + L], j in [-L, c);  S[j] = M[j - L] + .. + M[j]
inline void limit_gains(const float *u, int64_t c, float ceiling, int32_t L, float *g) {
    auto q = [&](int64_t k) { return k < 0 || k >= c ? kLimitUnity : limit_q(u[k], ceiling); };
    std::vector<int32_t> M((size_t)(c + L));  // M[j] at index j + L
    for (int64_t j = -L; j < c; j++) {
        int32_t m = kLimitUnity;
        for (int64_t k = j; k <= j + L; k++) m = q(k) < m ? q(k) : m;
        M[(size_t)(j + L)] = m;
    }
    for (int64_t j = 0; j < c; j++) {
        int32_t S = 0;
        for (int64_t k = j - L; k <= j; k++) S += M[(size_t)(k + L)];
        g[j] = limit_g(S, L);
    }
}

// the records of a plan's segments, in the plan's (dst) order: order[k] is the caller's segment.  limits must have passed
// limit_fault; nullptr: every record is off.
inline void limit_table(const vits_limit *limits, const std::vector<int> &order, std::vector<LimitSeg> &table) {
    table.assign(order.size(), LimitSeg{1.0f, 1, 0, 0});
    for (size_t k = 0; k < order.size() && limits; k++) {
        const vits_limit &l = limits[order[k]];
        if (l.mode == 1) table[k] = LimitSeg{l.ceiling, l.lookahead, 1, 0};
    }
}

}  // namespace vitsmi
