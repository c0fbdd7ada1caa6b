// shape.hpp — the plan of a shaped delivery (include/vitsmi.h, "shaped delivery"): the validation of shapes and breakpoints,
// the slope table and the scalar rule of one sample's multiplier, and what the shaped pack kernel reads: a record per segment
// and the envelope as knots.
// Host-side C++17, no HIP types, answered without a handle or a device - like delivery.hpp.
//
// The arithmetic of the rule is stated ONCE, in the functions marked SHAPE_FN below: under a HIP compiler they are host and
// device functions, and the kernel (shape.hip.hpp) calls the very same ones.  Every product, sum, difference and quotient of
// the definition is a rounding of its own, so each lives in a function compiled with contraction switched off (shape_mul
// ...).  HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators in its headers and do NOT do that: the compiler
// contracts __fadd_rn(g, __fmul_rn(s, t)) into one v_fmac_f32 (seen in the ISA of a probe kernel for gfx950), which rounds
// once instead of twice.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"

#if defined(__HIPCC__)
#define SHAPE_FN __host__ __device__ inline
#else
#define SHAPE_FN inline
#endif
// contraction off for the body that follows (clang: a pragma at the head of the body; GCC: an attribute of the function)
#if defined(__clang__)
#define SHAPE_EXACT
#define SHAPE_EXACT_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define SHAPE_EXACT __attribute__((optimize("fp-contract=off")))
#define SHAPE_EXACT_BODY
#else
#define SHAPE_EXACT
#define SHAPE_EXACT_BODY
#endif

namespace vitsmi {

constexpr int64_t kShapeMaxPoints = (int64_t)1 << 20;  // breakpoints of one call
constexpr float kShapeMinGain = 9.5367431640625e-07f;  // 2^-20: the smallest gain that is not 0
constexpr float kShapeMaxGain = 64.0f;

// one rounded fp32 operation each
SHAPE_EXACT SHAPE_FN float shape_mul(float x, float y) {
    SHAPE_EXACT_BODY
    return x * y;
}
SHAPE_EXACT SHAPE_FN float shape_add(float x, float y) {
    SHAPE_EXACT_BODY
    return x + y;
}
SHAPE_EXACT SHAPE_FN float shape_sub(float x, float y) {
    SHAPE_EXACT_BODY
    return x - y;
}
SHAPE_EXACT SHAPE_FN float shape_div(float x, float y) {
    SHAPE_EXACT_BODY
    return x / y;
}

// one segment as the shaped pack kernel reads it (32 bytes; parallel to the DeliverySeg table, in dst order)
struct ShapeSeg {
    int32_t a;         // first kept sample of the row (row sample i = a + j)
    int32_t c;         // kept samples (DeliverySeg::n)
    int32_t fade_in, fade_out;
    int32_t curve;
    int32_t n_points;
    int64_t first;  // the scalar rule: index of the segment's first point and slope in the call's tables; the kernel: of its
                    // first knot
};

// The envelope as the kernel reads it: one 16-byte record per INTERVAL, so that a sample whose interval is known needs no
// further load - position, gain and slope of the point the interval starts at, and where the next one starts.  A segment
// with m points has m + 1 knots: knot 0 covers the samples in front of p_0 (gain g_0, slope 0), knot k + 1 the samples from
// p_k on (g_k, s_k), the last one has slope 0 and no successor (next = INT_MAX, which no row sample reaches).  With them
// e = g + s * (float)(i - pos) is the definition's value in every case: 0 * d is 0 for every d >= 0 and g + 0 is g, which
// are the three cases the definition states apart (i <= p_0, i >= p_{m-1}, m == 0: one knot of gain 1).
struct alignas(16) ShapeKnot {
    int32_t pos;
    float gain, slope;
    int32_t next;
};

// curve(t): 0 linear, 1 smooth - (t * t) * (3 - 2 t), four roundings
SHAPE_FN float shape_curve(float t, int curve) {
    if (curve == 0) return t;
    return shape_mul(shape_mul(t, t), shape_sub(3.0f, shape_mul(2.0f, t)));
}

// the fade weights of kept sample j of c
SHAPE_FN float shape_w_in(int32_t j, int32_t fade_in, int curve) {
    if (fade_in == 0 || j >= fade_in) return 1.0f;
    return shape_curve(shape_div((float)j, (float)fade_in), curve);
}
SHAPE_FN float shape_w_out(int32_t j, int32_t c, int32_t fade_out, int curve) {
    const int32_t r = c - 1 - j;
    if (fade_out == 0 || r >= fade_out) return 1.0f;
    return shape_curve(shape_div((float)r, (float)fade_out), curve);
}

// the largest k with p[k].pos <= i, -1 when i lies in front of every point (m >= 0)
SHAPE_FN int shape_locate(const vits_env_point *p, int m, int32_t i) {
    int lo = -1, hi = m;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p[mid].pos <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the envelope at row sample i, with k = shape_locate(p, m, i); s: the slopes of the same points
SHAPE_FN float shape_env(const vits_env_point *p, const float *s, int m, int k, int32_t i) {
    if (m == 0) return 1.0f;
    if (k < 0 || i <= p[0].pos) return p[0].gain;
    if (k >= m - 1) return p[m - 1].gain;
    return shape_add(p[k].gain, shape_mul(s[k], (float)(i - p[k].pos)));
}

// the largest r in [0, m] with r == 0 or knots[r].pos <= i: the knot of row sample i among a segment's m + 1
SHAPE_FN int shape_knot_locate(const ShapeKnot *knots, int m, int32_t i) {
    int lo = 0, hi = m + 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (knots[mid].pos <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the envelope at row sample i, k its knot
SHAPE_FN float shape_knot_env(const ShapeKnot &k, int32_t i) { return shape_add(k.gain, shape_mul(k.slope, (float)(i - k.pos))); }

// mul = (e * w_in) * w_out
SHAPE_FN float shape_combine(float e, float w_in, float w_out) { return shape_mul(shape_mul(e, w_in), w_out); }

// a shape without fades and points: its multiplier is 1 everywhere
inline bool shape_trivial(const vits_shape &s) { return s.fade_in == 0 && s.fade_out == 0 && s.n_points == 0; }
inline bool any_shape(const vits_shape *shapes, int n_segs) {
    for (int g = 0; g < n_segs && shapes; g++)
        if (!shape_trivial(shapes[g])) return true;
    return false;
}

// "" or what is wrong with the shapes of a call, naming the segment and the value.  shapes == nullptr: "".
inline std::string shape_fault(const vits_shape *shapes, int n_segs, const vits_env_point *points, int64_t n_points) {
    if (!shapes) return "";
    char buf[240];
    if (n_points < 0 || n_points > kShapeMaxPoints) {
        std::snprintf(buf, sizeof buf, "n_points = %lld outside [0, %lld]", (long long)n_points, (long long)kShapeMaxPoints);
        return buf;
    }
    if (n_points > 0 && !points) return "points is null";
    for (int g = 0; g < n_segs; g++) {
        const vits_shape &s = shapes[g];
        buf[0] = 0;
        if (s.fade_in < 0) std::snprintf(buf, sizeof buf, "segment %d: fade_in %d is negative", g, s.fade_in);
        else if (s.fade_out < 0) std::snprintf(buf, sizeof buf, "segment %d: fade_out %d is negative", g, s.fade_out);
        else if (s.curve < 0 || s.curve > 1) std::snprintf(buf, sizeof buf, "segment %d: curve %d outside 0..1", g, s.curve);
        else if (s.n_points < 0) std::snprintf(buf, sizeof buf, "segment %d: n_points %d is negative", g, s.n_points);
        else if (s.first_point < 0 || s.first_point > n_points - s.n_points)
            std::snprintf(buf, sizeof buf, "segment %d: points [%lld, +%d) outside the call's %lld points", g, (long long)s.first_point,
                          s.n_points, (long long)n_points);
        if (buf[0]) return buf;
        for (int k = 0; k < s.n_points; k++) {
            const vits_env_point &p = points[s.first_point + k];
            if (p.pos < 0) std::snprintf(buf, sizeof buf, "segment %d: point %d: pos %d outside [0, %d]", g, k, p.pos, INT_MAX);
            else if (k > 0 && p.pos <= points[s.first_point + k - 1].pos)
                std::snprintf(buf, sizeof buf, "segment %d: point %d: pos %d does not ascend (point %d: pos %d)", g, k, p.pos, k - 1,
                              points[s.first_point + k - 1].pos);
            else if (!std::isfinite(p.gain) || p.gain < 0.f || (p.gain > 0.f && p.gain < kShapeMinGain) || p.gain > kShapeMaxGain)
                std::snprintf(buf, sizeof buf, "segment %d: point %d: gain %g is not 0 or within [2^-20, 64]", g, k, (double)p.gain);
            if (buf[0]) return buf;
        }
    }
    return "";
}

// the slope behind every point of the call: s[k] = (g[k+1] - g[k]) / (float)(p[k+1] - p[k]) where the positions ascend (a
// segment's intervals), 0 elsewhere (the last point of a segment, whose slope is never read).  One table for the call: a
// slope depends on its two points alone, so segments whose point ranges overlap read the same values.
inline void shape_slopes(const vits_env_point *points, int64_t n_points, std::vector<float> &slopes) {
    slopes.assign((size_t)n_points, 0.f);
    for (int64_t k = 0; k + 1 < n_points; k++) {
        const int64_t dp = (int64_t)points[k + 1].pos - points[k].pos;
        if (dp > 0) slopes[k] = shape_div(shape_sub(points[k + 1].gain, points[k].gain), (float)dp);
    }
}

// the records of a plan's segments, in the plan's (dst) order: order[k] is the caller's segment, first_kept / kept_count [k]
// its kept range.  shapes must have passed shape_fault.
inline void shape_table(const vits_shape *shapes, const std::vector<int> &order, const int64_t *first_kept, const int64_t *kept_count,
                        std::vector<ShapeSeg> &table) {
    table.resize(order.size());
    for (size_t k = 0; k < order.size(); k++) {
        const vits_shape &s = shapes[order[k]];
        table[k] = ShapeSeg{(int32_t)first_kept[k], (int32_t)kept_count[k], s.fade_in, s.fade_out, s.curve, s.n_points, s.first_point};
    }
}

// the knots a call's shapes need: a segment's points and one more
inline int64_t shape_knot_count(const vits_shape *shapes, int n_segs) {
    int64_t n = 0;
    for (int g = 0; g < n_segs && shapes; g++) n += (int64_t)shapes[g].n_points + 1;
    return n;
}

// the knots of the segments of `table` (shape_table's), segment by segment in its order; every record's `first` becomes the
// index of its segment's first knot
inline void shape_knots(std::vector<ShapeSeg> &table, const vits_env_point *points, std::vector<ShapeKnot> &knots) {
    knots.clear();
    for (ShapeSeg &t : table) {
        const vits_env_point *p = points + t.first;
        const int m = t.n_points;
        t.first = (int64_t)knots.size();
        if (m == 0) {
            knots.push_back(ShapeKnot{0, 1.0f, 0.f, INT_MAX});
            continue;
        }
        knots.push_back(ShapeKnot{0, p[0].gain, 0.f, p[0].pos});
        for (int k = 0; k < m; k++) {
            const bool last = k + 1 == m;
            const float slope = last ? 0.f : shape_div(shape_sub(p[k + 1].gain, p[k].gain), (float)(p[k + 1].pos - p[k].pos));
            knots.push_back(ShapeKnot{p[k].pos, p[k].gain, slope, last ? INT_MAX : p[k + 1].pos});
        }
    }
}

// the multiplier of row sample i as the kernel computes it: t and knots from shape_knots
inline float shape_gain_knots(const ShapeSeg &t, const ShapeKnot *knots, int32_t i) {
    const ShapeKnot *kn = knots + t.first;
    const float e = shape_knot_env(kn[shape_knot_locate(kn, t.n_points, i)], i);
    const int32_t j = i - t.a;
    return shape_combine(e, shape_w_in(j, t.fade_in, t.curve), shape_w_out(j, t.c, t.fade_out, t.curve));
}

// the multiplier of row sample i = t.a + j, j in [0, t.c): the scalar rule
inline float shape_gain(const ShapeSeg &t, const vits_env_point *points, const float *slopes, int32_t i) {
    const vits_env_point *p = points + t.first;
    const int k = shape_locate(p, t.n_points, i);
    const float e = shape_env(p, slopes + t.first, t.n_points, k, i);
    const int32_t j = i - t.a;
    return shape_combine(e, shape_w_in(j, t.fade_in, t.curve), shape_w_out(j, t.c, t.fade_out, t.curve));
}

}  // namespace vitsmi
