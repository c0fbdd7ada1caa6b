// stream_shape.hpp — the plan of a shaped, limited encoded stream (include/vitsmi.h, "shaped streaming"): the validation of
// the shaping, the chunk timeline, and what the stream's kernels (stream_shape.hip.hpp) read: a record per row and the
// envelopes as knots.
// Host-side C++17, no HIP types, answered without a handle or a device - like shape.hpp and limit.hpp, whose rules it
// reuses unchanged: a row of the stream is a segment that keeps the whole row, a = 0 and c = n_b.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"
#include "limit.hpp"
#include "shape.hpp"

namespace vitsmi {

// one row as the stream's kernels read it (32 bytes).  c is not here: the kernels read n_b from the device (StreamPackRows)
struct StreamShapeRow {
    int32_t fade_in, fade_out;
    int32_t curve;
    int32_t n_points;
    int32_t first;  // index of the row's first knot
    float ceiling;  // 0: the row is not limited (g = 1, no clamp)
    int32_t pad[2];
};

inline bool stream_shaped(const vits_stream_shaping *s, int B) {
    return s && (s->lookahead != 0 || s->plan || any_shape(s->shapes, B));
}

// "" or what is wrong with the shaping of a call, naming the row and the value.  nullptr: "".  volume (nullable): the volumes
// of the limited rows are checked where they are given.
inline std::string stream_shape_fault(const vits_stream_shaping *s, const float *volume, int B) {
    if (!s) return "";
    std::string e = shape_fault(s->shapes, B, s->points, s->n_points);
    if (!e.empty()) {
        const std::string word = "segment ";  // (a stream's segment IS its row)
        if (e.compare(0, word.size(), word) == 0) e = "row " + e.substr(word.size());
        return e;
    }
    char buf[200];
    if (s->lookahead < 0 || s->lookahead > VITS_LIMIT_MAX_LOOKAHEAD) {
        std::snprintf(buf, sizeof buf, "lookahead %d outside [0, %d]", s->lookahead, VITS_LIMIT_MAX_LOOKAHEAD);
        return buf;
    }
    for (int b = 0; b < B && s->ceiling; b++) {
        const float c = s->ceiling[b];
        buf[0] = 0;
        if (!(std::isfinite(c) && c >= 0.f && c <= 1.f))
            std::snprintf(buf, sizeof buf, "row %d: limit ceiling %g is not 0, or finite and within (0, 1]", b, (double)c);
        else if (c > 0.f && s->lookahead > 0 && volume && !(fabsf(volume[b]) <= kLimitMaxVolume))
            std::snprintf(buf, sizeof buf, "row %d: volume %g of a limited row: |volume| is at most %g", b, (double)volume[b],
                          (double)kLimitMaxVolume);
        if (buf[0]) return buf;
    }
    return "";
}

// The timeline: a rendered piece [first, first + n) of rows of `total` samples delivers [e_first, e_first + e_n) - everything
// whose look-ahead of L samples has been rendered, the last piece the rest.  e_n == 0: the piece completes nothing.
inline void stream_emit_range(int64_t first, int64_t n, bool is_last, int64_t total, int64_t L, int64_t &e_first, int64_t &e_n) {
    e_first = first - L > 0 ? first - L : 0;
    int64_t end = is_last ? total : first + n - L;
    end = end > total ? total : end;
    e_n = end > e_first ? end - e_first : 0;
}

// the records and knots of a call's B rows; the shaping has passed stream_shape_fault (nullptr: every row plain)
inline void stream_shape_table(const vits_stream_shaping *s, int B, std::vector<StreamShapeRow> &rows, std::vector<ShapeKnot> &knots) {
    std::vector<ShapeSeg> table((size_t)B);
    for (int b = 0; b < B; b++) {
        const vits_shape sh = s && s->shapes ? s->shapes[b] : vits_shape{};
        table[b] = ShapeSeg{0, 0, sh.fade_in, sh.fade_out, sh.curve, sh.n_points, sh.first_point};
    }
    shape_knots(table, s ? s->points : nullptr, knots);
    rows.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const float c = s && s->lookahead > 0 && s->ceiling ? s->ceiling[b] : 0.f;
        rows[b] = StreamShapeRow{table[b].fade_in, table[b].fade_out, table[b].curve, table[b].n_points, (int32_t)table[b].first, c, {0, 0}};
    }
}

// the knots a call's B rows need: a row's points and one more
inline int64_t stream_knot_count(const vits_stream_shaping *s, int B) {
    return s && s->shapes ? shape_knot_count(s->shapes, B) : (int64_t)B;
}

// ---- the leading trim of a stream (include/vitsmi.h, "trimmed streaming"): the onsets' validation, the start rule, and what
// the scan (stream_trim.hip.hpp) reads

constexpr int32_t kStreamNoStart = INT32_MAX;  // start[b] of a trimmed row whose onset has not been found

// one row as the scan reads it (16 bytes): thr is the resolved threshold - mode 2's one fp32 product is made on the host
struct StreamOnsetRow {
    int32_t on;  // 0: the row is not trimmed (its start is 0 from the beginning)
    float thr;
    int32_t keep_lead;
    int32_t pad;
};

inline bool stream_trimmed(const vits_stream_onset *o, int B) {
    for (int b = 0; o && b < B; b++)
        if (o[b].mode != 0) return true;
    return false;
}

// "" or what is wrong with the onsets of a call, naming the row and the value.  nullptr: "".
inline std::string stream_onset_fault(const vits_stream_onset *o, const float *ref_peak, int B) {
    char buf[200];
    for (int b = 0; o && b < B; b++) {
        buf[0] = 0;
        if (o[b].mode < 0 || o[b].mode > 2)
            std::snprintf(buf, sizeof buf, "row %d: onset mode %d outside 0..2", b, (int)o[b].mode);
        else if (!(std::isfinite(o[b].threshold) && o[b].threshold >= 0.f))
            std::snprintf(buf, sizeof buf, "row %d: onset threshold %g is not a finite value >= 0", b, (double)o[b].threshold);
        else if (o[b].keep_lead < 0)
            std::snprintf(buf, sizeof buf, "row %d: onset keep_lead %d is negative", b, (int)o[b].keep_lead);
        else if (o[b].reserved != 0)
            std::snprintf(buf, sizeof buf, "row %d: onset reserved %d is not 0", b, (int)o[b].reserved);
        else if (o[b].mode == 2 && !ref_peak)
            std::snprintf(buf, sizeof buf, "row %d: onset mode 2 needs ref_peak", b);
        if (buf[0]) return buf;
    }
    return "";
}

// a_b of a row whose first active sample f lies in a piece that delivers from `delivered_before` on (its e_first)
inline int64_t stream_onset_start(int64_t f, int64_t keep_lead, int64_t delivered_before) {
    const int64_t a = f - keep_lead;
    return a > delivered_before ? a : delivered_before;
}

// the scan's records of a call's B rows; the onsets have passed stream_onset_fault
inline void stream_onset_table(const vits_stream_onset *o, const float *ref_peak, int B, std::vector<StreamOnsetRow> &rows) {
    rows.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        const float thr = o[b].mode == 2 ? o[b].threshold * ref_peak[b] : o[b].threshold;
        rows[b] = StreamOnsetRow{o[b].mode != 0, thr, o[b].keep_lead, 0};
    }
}

}  // namespace vitsmi
