// delivery.hpp — the plan of a delivery (include/vitsmi.h, "delivery"): which rows of the last run go where in the caller's
// byte streams, validated and laid out on the host.  Host-side C++17, no HIP types: like the resampler's plan it is a pure
// function of its arguments, answered without a handle or a device.
//
// The device never sees silence.  It writes ONE packed buffer: the encoded audio of the segments in `dst` order, back to
// back, element p of the packed buffer at byte w * p.  The plan therefore carries three things: the segment table the
// kernels read (DeliverySeg, in dst order, with each segment's first packed element), the copies that move maximal
// silence-free runs of the packed buffer to their place in dst, and the silence regions the host fills itself.
//
// A trimmed delivery (vitsmi.h, "trimmed delivery") is the same plan over a sub-range of every row: `counts` are then the
// kept counts, `first` the kept ranges' first samples, and the trims bring the silence behind each segment.
//
// A levelled delivery (vitsmi.h, "levelled delivery") changes nothing in the layout: once the gains are known, level_apply
// marks the levelled segments of a finished plan and puts each one's gain into its record.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"

namespace vitsmi {

// bytes per element of an encoding; 0: unknown
inline int delivery_width(int encoding) {
    switch (encoding) {
        case VITS_ENC_PCM16: return 2;
        case VITS_ENC_ULAW:
        case VITS_ENC_ALAW: return 1;
        case VITS_ENC_F32: return 4;
    }
    return 0;
}

// one segment as the kernels read it (32 bytes; the table is in dst order, `start` ascending)
struct DeliverySeg {
    int64_t start;  // first packed element of this segment (prefix sum of n)
    int64_t src;    // element offset of the segment's first sample in the waveform: row * pitch (+ the kept range's start)
    int32_t n;      // valid (trimmed: kept) samples of the row
    int32_t peak;   // peak slot to normalise by (row: [0, B); stream: B + stream), -1, or kDeliveryLevelled
    float volume;
    int32_t pad;    // a levelled segment: the bits of its gain (the trim scan's table: the trim's mode)
};
constexpr int32_t kDeliveryLevelled = -2;  // `peak` of a levelled segment: v = x * gain, no normalisation

struct DeliveryCopy {
    int64_t packed_off, dst_off, bytes;
};
struct DeliveryFill {
    int64_t dst_off, elems;
};

struct DeliveryPlan {
    int encoding = 0, width = 0;
    std::vector<int64_t> stream_samples, stream_offsets;  // [J], [J + 1]
    std::vector<DeliverySeg> segs;
    std::vector<int> order;  // segs[k] is the caller's segment order[k]
    std::vector<DeliveryCopy> copies;
    std::vector<DeliveryFill> fills;
    int64_t packed_elems = 0, total_bytes = 0;
    int max_n = 0;          // the longest segment (the peak launch's grid)
    bool any_norm = false;  // some segment normalises: the peak launch is needed
};

// "" or what is wrong with one trim, naming the value (the caller names the segment)
inline std::string trim_fault(const vits_trim &t) {
    char buf[160];
    buf[0] = 0;
    if (t.mode < 0 || t.mode > 2) std::snprintf(buf, sizeof buf, "trim mode %d outside 0..2", t.mode);
    else if (!std::isfinite(t.threshold) || t.threshold < 0) std::snprintf(buf, sizeof buf, "trim threshold %g is not finite and >= 0", (double)t.threshold);
    else if (t.keep_lead < 0) std::snprintf(buf, sizeof buf, "keep_lead %d is negative", t.keep_lead);
    else if (t.keep_tail < 0) std::snprintf(buf, sizeof buf, "keep_tail %d is negative", t.keep_tail);
    else if (t.tail_samples < 0 || t.tail_samples > INT_MAX)
        std::snprintf(buf, sizeof buf, "tail_samples %lld outside [0, %d]", (long long)t.tail_samples, INT_MAX);
    return buf;
}

// the rates a levelled delivery admits (the smallest one bounds the sub-blocks of a row: workspace.hpp, carve_level)
constexpr int kLevelMinRate = 8000, kLevelMaxRate = 192000;

// "" or what is wrong with one level, naming the value (the caller names the segment)
inline std::string level_fault(const vits_level &l) {
    char buf[160];
    buf[0] = 0;
    if (l.mode < 0 || l.mode > 2) std::snprintf(buf, sizeof buf, "level mode %d outside 0..2", l.mode);
    else if (!std::isfinite(l.target_lufs) || l.target_lufs < -70.f || l.target_lufs > 0.f)
        std::snprintf(buf, sizeof buf, "target_lufs %g is not finite and within [-70, 0]", (double)l.target_lufs);
    else if (!std::isfinite(l.max_gain_db) || l.max_gain_db < 0.f || l.max_gain_db > 120.f)
        std::snprintf(buf, sizeof buf, "max_gain_db %g is not finite and within [0, 120]", (double)l.max_gain_db);
    else if (!std::isfinite(l.peak_ceiling) || l.peak_ceiling < 0.f || l.peak_ceiling > 1.f)
        std::snprintf(buf, sizeof buf, "peak_ceiling %g is not finite and within [0, 1]", (double)l.peak_ceiling);
    return buf;
}

// "" or what is wrong with the levels of a plan that delivery_plan has accepted: each level by itself, a levelled segment
// that also normalises, the mode-2 segments of a stream that disagree, the rate.  levels == nullptr: "".
inline std::string level_plan_fault(const vits_segment *segs, const vits_level *levels, int n_segs, int n_streams, int sample_rate) {
    if (!levels) return "";
    char buf[240];
    bool any = false;
    std::vector<int> lead(n_streams, -1);  // a stream's first mode-2 segment
    for (int g = 0; g < n_segs; g++) {
        const vits_level &l = levels[g];
        const std::string e = level_fault(l);
        if (!e.empty()) {
            std::snprintf(buf, sizeof buf, "segment %d: %s", g, e.c_str());
            return buf;
        }
        if (l.mode == 0) continue;
        any = true;
        if (segs[g].normalize != 0) {
            std::snprintf(buf, sizeof buf, "segment %d: normalize %d with level mode %d: a levelled segment is not normalised", g,
                          segs[g].normalize, l.mode);
            return buf;
        }
        if (l.mode != 2) continue;
        const int f = lead[segs[g].stream];
        if (f < 0) {
            lead[segs[g].stream] = g;
            continue;
        }
        const vits_level &o = levels[f];
        if (l.target_lufs != o.target_lufs || l.max_gain_db != o.max_gain_db || l.peak_ceiling != o.peak_ceiling) {
            std::snprintf(buf, sizeof buf, "segment %d: stream level (%g LUFS, %g dB, ceiling %g) differs from segment %d's (%g, %g, %g)", g,
                          (double)l.target_lufs, (double)l.max_gain_db, (double)l.peak_ceiling, f, (double)o.target_lufs,
                          (double)o.max_gain_db, (double)o.peak_ceiling);
            return buf;
        }
    }
    if (any && (sample_rate < kLevelMinRate || sample_rate > kLevelMaxRate)) {
        std::snprintf(buf, sizeof buf, "sample_rate %d outside [%d, %d]", sample_rate, kLevelMinRate, kLevelMaxRate);
        return buf;
    }
    return "";
}

// the kept range [a, a + c) of a row of n valid samples whose first / last active samples are f / l (f > l: none active)
inline void trim_range(int64_t n, int64_t f, int64_t l, const vits_trim &t, int64_t &a, int64_t &c) {
    a = 0;
    c = n;
    if (t.mode == 0) return;
    if (f > l) {
        c = 0;
        return;
    }
    a = f - t.keep_lead > 0 ? f - t.keep_lead : 0;
    const int64_t e = l + 1 + t.keep_tail < n ? l + 1 + t.keep_tail : n;
    c = e - a;
}

// "" or what is wrong with the plan, naming the segment and the value.  counts [B]: the rows' valid samples; pitch: samples
// between two rows of the waveform.  trims [n_segs] (nullable): each is validated and its tail_samples of silence follow its
// segment; first [B] (nullable): the segment of row r starts at sample first[r] of the row - counts[r] is then what is kept
// of it.  Without the two this is the untrimmed plan exactly.
inline std::string delivery_plan(const int64_t *counts, int B, int64_t pitch, const vits_segment *segs, int n_segs, int n_streams,
                                 int encoding, DeliveryPlan &p, const vits_trim *trims = nullptr, const int64_t *first = nullptr) {
    char buf[200];
    const int w = delivery_width(encoding);
    if (!w) {
        std::snprintf(buf, sizeof buf, "unknown encoding %d (0 PCM16, 1 u-law, 2 A-law, 3 F32)", encoding);
        return buf;
    }
    if (B < 1 || !counts) return "delivery: no rows";
    if (n_streams < 1 || n_streams > B) {
        std::snprintf(buf, sizeof buf, "n_streams = %d outside [1, %d]", n_streams, B);
        return buf;
    }
    if (n_segs < 0 || n_segs > B || (n_segs > 0 && !segs)) {
        std::snprintf(buf, sizeof buf, "n_segs = %d outside [0, %d]", n_segs, B);
        return buf;
    }
    std::vector<int> seen(B, -1), per_stream(n_streams + 1, 0);
    for (int g = 0; g < n_segs; g++) {
        const vits_segment &s = segs[g];
        if (s.row < 0 || s.row >= B) {
            std::snprintf(buf, sizeof buf, "segment %d: row %d outside [0, %d)", g, s.row, B);
            return buf;
        }
        if (seen[s.row] >= 0) {
            std::snprintf(buf, sizeof buf, "segment %d: row %d is already in segment %d", g, s.row, seen[s.row]);
            return buf;
        }
        seen[s.row] = g;
        if (s.stream < 0 || s.stream >= n_streams) {
            std::snprintf(buf, sizeof buf, "segment %d: stream %d outside [0, %d)", g, s.stream, n_streams);
            return buf;
        }
        if (s.lead_samples < 0 || s.lead_samples > INT_MAX) {
            std::snprintf(buf, sizeof buf, "segment %d: lead_samples %lld outside [0, %d]", g, (long long)s.lead_samples, INT_MAX);
            return buf;
        }
        if (s.normalize < 0 || s.normalize > 2) {
            std::snprintf(buf, sizeof buf, "segment %d: normalize %d outside 0..2", g, s.normalize);
            return buf;
        }
        if (!std::isfinite(s.volume)) {
            std::snprintf(buf, sizeof buf, "segment %d: volume %g is not finite", g, (double)s.volume);
            return buf;
        }
        if (counts[s.row] < 0 || counts[s.row] > INT_MAX) {
            std::snprintf(buf, sizeof buf, "segment %d: row %d has %lld samples, outside [0, %d]", g, s.row, (long long)counts[s.row], INT_MAX);
            return buf;
        }
        if (trims) {
            const std::string e = trim_fault(trims[g]);
            if (!e.empty()) {
                std::snprintf(buf, sizeof buf, "segment %d: %s", g, e.c_str());
                return buf;
            }
        }
        if (first && (first[s.row] < 0 || first[s.row] > INT_MAX - counts[s.row])) {
            std::snprintf(buf, sizeof buf, "segment %d: row %d is kept from sample %lld on", g, s.row, (long long)first[s.row]);
            return buf;
        }
        per_stream[s.stream + 1]++;
    }
    // dst order: stream by stream, a stream's segments in the order given (a counting sort)
    for (int j = 0; j < n_streams; j++) per_stream[j + 1] += per_stream[j];
    std::vector<int> order(n_segs);
    {
        std::vector<int> at(per_stream.begin(), per_stream.end() - 1);
        for (int g = 0; g < n_segs; g++) order[at[segs[g].stream]++] = g;
    }
    p = DeliveryPlan{};
    p.encoding = encoding;
    p.width = w;
    p.stream_samples.assign(n_streams, 0);
    p.stream_offsets.assign(n_streams + 1, 0);
    p.segs.reserve(n_segs);
    p.order = order;
    int64_t packed = 0, dst = 0;  // elements
    int k = 0;
    for (int j = 0; j < n_streams; j++) {
        p.stream_offsets[j] = dst * w;
        for (; k < per_stream[j + 1]; k++) {
            const vits_segment &s = segs[order[k]];
            const int64_t n = counts[s.row];
            const int64_t tail = trims ? trims[order[k]].tail_samples : 0;
            if (s.lead_samples > 0) {
                p.fills.push_back({dst * w, s.lead_samples});
                dst += s.lead_samples;
            }
            if (n > 0) {
                // a copy runs on while no silence lies in front of the segment: no lead of its own, and (a tail has moved
                // dst on) no tail behind the copy's last segment
                if (!p.copies.empty() && s.lead_samples == 0 && p.copies.back().dst_off + p.copies.back().bytes == dst * w)
                    p.copies.back().bytes += n * w;
                else
                    p.copies.push_back({packed * w, dst * w, n * w});
            }
            DeliverySeg d{};
            d.start = packed;
            d.src = (int64_t)s.row * pitch + (first ? first[s.row] : 0);
            d.n = (int32_t)n;
            d.peak = s.normalize == 1 ? s.row : (s.normalize == 2 ? B + s.stream : -1);
            d.volume = s.volume;
            p.segs.push_back(d);
            p.any_norm = p.any_norm || s.normalize != 0;
            p.max_n = d.n > p.max_n ? d.n : p.max_n;
            packed += n;
            dst += n;
            if (tail > 0) {
                p.fills.push_back({dst * w, tail});
                dst += tail;
            }
            p.stream_samples[j] += s.lead_samples + n + tail;
        }
    }
    p.stream_offsets[n_streams] = dst * w;
    p.packed_elems = packed;
    p.total_bytes = dst * w;
    return "";
}

// a finished plan with the gains of its levelled segments: gain [n_segs] in the caller's order
inline void level_apply(DeliveryPlan &p, const vits_level *levels, const float *gain) {
    for (size_t k = 0; k < p.segs.size() && levels; k++) {
        const int g = p.order[k];
        if (levels[g].mode == 0) continue;
        p.segs[k].peak = kDeliveryLevelled;
        std::memcpy(&p.segs[k].pad, &gain[g], sizeof(float));
    }
}

// the silence regions of dst: the encoding of sample value 0
inline void delivery_silence(const DeliveryPlan &p, void *dst) {
    const int byte = p.encoding == VITS_ENC_ULAW ? 0xFF : (p.encoding == VITS_ENC_ALAW ? 0xD5 : 0);
    for (const DeliveryFill &f : p.fills) std::memset(static_cast<char *>(dst) + f.dst_off, byte, (size_t)(f.elems * p.width));
}

}  // namespace vitsmi
