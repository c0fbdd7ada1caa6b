// delivery_run.hip.hpp — a delivery from start to finish over a waveform on the device (include/vitsmi.h, "delivery" to
// "shaped delivery"): the stages - the scan, the measurement, the enqueue, the reports - and delivery_run, the ONE sequence
// behind vits_deliver, vits_deliver_trimmed / _leveled / _shaped / _limited and the vits_test_deliver* hooks (vitsmi.hip).
//
// Nothing here knows a handle.  Where the handle and a hook differ they hand it in: how the call's buffers (workspace.hpp,
// carve_delivery_call) are obtained, and what follows the call's first wait.  Refusals come back as a code and a message
// for the caller's own fail().
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vitsmi.h"
#include "delivery.hip.hpp"
#include "limit.hip.hpp"
#include "loudness.hip.hpp"
#include "shape.hip.hpp"
#include "workspace.hpp"

namespace vitsmi {

// what a shaped delivery adds to the enqueue: the records of the plan's segments and their knots (host), and carve_shape's
// buffers they go to.  The vectors are the pageable sources of copies: they outlive the caller's wait.
struct ShapeJob {
    std::vector<ShapeSeg> table;
    std::vector<ShapeKnot> knots;
    ShapeBufs sb{};
};

// the job of a finished plan p (over the kept ranges first / kept [B]); shapes have passed shape_fault (nullptr: a limited
// call without shapes - every segment gets the shape without fades and points)
inline void shape_job(const DeliveryPlan &p, const vits_segment *segs, const vits_shape *shapes, const vits_env_point *points,
                      const std::vector<int64_t> &first, const std::vector<int64_t> &kept, ShapeJob &job) {
    std::vector<int64_t> a(p.order.size()), c(p.order.size());
    const std::vector<vits_shape> none(shapes ? 0 : p.order.size(), vits_shape{});
    if (!shapes) shapes = none.data();
    for (size_t k = 0; k < p.order.size(); k++) {
        const int row = segs[p.order[k]].row;
        a[k] = first[row];
        c[k] = kept[row];
    }
    shape_table(shapes, p.order, a.data(), c.data(), job.table);
    shape_knots(job.table, points, job.knots);
}

// what a limited delivery adds on top of a ShapeJob: the records of the plan's segments (host) and carve_limit's buffers
struct LimitJob {
    std::vector<LimitSeg> table;
    LimitBufs lb{};
};

// Everything a delivery puts on the stream: segment table up, peaks cleared, the launches, the copies into dst; then the
// silence, on the host.  The caller synchronises.  db: carve_delivery's buffers for a waveform of at least the plan's rows.
// job: a shaped delivery's tables (nullptr: none - launch_delivery, as ever).  lim: a limited delivery's (nullptr: none;
// with one, `job` is there too - launch_delivery_limited in the place of launch_delivery_shaped).
inline hipError_t delivery_enqueue(const float *d_x, const DeliveryPlan &p, const DeliveryBufs &db, int B, hipStream_t st, void *dst,
                                   const ShapeJob *job = nullptr, const LimitJob *lim = nullptr) {
    hipError_t e = hipSuccess;
    if (p.packed_elems > 0) {
        e = hipMemcpyAsync(db.segs, p.segs.data(), p.segs.size() * sizeof(DeliverySeg), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && p.any_norm) e = hipMemsetAsync(db.peak, 0, 2 * (size_t)B * sizeof(unsigned), st);
        if (job) {
            if (e == hipSuccess) e = hipMemcpyAsync(job->sb.segs, job->table.data(), job->table.size() * sizeof(ShapeSeg), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(job->sb.knots, job->knots.data(), job->knots.size() * sizeof(ShapeKnot), hipMemcpyHostToDevice, st);
            if (lim) {
                if (e == hipSuccess) e = hipMemcpyAsync(lim->lb.segs, lim->table.data(), lim->table.size() * sizeof(LimitSeg), hipMemcpyHostToDevice, st);
                if (e == hipSuccess)
                    e = launch_delivery_limited(d_x, p, db.segs, db.peak, db.packed, job->sb.segs, job->sb.knots, lim->lb.segs, lim->lb.gain, st);
            } else if (e == hipSuccess)
                e = launch_delivery_shaped(d_x, p, db.segs, db.peak, db.packed, job->sb.segs, job->sb.knots, st);
        } else if (e == hipSuccess)
            e = launch_delivery(d_x, p, db.segs, db.peak, db.packed, st);
        for (size_t i = 0; i < p.copies.size() && e == hipSuccess; i++)
            e = hipMemcpyAsync(static_cast<char *>(dst) + p.copies[i].dst_off, db.packed + p.copies[i].packed_off,
                               (size_t)p.copies[i].bytes, hipMemcpyDeviceToHost, st);
    }
    delivery_silence(p, dst);
    return e;
}

inline void delivery_report(const DeliveryPlan &p, int64_t *stream_samples, int64_t *stream_offsets) {
    for (size_t j = 0; j < p.stream_samples.size() && stream_samples; j++) stream_samples[j] = p.stream_samples[j];
    for (size_t j = 0; j < p.stream_offsets.size() && stream_offsets; j++) stream_offsets[j] = p.stream_offsets[j];
}

// ---- trimmed delivery (vitsmi.h, "trimmed delivery"): the scan in front of the delivery, the kept ranges and the plan
// over them on the host in between

// The scan of the plan p0 (over the whole rows) and the wait for it: first / kept [B] receive every row's kept range (rows
// outside the plan, and segments whose trim is off: the whole row).  Waits whatever happened: the tables are the pageable
// sources of copies that may be in flight.
inline hipError_t trim_scan(const float *d_x, const DeliveryPlan &p0, const vits_segment *segs, const vits_trim *trims, const int64_t *counts,
                            int B, const DeliveryBufs &db, const TrimBufs &tb, hipStream_t st, std::vector<int64_t> &first,
                            std::vector<int64_t> &kept) {
    first.assign(B, 0);
    kept.assign(counts, counts + B);
    const int G = (int)p0.segs.size();
    std::vector<DeliverySeg> scan(p0.segs);
    std::vector<int32_t> bounds(2 * (size_t)G);
    bool any = false, any_rel = false;
    for (int k = 0; k < G && trims; k++) {
        const vits_trim &t = trims[p0.order[k]];
        scan[k].peak = t.mode == 2 ? k : -1;
        scan[k].volume = t.threshold;
        scan[k].pad = t.mode;
        bounds[2 * k] = INT_MAX;
        bounds[2 * k + 1] = -1;
        any = any || t.mode != 0;
        any_rel = any_rel || t.mode == 2;
    }
    hipError_t e = hipSuccess;
    if (any && p0.max_n > 0) {  // (rows without samples keep their presets: none active)
        e = hipMemcpyAsync(db.segs, scan.data(), (size_t)G * sizeof(DeliverySeg), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(tb.bounds, bounds.data(), bounds.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && any_rel) e = hipMemsetAsync(tb.peak_all, 0, (size_t)G * sizeof(unsigned), st);
        if (e == hipSuccess) e = launch_trim_scan(d_x, db.segs, G, p0.max_n, any_rel, tb.peak_all, tb.bounds, st);
        if (e == hipSuccess) e = hipMemcpyAsync(bounds.data(), tb.bounds, bounds.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    }
    const hipError_t done = hipStreamSynchronize(st);
    if (e == hipSuccess) e = done;
    if (e != hipSuccess || !any) return e;
    for (int k = 0; k < G; k++) {
        const int g = p0.order[k], row = segs[g].row;
        trim_range(counts[row], bounds[2 * k], bounds[2 * k + 1], trims[g], first[row], kept[row]);
    }
    return hipSuccess;
}

inline void trim_report(const vits_segment *segs, int n_segs, const std::vector<int64_t> &first, const std::vector<int64_t> &kept,
                        int64_t *kept_first, int64_t *kept_count) {
    for (int g = 0; g < n_segs; g++) {
        if (kept_first) kept_first[g] = first[segs[g].row];
        if (kept_count) kept_count[g] = kept[segs[g].row];
    }
}

// ---- levelled delivery (vitsmi.h, "levelled delivery"): the measurement between the kept ranges and the delivery

inline bool any_level(const vits_level *levels, int n_segs) {
    for (int g = 0; g < n_segs && levels; g++)
        if (levels[g].mode != 0) return true;
    return false;
}

// The loudness and peak launches over the plan p (over the kept ranges), the copy of energies and peaks, the wait, then
// gates and gains on the host: loud / gain [n_segs] in the caller's order (mode 0: NaN / 1).  Waits whatever happened: the
// tables are the pageable sources of copies that may be in flight.
inline hipError_t level_measure(const float *d_x, const DeliveryPlan &p, const vits_segment *segs, const vits_level *levels, int n_segs,
                                int n_streams, int sample_rate, const DeliveryBufs &db, const LevelBufs &lb, hipStream_t st,
                                std::vector<double> &loud, std::vector<float> &gain) {
    loud.assign(n_segs, std::numeric_limits<double>::quiet_NaN());
    gain.assign(n_segs, 1.0f);
    if (!any_level(levels, n_segs)) return hipSuccess;
    const LoudCoef k = loudness_coef(sample_rate);
    const int G = (int)p.segs.size();
    std::vector<DeliverySeg> table(p.segs);  // the peak launch's: slot k for a levelled segment
    std::vector<LoudSeg> ls;                 // the loudness launches': the levelled segments only
    std::vector<int> ls_k;                   // ... and which of the plan's each one is
    std::vector<int32_t> n_sub(G, 0);
    int64_t chunks = 0, subs = 0;
    int max_n = 0;
    for (int kk = 0; kk < G; kk++) {
        table[kk].peak = -1;
        if (levels[p.order[kk]].mode == 0) continue;
        table[kk].peak = kk;
        n_sub[kk] = p.segs[kk].n / k.hop;
        LoudSeg s{};
        s.src = p.segs[kk].src;
        s.chunk0 = chunks;
        s.sub0 = subs;
        s.n = n_sub[kk] * k.hop;
        chunks += ((int64_t)s.n + kLoudChunk - 1) / kLoudChunk;
        subs += n_sub[kk];
        max_n = s.n > max_n ? s.n : max_n;
        ls.push_back(s);
        ls_k.push_back(kk);
    }
    if ((size_t)chunks > lb.n_chunks || (size_t)subs > lb.n_subs || (size_t)G > lb.n_peaks) return hipErrorInvalidValue;  // (cannot happen: carve_level)
    std::vector<unsigned> result(lb.n_peaks + (size_t)subs, 0u);
    hipError_t e = hipSuccess;
    if (p.max_n > 0) {  // (segments without samples: peak 0, no sub-blocks)
        e = hipMemcpyAsync(db.segs, table.data(), (size_t)G * sizeof(DeliverySeg), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemsetAsync(lb.result, 0, lb.n_peaks * sizeof(unsigned), st);
        if (e == hipSuccess) e = launch_level_peaks(d_x, db.segs, G, p.max_n, lb.result, st);
        if (e == hipSuccess && max_n > 0) {
            e = hipMemcpyAsync(lb.segs, ls.data(), ls.size() * sizeof(LoudSeg), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = launch_loudness(d_x, lb.segs, (int)ls.size(), max_n, k, lb.fin, lb.init, lb.part, lb.e(), st);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(result.data(), lb.result, result.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st);
    }
    const hipError_t done = hipStreamSynchronize(st);
    if (e == hipSuccess) e = done;
    if (e != hipSuccess) return e;
    const float *peaks = reinterpret_cast<const float *>(result.data());
    const float *en = peaks + lb.n_peaks;
    // mode 1: a segment by itself
    for (size_t i = 0; i < ls.size(); i++) {
        const int kk = ls_k[i], g = p.order[kk];
        if (levels[g].mode != 1) continue;
        loud[g] = loudness_gate(en + ls[i].sub0, &n_sub[kk], 1, k.hop).L;
        gain[g] = level_gain(loud[g], peaks[kk], levels[g]);
    }
    // mode 2: the stream's mode-2 segments pooled (the plan's order within a stream is the caller's)
    for (int j = 0; j < n_streams; j++) {
        std::vector<float> pool;
        std::vector<int32_t> pool_n;
        float peak = 0.f;
        int lead = -1;
        for (size_t i = 0; i < ls.size(); i++) {
            const int kk = ls_k[i], g = p.order[kk];
            if (levels[g].mode != 2 || segs[g].stream != j) continue;
            lead = lead < 0 ? g : lead;
            pool.insert(pool.end(), en + ls[i].sub0, en + ls[i].sub0 + n_sub[kk]);
            pool_n.push_back(n_sub[kk]);
            peak = fmaxf(peak, peaks[kk]);
        }
        if (lead < 0) continue;
        const double L = loudness_gate(pool.data(), pool_n.data(), (int)pool_n.size(), k.hop).L;
        const float gn = level_gain(L, peak, levels[lead]);
        for (int g = 0; g < n_segs; g++)
            if (levels[g].mode == 2 && segs[g].stream == j) {
                loud[g] = L;
                gain[g] = gn;
            }
    }
    return hipSuccess;
}

inline void level_report(int n_segs, const std::vector<double> &loud, const std::vector<float> &gn, double *loudness, float *gain) {
    for (int g = 0; g < n_segs; g++) {
        if (loudness) loudness[g] = loud[g];
        if (gain) gain[g] = gn[g];
    }
}

// ---- the one sequence

// a VITS code and its message
struct DeliveryStatus {
    int code = VITS_OK;
    std::string msg;
};

inline DeliveryStatus delivery_refusal(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return {code, buf};
}

// what a call asks for (trims, levels, shapes and points: nullable, as in vitsmi.h) ...
struct DeliveryRequest {
    const vits_segment *segs;
    const vits_trim *trims;
    const vits_level *levels;
    const vits_shape *shapes;
    const vits_env_point *points;
    int64_t n_points;
    int n_segs, n_streams, encoding, sample_rate;
    void *dst;
    size_t dst_bytes;
    bool kept;  // the scan and the measurement in front of the delivery: every entry but vits_deliver and vits_test_deliver
    const vits_limit *limits = nullptr;  // (nullable; behind the rest: the entries without limits state none)
};

// ... and where it wants the answers (each nullable)
struct DeliveryOutputs {
    int64_t *stream_samples, *stream_offsets, *kept_first, *kept_count;
    double *loudness;
    float *gain;
};

// A delivery of the waveform [B][S] whose rows hold counts [B] valid samples, on `st`.
//   bufs(need, d_x, cb) -> DeliveryStatus: called once, when the request has passed every check that needs no device and
//       a plain delivery is known to have a dst that is large enough - nothing is enqueued or allocated before.  It yields
//       the waveform on the device and the call's buffers, carved by carve_delivery_call with `need`.
//   waited() -> DeliveryStatus: called behind the call's first wait - the scan's in a kept delivery (which always waits,
//       trims or none), the only one in a plain delivery.
// A plain delivery (!rq.kept): without dst the layout is reported and nothing else happens; with one nothing is waited for
// before the enqueue.  A kept one: dst == nullptr still scans and measures; a dst that is too small for the kept ranges is
// refused after the scan, untouched.
template <class Bufs, class Waited>
DeliveryStatus delivery_run(const int64_t *counts, int B, int S, hipStream_t st, const DeliveryRequest &rq, const DeliveryOutputs &out,
                            Bufs &&bufs, Waited &&waited) {
    DeliveryPlan p0;  // over the whole rows: the validation, a plain delivery's plan, and the table the scan reads
    std::string e = delivery_plan(counts, B, S, rq.segs, rq.n_segs, rq.n_streams, rq.encoding, p0, rq.trims);
    if (e.empty()) e = level_plan_fault(rq.segs, rq.levels, rq.n_segs, rq.n_streams, rq.sample_rate);
    if (e.empty()) e = shape_fault(rq.shapes, rq.n_segs, rq.points, rq.n_points);
    if (e.empty()) e = limit_fault(rq.limits, rq.segs, rq.n_segs);
    if (!e.empty()) return {VITS_E_ARG, e};
    const bool limited = rq.kept && any_limit(rq.limits, rq.n_segs);
    const bool shaped = limited || any_shape(rq.shapes, rq.n_segs);  // (the limiter's kernels read every segment's shape record)
    const DeliveryNeeds need{rq.kept, any_level(rq.levels, rq.n_segs), shaped,
                             rq.shapes ? shape_knot_count(rq.shapes, rq.n_segs) : (limited ? (int64_t)rq.n_segs : 0), limited};
    if (!rq.kept) {
        if (!rq.dst) {  // the layout only: nothing is enqueued, nothing waited for
            delivery_report(p0, out.stream_samples, out.stream_offsets);
            return {};
        }
        if (rq.dst_bytes < (size_t)p0.total_bytes)
            return delivery_refusal(VITS_E_ARG, "delivery buffer too small: %zu bytes, %lld needed", rq.dst_bytes, (long long)p0.total_bytes);
    }
    const float *d_x = nullptr;
    DeliveryCallBufs cb{};
    if (DeliveryStatus s = bufs(need, d_x, cb); s.code) return s;
    std::vector<int64_t> first, kept;
    std::vector<double> loud;
    std::vector<float> gn;
    DeliveryPlan pk;  // over the kept ranges
    if (rq.kept) {
        hipError_t err = trim_scan(d_x, p0, rq.segs, rq.trims, counts, B, cb.dlv, cb.trim, st, first, kept);
        if (err != hipSuccess) return delivery_refusal(VITS_E_DEVICE, "trim scan failed: %s", hipGetErrorString(err));
        if (DeliveryStatus s = waited(); s.code) return s;
        e = delivery_plan(kept.data(), B, S, rq.segs, rq.n_segs, rq.n_streams, rq.encoding, pk, rq.trims, first.data());
        if (!e.empty()) return {VITS_E_ARG, e};
        if (rq.dst && rq.dst_bytes < (size_t)pk.total_bytes)
            return delivery_refusal(VITS_E_ARG, "delivery buffer too small: %zu bytes, %lld needed", rq.dst_bytes, (long long)pk.total_bytes);
        err = level_measure(d_x, pk, rq.segs, rq.levels, rq.n_segs, rq.n_streams, rq.sample_rate, cb.dlv, cb.level, st, loud, gn);
        if (err != hipSuccess) return delivery_refusal(VITS_E_DEVICE, "loudness measurement failed: %s", hipGetErrorString(err));
        level_apply(pk, rq.levels, gn.data());
    }
    const DeliveryPlan &p = rq.kept ? pk : p0;
    ShapeJob job;
    LimitJob lim;
    if (rq.dst) {
        job.sb = cb.shape;
        lim.lb = cb.limit;
        if (shaped) shape_job(p, rq.segs, rq.shapes, rq.points, first, kept, job);
        if (limited) limit_table(rq.limits, p.order, lim.table);
        // (wait whatever the enqueue answered: the plan's tables are the pageable sources of copies that may be in flight)
        hipError_t err = delivery_enqueue(d_x, p, cb.dlv, B, st, rq.dst, shaped ? &job : nullptr, limited ? &lim : nullptr);
        const hipError_t done = hipStreamSynchronize(st);
        if (err == hipSuccess) err = done;
        if (err != hipSuccess) return delivery_refusal(VITS_E_DEVICE, "delivery failed: %s", hipGetErrorString(err));
        if (!rq.kept)
            if (DeliveryStatus s = waited(); s.code) return s;
    }
    delivery_report(p, out.stream_samples, out.stream_offsets);
    if (rq.kept) {
        trim_report(rq.segs, rq.n_segs, first, kept, out.kept_first, out.kept_count);
        level_report(rq.n_segs, loud, gn, out.loudness, out.gain);
    }
    return {};
}

}  // namespace vitsmi
