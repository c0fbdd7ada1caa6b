// stream_run.hip.hpp — the stages a piece of a chunked run goes through behind the generator: the warp's piece entry with its
// history ("streamed pitch") or the resampler's with its carry (include/vitsmi.h, "Output rate"), and the encoded sink's pack, plain ("encoded streaming") or shaped and limited ("shaped
// streaming", stream_shape.hip.hpp), with the scan of a trimmed stream in front ("trimmed streaming", stream_trim.hip.hpp).  The pipeline (vitsmi.hip, render_chunks) and the hooks vits_test_resample_pieces /
// vits_test_stream_pack / _shaped run THESE functions.  Nothing here knows a handle.  The buffers are carve_stream's (workspace.hpp);
// errors come back as hipError_t, launch counts by reference.  All is enqueued on the caller's stream; the caller copies out and waits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "resample.hip.hpp"
#include "stream_shape.hip.hpp"
#include "stream_trim.hip.hpp"
#include "warp.hip.hpp"
#include "workspace.hpp"

namespace vitsmi {

// ---- resampled pieces: the batch path's [B][S_out], bit for bit, whatever the pieces
struct ResampleRun {
    ResamplePlan plan;
    ResampleArgs a{};  // what every piece shares: the table, the rows' counts, the output buffer
    float *carry[2] = {nullptr, nullptr};
    int S_out = 0;
    int gen = 0;      // the carry generation in front of the next piece
    int emitted = 0;  // output samples delivered so far
};

// the rows' counts (ylen[b] * hop, without frame counts n_all; at most n_all) and a zero carry in front of the first piece
inline hipError_t resample_run_begin(ResampleRun &r, const ResampleDev &dev, const ResampleBufs &rb, const int *ylen, int hop, int n_all,
                                     int S_out, int B, hipStream_t st) {
    r = ResampleRun{dev.plan, resample_args(dev), {rb.carry[0], rb.carry[1]}, S_out};
    r.a.n_in = rb.n_in;
    r.a.n_out = rb.n_out;
    r.a.y = rb.out;
    resample_counts_kernel<<<(B + 63) / 64, 64, 0, st>>>(ylen, hop, n_all, dev.plan.L, dev.plan.M, rb.n_in, rb.n_out, B);
    return hipMemsetAsync(rb.carry[0], 0, (size_t)B * dev.plan.K * sizeof(float), st);
}

// The piece x [B][n], input samples [first, first + n) of every row: "carry | piece" in, the output samples whose K inputs now all
// exist - the last piece: the rest - out to rb.out as [B][e_n], they are [e_first, e_first + e_n); behind every piece but the last the
// carry's other generation.  e_n == 0: it completes nothing.  (launches: two per piece, as a run's statistics have always counted.)
inline hipError_t resample_run_piece(ResampleRun &r, const float *x, int64_t x_pitch, int64_t first, int64_t n, bool is_last, int B,
                                     hipStream_t st, int64_t &e_first, int64_t &e_n, int &launches) {
    const int n_hi = (int)resample_emit_end(r.plan, first + n, is_last, r.S_out), ne = n_hi - r.emitted;
    ResampleArgs a = r.a;
    a.x = x;
    a.x_pitch = x_pitch;
    a.x_first = (int)first;
    a.x_n = (int)n;
    a.carry = r.carry[r.gen];
    a.y_pitch = ne;  // (the previous piece's copy-out precedes this one on the stream)
    a.y_first = r.emitted;
    a.n_lo = r.emitted;
    a.n_hi = n_hi;
    hipError_t e = launch_resample(a, B, /*piece=*/true, st);
    if (e == hipSuccess && !is_last) {
        resample_carry_kernel<<<dim3((unsigned)((a.K + 255) / 256), B), 256, 0, st>>>(a.carry, x, x_pitch, a.x_n, a.K, r.carry[r.gen ^ 1]);
        e = hipGetLastError();
        r.gen ^= 1;
    }
    launches = 2;
    e_first = r.emitted;
    e_n = ne > 0 ? ne : 0;
    if (ne > 0) r.emitted = n_hi;
    return e;
}

// ---- warped pieces ("streamed pitch"): the whole run's [B][S_w], bit for bit, whatever the pieces.  The stage in FRONT of the others:
// it keeps the native waveform (the history), and what a piece completes by the emit rule (warp.hpp) leaves it on the output timeline.

// A WarpRun's plan is one of four: records of either family (`glide`: which kernel a window launches) under native or folded
// rows (`folded`, "pitch at an output rate": WarpRateRow in place of WarpRow, the wide kernels).  One record vector and one row
// vector are in use.  THE choice among the four: f(the run's records, the run's rows), both as their typed vectors - nothing
// else looks at the flags.  (r: a WarpRun, const or not.)
template <class Run, class F>
inline auto warp_run_visit(Run &r, F f) {
    if (r.folded) return r.glide ? f(r.gsegs, r.rrows) : f(r.wsegs, r.rrows);
    return r.glide ? f(r.gsegs, r.rows) : f(r.wsegs, r.rows);
}

struct WarpRun {
    bool glide = false, folded = false;
    std::vector<vits_warp_seg> wsegs;
    std::vector<vits_glide_seg> gsegs;
    std::vector<WarpRow> rows;          // [B]
    std::vector<WarpRateRow> rrows;     // [B]
    std::vector<int32_t> first;         // [B + 1]
    std::vector<int64_t> spans;         // [B][T]: k per token, as vits_last_token_spans reports it
    int64_t S_w = 0, n_cap = 0;
    int64_t half = kWarpMaxHalf;        // the largest Kh the emit rule counts with (warp_plan_extent)
    int64_t emitted = 0, e_end = 0;     // output samples delivered so far / complete behind the last piece
    WarpStreamBufs wb{};
    const float *G = nullptr;
    std::vector<char> up;               // (pageable source of the plan's upload where the caller has no pinned block)
    size_t row_bytes() const { return warp_run_visit(*this, [](auto &, auto &rows) { return sizeof(rows[0]); }); }
    int32_t row_out(int b) const { return warp_run_visit(*this, [b](auto &, auto &rows) { return rows[(size_t)b].n_out; }); }
    int64_t n_segs() const { return warp_run_visit(*this, [](auto &segs, auto &) { return (int64_t)segs.size(); }); }
};

// The plan [segs | rows] and the rows' output counts, uploaded once; pin (nullable): plan_bytes + 4 B bytes of pinned memory.
inline hipError_t warp_run_begin(WarpRun &r, const WarpStreamBufs &wb, const float *G, int64_t n_cap, int B, char *pin, hipStream_t st) {
    r.wb = wb;
    r.G = G;
    r.n_cap = n_cap;
    r.emitted = r.e_end = 0;
    if (!pin) {
        r.up.resize(wb.plan_bytes + (size_t)B * sizeof(int));
        pin = r.up.data();
    }
    int *pin_nout = reinterpret_cast<int *>(pin + wb.plan_bytes);
    warp_run_visit(r, [&](auto &segs, auto &rows) {
        const size_t seg_bytes = segs.size() * sizeof(segs[0]);
        if (seg_bytes) std::memcpy(pin, segs.data(), seg_bytes);
        std::memcpy(pin + seg_bytes, rows.data(), (size_t)B * sizeof(rows[0]));
        for (int b = 0; b < B; b++) pin_nout[b] = rows[(size_t)b].n_out;
    });
    hipError_t e = hipMemcpyAsync(wb.segs, pin, wb.plan_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(wb.n_out, pin_nout, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st);
    return e;
}

// The piece x [B][n], input samples [first, first + n) of every row, joins the history; what then exists of the output - e(first + n)
// by the emit rule - is r.e_end.  Nothing is launched: warp_run_window renders [emitted, e_end) in windows of at most n_cap.
inline hipError_t warp_run_piece(WarpRun &r, const float *x, int64_t x_pitch, int64_t first, int64_t n, bool is_last, int B, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (n > 0)
        e = hipMemcpy2DAsync(r.wb.hist + first, (size_t)r.wb.hist_pitch * 4, x, (size_t)x_pitch * 4, (size_t)n * 4, B, hipMemcpyDeviceToDevice, st);
    const int64_t end = warp_run_visit(r, [&](auto &segs, auto &rows) { return warp_emit_end(segs.data(), rows, r.S_w, first + n, is_last, r.half); });
    r.e_end = end > r.e_end ? end : r.e_end;
    return e;
}

// The next window of what the last piece completed: output samples [e_first, e_first + e_n) of every row at y [B][e_n], one launch.
// e_n == 0: nothing is left of it (a piece that completes nothing: at once).
inline hipError_t warp_run_window(WarpRun &r, int B, hipStream_t st, const float *&y, int64_t &e_first, int64_t &e_n, int &launches) {
    const int64_t left = r.e_end - r.emitted;
    e_first = r.emitted;
    e_n = left < r.n_cap ? left : r.n_cap;
    launches = 0;
    if (e_n <= 0) {
        e_n = 0;
        return hipSuccess;
    }
    y = r.wb.out;
    launches = 1;
    r.emitted += e_n;
    return warp_run_visit(r, [&](auto &segs, auto &rows) {
        using Seg = std::decay_t<decltype(segs[0])>;
        using Row = std::decay_t<decltype(rows[0])>;
        WarpArgsT<Seg, Row> a{};
        a.segs = reinterpret_cast<const Seg *>(r.wb.segs);
        a.rows = static_cast<const Row *>(r.wb.rows);
        a.G = r.G;
        a.x = r.wb.hist;
        a.x_pitch = r.wb.hist_pitch;
        a.y = r.wb.out;  // (the previous window's pack or copy-out precedes this one on the stream)
        a.y_pitch = e_n;
        a.n_lo = (int)e_first;
        a.n_hi = (int)(e_first + e_n);
        return launch_warp_tile(a, B, st);
    });
}

// ---- packed pieces: the encoded sink.  A piece reaches sp's chunk buffer as [B][pitch] bytes that end at the running peaks.
struct StreamPackRun {
    int encoding = 0, width = 0;
    bool norm = false, shaped = false;
    StreamPackBufs sp{};
    StreamPackRows rows{nullptr, 1, 0};
    int64_t total = 0;
    StreamShapeRun shape;
    std::vector<float> up;  // (pageable source of an asynchronous copy: lives until the pieces behind it have been waited for)
    // a trimmed stream: the scan's records, and whether the next piece is still scanned - until the host has read back that
    // every trimmed row's start is known or the row has ended (stream_pack_seen)
    bool trimmed = false, scan = false;
    std::vector<StreamOnsetRow> onsets;
    std::vector<int64_t> row_n;  // the rows' valid samples, where the caller has them on the host (else: empty)
    // bytes one copy takes behind a chunk's B * pitch: the running peaks - and a trimmed stream's starts behind them
    size_t tail_bytes(int B) const { return trimmed ? (StreamPackBufs::peak_floats(B) + (size_t)B) * sizeof(float) : (size_t)B * sizeof(float); }
};

// The per-run upload [zeros of the running peaks | {ref_peak, volume} per row] in one copy and, with a `shaping` (nullptr: the
// plain kernel), its records and knots.  fmt and shaping are validated; rows / total: the rows' valid samples and their length.
// onsets (nullable, validated; every mode 0: as nullptr): a trimmed stream - it takes the shaped kernels whatever the shaping,
// sp and ss are carved `trimmed`, and the upload is [peaks | starts: 0, or kStreamNoStart for a trimmed row | table].
// row_n (nullable): the rows' valid samples on the host, for stream_pack_seen.
inline hipError_t stream_pack_begin(StreamPackRun &r, const vits_stream_format *fmt, const vits_stream_shaping *shaping, int B,
                                    const StreamPackBufs &sp, const StreamShapeBufs &ss, const StreamPackRows &rows, int64_t total,
                                    hipStream_t st, const vits_stream_onset *onsets = nullptr, const int64_t *row_n = nullptr) {
    static const vits_stream_shaping none{};
    r.encoding = fmt->encoding;
    r.width = delivery_width(fmt->encoding);
    r.norm = fmt->ref_peak != nullptr;
    r.trimmed = r.scan = stream_trimmed(onsets, B);
    r.shaped = shaping != nullptr || r.trimmed;
    r.sp = sp;
    r.rows = rows;
    r.total = total;
    r.row_n.clear();
    if (row_n) r.row_n.assign(row_n, row_n + B);
    const size_t Bp = StreamPackBufs::peak_floats(B), Bs = r.trimmed ? Bp : 0;
    r.up.assign(Bp + Bs + 2 * (size_t)B, 0.f);
    if (r.trimmed) {
        stream_onset_table(onsets, fmt->ref_peak, B, r.onsets);
        for (int b = 0; b < B; b++) {
            const int32_t s0 = r.onsets[b].on ? kStreamNoStart : 0;
            std::memcpy(&r.up[Bp + b], &s0, sizeof s0);
        }
    }
    for (int b = 0; b < B; b++) {
        r.up[Bp + Bs + 2 * b] = fmt->ref_peak ? fmt->ref_peak[b] : 1.0f;
        r.up[Bp + Bs + 2 * b + 1] = fmt->volume ? fmt->volume[b] : 1.0f;
    }
    hipError_t e = hipMemcpyAsync(sp.peak_run, r.up.data(), r.up.size() * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && r.trimmed)
        e = hipMemcpyAsync(ss.onsets, r.onsets.data(), r.onsets.size() * sizeof(StreamOnsetRow), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && r.shaped) e = stream_shape_begin(r.shape, shaping ? shaping : &none, B, ss, st);
    return e;
}

// What the host has read back behind a chunk that delivered through `delivered_end`: start [B].  Once every trimmed row's start
// is known, or the row has ended in front of delivered_end (what is delivered has been scanned), no later piece is scanned.
inline void stream_pack_seen(StreamPackRun &r, const int32_t *start, int64_t delivered_end, int B) {
    if (!r.scan) return;
    for (int b = 0; b < B; b++) {
        const int64_t nb = r.row_n.empty() ? r.total : r.row_n[b];
        if (r.onsets[b].on && start[b] == kStreamNoStart && nb > delivered_end) return;
    }
    r.scan = false;
}

// The piece x [B][n] at `first`: what it delivers - itself or, shaped with a look-ahead, the range that far behind it - as [B][pitch]
// bytes at d with the running peaks behind, for one copy.  e_n == 0: it lies inside the look-ahead, nothing was delivered, d is not set.
inline hipError_t stream_pack_piece(StreamPackRun &r, const float *x, int64_t x_pitch, int64_t first, int64_t n, int B, hipStream_t st,
                                    unsigned char *&d, int64_t &e_first, int64_t &e_n, size_t &pitch, int &launches) {
    pitch = StreamPackBufs::pitch(r.width, n);
    if (r.shaped) {
        if (r.scan) {  // in front of the pack launch; D: what stream_shape_chunk is about to compute
            int64_t D = 0, dn = 0;
            stream_emit_range(first, n, first + n >= r.total, r.total, r.shape.L, D, dn);
            const hipError_t es = launch_stream_onset(x, x_pitch, r.rows, B, (int)first, (int)n, (int)D, r.shape.ss.onsets, r.sp.start, st);
            if (es != hipSuccess) return es;
        }
        const bool scanned = r.scan;
        const hipError_t e = stream_shape_chunk(r.shape, r.encoding, r.width, x, x_pitch, r.rows, B, first, n, r.total, r.sp, r.norm, st, e_first,
                                                e_n, d, launches);
        pitch = StreamPackBufs::pitch(r.width, e_n);
        launches += scanned ? 1 : 0;
        return e;
    }
    e_first = first;
    e_n = n;
    d = r.sp.at(B, pitch);
    launches = 1;
    return launch_stream_pack(r.encoding, x, x_pitch, r.rows, B, (int)first, (int)n, r.sp.fmt, r.norm, d, r.sp.peak_run, st);
}

}  // namespace vitsmi
