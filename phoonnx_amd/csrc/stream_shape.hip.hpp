// stream_shape.hip.hpp — the kernels of a shaped, limited encoded stream (include/vitsmi.h, "shaped streaming"; the plan:
// stream_shape.hpp).
//
// They stand beside stream_pack_kernel (stream_pack.hip.hpp), which is not touched: a stream without fades, points and
// limiter launches exactly what it launched before.  A row of the stream is a segment of the limited delivery that keeps the
// whole row - kept range [0, n_b), peak := ref_peak[b], no level gain - and both kernels form the unlimited value u of a
// sample with ONE function, stream_shape_value: limit_value's operations (limit.hip.hpp) in its order, with shape.hpp's
// multiplier and the knot walk by row position.
//
// stream_pack_shaped_kernel<ENC> (L = 0) is stream_pack_kernel with that multiplier in front of the clip; the fades count
// against n_b, which it reads from StreamPackRows like the valid count.
//
// stream_pack_limited_kernel<ENC> (L > 0) is ONE launch per chunk: the gain never leaves LDS.  The rendered piece is
// [first, first + n); the launch delivers [e0, e0 + en), L samples behind it (stream_shape.hpp, stream_emit_range).  Grid
// (tiles of the delivered range, B); a workgroup owns kStreamTile delivered elements of one row - whole 16-byte cells in
// every encoding - and
//   stages  q[j] for j in [d0 - L, d0 + nt + L) in LDS, and u of its own elements beside it: a sample in front of `first`
//           comes from the carry (the last 2 L raw samples of the row in front of the piece), one from `first` on from the
//           piece; 65536 outside [0, n_b) without loading - behind a row's end lies whatever the generator rendered;
//   runs    limit_window_sums (limit.hip.hpp): the doubling minima and the int32 prefix sums of limit_gain_kernel, the one
//           parallel form of the rule - skipped where no staged sample is above the ceiling (g = S / S = 1.0f by the rule);
//   applies g = limit_g(S), the product and the clamp (limit.hpp), the clip and the encoder, parks the elements in LDS and
//           stores whole 16-byte cells, silence cells included.
// A row that is not limited (ceiling 0) gets g = 1 and no clamp, with the same delay: a chunk stays rectangular.
// The running peak folds |x| of the staged samples from `fold_from` on - the samples rendered since the last launch; pieces
// that completed nothing made none, and theirs are still in the carry - into one atomicMax per wave, as stream_pack_kernel.
// Every loop that holds a barrier runs a trip count that depends on the tile and L alone.  LDS is static: limit_gain_kernel's
// two buffers (32 KiB), u of a tile (8 KiB), the encoded tile (8 KiB).
//
// A trimmed stream (include/vitsmi.h, "trimmed streaming"; the scan: stream_trim.hip.hpp) runs the TRIM instantiations of both
// kernels: the kept range is [start[b], n_b) instead of [0, n_b) - the fades count from start[b], the knots stay row
// positions, what lies in front is outside the limiter's windows and is delivered as silence.  The instantiations without
// TRIM are the kernels as they were, and are what every stream without onsets launches.
//
// stream_carry_kernel writes the other generation of the carry behind a piece: the last K = 2 L samples of
// "old carry | piece", right also where the piece is shorter than the carry (resample_carry_kernel's form).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "delivery.hip.hpp"
#include "limit.hip.hpp"
#include "stream_pack.hip.hpp"
#include "stream_shape.hpp"
#include "workspace.hpp"

namespace vitsmi {

constexpr int kStreamTile = kLimitTile;  // delivered elements of a workgroup of the limited stream pack: the staged range is limit_gain_kernel's

// u of row sample j whose raw value is v, kept sample jf of a kept range of c samples (an untrimmed row: jf = j, c = n_b; a
// trimmed one: jf = j - a_b, c = n_b - a_b): limit_value's operations, with peak := ref (norm) and no level gain.  The knots
// walk by row position, the fades count within the kept range.
__device__ inline float stream_shape_value(float v, bool norm, float ref, float volume, const StreamShapeRow &r, const ShapeKnot *knots,
                                           int32_t j, int32_t jf, int32_t c, LimitKnotWalk &w) {
    if (!w.located) {
        w.kp = shape_knot_locate(knots + r.first, r.n_points, j);
        w.kn = knots[r.first + w.kp];
        w.located = true;
    }
    while (j >= w.kn.next) w.kn = knots[r.first + ++w.kp];  // (the last knot's next is INT_MAX: kp stays <= n_points)
    const float mul = shape_combine(shape_knot_env(w.kn, j), shape_w_in(jf, r.fade_in, r.curve), shape_w_out(jf, c, r.fade_out, r.curve));
    if (norm) v = ref < 1e-8f ? 0.f : v / ref;
    if (volume != 1.0f) v = v * volume;
    return shape_mul(v, mul);
}

// a row's sample count n_b, as stream_pack_kernel reads it
__device__ inline int stream_row_count(const StreamPackRows &rows, int b) {
    int64_t nb = rows.len ? (int64_t)rows.len[b] * rows.mul : rows.all;
    nb = nb > rows.all ? rows.all : nb;
    return nb < 0 ? 0 : (int)nb;
}

// stream_pack_kernel's arguments and the rows' records and knots.  TRIM (a trimmed stream, "trimmed streaming"): the kept range
// of row b is [start[b], n_b) - kStreamNoStart while the onset is unknown: nothing of the row is kept yet - and every element
// in front of it is silence; the running peak still folds every valid sample.  Without TRIM `start` is not read.
template <int ENC, bool TRIM>
__global__ __launch_bounds__(kDeliveryThreads) void stream_pack_shaped_kernel(const float *x, int64_t x_pitch, StreamPackRows rows, int first,
                                                                              int n, const float *fmt, int norm, uint4 *bytes,
                                                                              int cells_per_row, unsigned *peak_run,
                                                                              const StreamShapeRow *srows, const ShapeKnot *knots,
                                                                              const int32_t *start) {
    using T = typename DeliveryElem<ENC>::type;
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ uint4 tile[kDeliveryThreads];
    T *lt = reinterpret_cast<T *>(tile);
    const int b = blockIdx.y;
    const int nb = stream_row_count(rows, b);
    const int64_t vl = (int64_t)nb - first;
    const int valid = vl < 0 ? 0 : (vl > n ? n : (int)vl);
    const float ref = fmt[2 * b], volume = fmt[2 * b + 1];
    const float *xr = x + (int64_t)b * x_pitch;
    const StreamShapeRow sr = srows[b];
    const int ab = TRIM ? start[b] : 0;
    LimitKnotWalk walk;
    const T silence = delivery_encode<ENC>(delivery_value(0.0f, false, 1.0f, 1.0f));
    const int base = blockIdx.x * (kDeliveryThreads * E);
    float m = 0.f;
    for (int i = 0; i < E; i++) {
        const int e = base + i * kDeliveryThreads + (int)threadIdx.x;
        T o = silence;
        if (e < valid) {
            const float v = xr[e];
            m = fmaxf(m, fabsf(v));
            if (!TRIM || first + e >= ab) {
                const float u = stream_shape_value(v, norm != 0, ref, volume, sr, knots, first + e, first + e - ab, nb - ab, walk);
                o = delivery_encode<ENC>(fminf(fmaxf(u, -1.0f), 1.0f));
            }
        }
        lt[i * kDeliveryThreads + threadIdx.x] = o;
    }
    __syncthreads();
    const int cell = blockIdx.x * kDeliveryThreads + (int)threadIdx.x;
    if (cell < cells_per_row) bytes[(int64_t)b * cells_per_row + cell] = tile[threadIdx.x];
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(&peak_run[b], __float_as_uint(m));
}

// the piece x [B][n] at `first`, the delivered range [e0, e0 + en), the carry [B][2 L] in front of the piece
struct StreamLimitArgs {
    const float *x;
    int64_t x_pitch;
    int first, n;
    int e0, en;
    int fold_from;
    int L;
    const float *carry;
};

// TRIM: as in stream_pack_shaped_kernel - a staged sample in front of start[b] is outside the kept range (q = 65536, the
// delivery's "a segment never sees the rest of its row") and a delivered one is silence
template <int ENC, bool TRIM>
__global__ __launch_bounds__(kDeliveryThreads) void stream_pack_limited_kernel(StreamLimitArgs a, StreamPackRows rows, const float *fmt, int norm,
                                                                               uint4 *bytes, int cells_per_row, unsigned *peak_run,
                                                                               const StreamShapeRow *srows, const ShapeKnot *knots,
                                                                               const int32_t *start) {
    using T = typename DeliveryElem<ENC>::type;
    constexpr int E = 16 / (int)sizeof(T);
    constexpr int kCells = kStreamTile / E;  // 16-byte cells of a tile
    __shared__ int32_t buf[2][kLimitStage];
    __shared__ int32_t wave_sum[kDeliveryThreads / 64];
    __shared__ float us[kStreamTile];
    __shared__ uint4 cells[kStreamTile * sizeof(float) / 16];
    T *lt = reinterpret_cast<T *>(cells);
    const int lane = threadIdx.x;
    const int b = blockIdx.y;
    const int nb = stream_row_count(rows, b);
    const float ref = fmt[2 * b], volume = fmt[2 * b + 1];
    const float *xr = a.x + (int64_t)b * a.x_pitch;
    const float *cr = a.carry + (int64_t)b * 2 * a.L;
    const StreamShapeRow sr = srows[b];
    const bool limited = sr.ceiling > 0.f;
    const int ab = TRIM ? start[b] : 0;
    const int L = a.L;
    // the tile: delivered elements [d0, d0 + nt) of the row (everything here but `lane` is uniform over the workgroup)
    const int off = blockIdx.x * kStreamTile;
    const int d0 = a.e0 + off;
    const int nt = a.en - off < kStreamTile ? a.en - off : kStreamTile;  // >= 1: the grid covers the cells of en elements
    const int nq = nt + 2 * L;                                           // staged: j = d0 - L + t, t < nq
    LimitKnotWalk walk;
    bool ducks = false;  // some staged sample of this lane is above the ceiling
    float m = 0.f;
    for (int t = lane; t < nq; t += kDeliveryThreads) {
        const int j = d0 - L + t;
        int32_t q = kLimitUnity;
        float u = 0.f;
        const int r = j - a.first;  // the sample's place in the piece; in front of it: in the carry, 2 L + r
        if (j >= 0 && j < nb && r >= -2 * L && r < a.n) {
            const float v = r < 0 ? cr[2 * L + r] : xr[r];
            if (j >= a.fold_from) m = fmaxf(m, fabsf(v));
            if (!TRIM || j >= ab) {
                u = stream_shape_value(v, norm != 0, ref, volume, sr, knots, j, j - ab, nb - ab, walk);
                if (limited) q = limit_q(u, sr.ceiling);
            }
        }
        buf[0][t] = q;
        if (t >= L && t < L + nt) us[t - L] = u;
        ducks = ducks || q < kLimitUnity;
    }
    // (the barrier's answer is the workgroup's: uniform.)  Nothing above the ceiling within L of the tile: every M is 65536,
    // S = (L + 1) * 65536 and g = S / S = 1.0f - the rule's own value, without the passes
    const bool pass = __syncthreads_or(ducks);
    const int32_t *M = nullptr;
    if (pass) M = limit_window_sums(buf, wave_sum, nt, L);
    const T silence = delivery_encode<ENC>(delivery_value(0.0f, false, 1.0f, 1.0f));
    for (int i = lane; i < kStreamTile; i += kDeliveryThreads) {
        T o = silence;
        if (i < nt && d0 + i < nb && (!TRIM || d0 + i >= ab)) {
            float v = us[i];
            if (limited) v = limit_apply(v, pass ? limit_g(M[i + L + 1] - M[i], L) : 1.0f, sr.ceiling);
            o = delivery_encode<ENC>(fminf(fmaxf(v, -1.0f), 1.0f));
        }
        lt[i] = o;
    }
    __syncthreads();
    for (int c = lane; c < kCells; c += kDeliveryThreads) {
        const int cell = blockIdx.x * kCells + c;
        if (cell < cells_per_row) bytes[(int64_t)b * cells_per_row + cell] = cells[c];
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((lane & 63) == 0 && m > 0.f) atomicMax(&peak_run[b], __float_as_uint(m));  // non-negative floats order as uints
}

// the carry behind a piece of x_n samples: the last K samples of "old carry | piece" (unmasked: readers mask by position)
__global__ void stream_carry_kernel(const float *old, const float *x, int64_t x_pitch, int x_n, int K, float *nw) {
    const int b = blockIdx.y, q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= K) return;
    const int64_t r = (int64_t)x_n - K + q;  // position relative to the piece's first sample
    nw[(int64_t)b * K + q] = r >= 0 ? x[(int64_t)b * x_pitch + r] : old[(int64_t)b * K + r + K];
}

// one chunk on `st`, L = 0: launch_stream_pack with the rows' records and knots
inline hipError_t launch_stream_pack_shaped(int encoding, const float *x, int64_t x_pitch, const StreamPackRows &rows, int B, int first, int n,
                                            const float *fmt, bool norm, void *bytes, unsigned *peak_run, const StreamShapeRow *srows,
                                            const ShapeKnot *knots, const int32_t *start, hipStream_t st) {
    const int width = delivery_width(encoding);
    const int cells = (int)(stream_pack_pitch(width, n) / 16);
    const dim3 grid((unsigned)((cells + kDeliveryThreads - 1) / kDeliveryThreads), (unsigned)B);
    uint4 *out = static_cast<uint4 *>(bytes);
    const int nm = norm ? 1 : 0;
    stream_for_encoding(encoding, [&](auto enc) {
        if (start)
            stream_pack_shaped_kernel<decltype(enc)::value, true><<<grid, kDeliveryThreads, 0, st>>>(x, x_pitch, rows, first, n, fmt, nm, out, cells,
                                                                                                     peak_run, srows, knots, start);
        else
            stream_pack_shaped_kernel<decltype(enc)::value, false><<<grid, kDeliveryThreads, 0, st>>>(x, x_pitch, rows, first, n, fmt, nm, out, cells,
                                                                                                      peak_run, srows, knots, nullptr);
    });
    return hipGetLastError();
}

// one chunk on `st`, L > 0: bytes [B][pitch] of the delivered range, pitch = stream_pack_pitch(width, a.en); a.en >= 1
inline hipError_t launch_stream_pack_limited(int encoding, const StreamLimitArgs &a, const StreamPackRows &rows, int B, const float *fmt, bool norm,
                                             void *bytes, unsigned *peak_run, const StreamShapeRow *srows, const ShapeKnot *knots,
                                             const int32_t *start, hipStream_t st) {
    const int width = delivery_width(encoding);
    const int cells = (int)(stream_pack_pitch(width, a.en) / 16);
    const dim3 grid((unsigned)((a.en + kStreamTile - 1) / kStreamTile), (unsigned)B);
    uint4 *out = static_cast<uint4 *>(bytes);
    const int nm = norm ? 1 : 0;
    stream_for_encoding(encoding, [&](auto enc) {
        if (start)
            stream_pack_limited_kernel<decltype(enc)::value, true><<<grid, kDeliveryThreads, 0, st>>>(a, rows, fmt, nm, out, cells, peak_run, srows,
                                                                                                      knots, start);
        else
            stream_pack_limited_kernel<decltype(enc)::value, false><<<grid, kDeliveryThreads, 0, st>>>(a, rows, fmt, nm, out, cells, peak_run, srows,
                                                                                                       knots, nullptr);
    });
    return hipGetLastError();
}

// the carry behind the piece x [B][x_n]: generation `nw` from generation `old`
inline hipError_t launch_stream_carry(const float *old, const float *x, int64_t x_pitch, int x_n, int L, int B, float *nw, hipStream_t st) {
    stream_carry_kernel<<<dim3((unsigned)((2 * L + 255) / 256), (unsigned)B), 256, 0, st>>>(old, x, x_pitch, x_n, 2 * L, nw);
    return hipGetLastError();
}

// ---- a shaped stream from its first chunk to its last: the shaped form of the pack stage (stream_run.hip.hpp,
// stream_pack_begin / stream_pack_piece), which the pipeline and the test hooks run

// the state of one run.  The vectors are the pageable sources of copies: they outlive the run's waits.
struct StreamShapeRun {
    int L = 0;
    StreamShapeBufs ss{};
    int gen = 0;            // the carry generation in front of the next piece
    int64_t fold_from = 0;  // the first rendered sample the running peak has not seen
    std::vector<StreamShapeRow> rows;
    std::vector<ShapeKnot> knots;
};

// records and knots up, the carry zeroed; the shaping has passed stream_shape_fault, ss is carve_stream_shape's for its L and
// stream_knot_count
inline hipError_t stream_shape_begin(StreamShapeRun &r, const vits_stream_shaping *s, int B, const StreamShapeBufs &ss, hipStream_t st) {
    r.L = s->lookahead;
    r.ss = ss;
    r.gen = 0;
    r.fold_from = 0;
    stream_shape_table(s, B, r.rows, r.knots);
    hipError_t e = hipMemcpyAsync(ss.rows, r.rows.data(), r.rows.size() * sizeof(StreamShapeRow), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ss.knots, r.knots.data(), r.knots.size() * sizeof(ShapeKnot), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && r.L > 0) e = hipMemsetAsync(ss.carry[0], 0, (size_t)B * 2 * r.L * sizeof(float), st);
    return e;
}

// The rendered piece x [B][n] at `first` of rows of `total` samples: what it delivers - [e_first, e_first + e_n), encoded at
// d = sp.at(B, pitch of e_n) with the running peaks behind - and the carry for the next piece.  e_n == 0: nothing was
// delivered (d is not set).  launches receives the number of launches made.
inline hipError_t stream_shape_chunk(StreamShapeRun &r, int encoding, int width, const float *x, int64_t x_pitch, const StreamPackRows &rows,
                                     int B, int64_t first, int64_t n, int64_t total, const StreamPackBufs &sp, bool norm, hipStream_t st,
                                     int64_t &e_first, int64_t &e_n, unsigned char *&d, int &launches) {
    const bool is_last = first + n >= total;
    stream_emit_range(first, n, is_last, total, r.L, e_first, e_n);
    hipError_t e = hipSuccess;
    launches = 0;
    if (e_n > 0) {
        d = sp.at(B, StreamPackBufs::pitch(width, e_n));
        if (r.L == 0)
            e = launch_stream_pack_shaped(encoding, x, x_pitch, rows, B, (int)first, (int)n, sp.fmt, norm, d, sp.peak_run, r.ss.rows,
                                          r.ss.knots, sp.start, st);
        else {
            const StreamLimitArgs a{x, x_pitch, (int)first, (int)n, (int)e_first, (int)e_n, (int)r.fold_from, r.L, r.ss.carry[r.gen]};
            e = launch_stream_pack_limited(encoding, a, rows, B, sp.fmt, norm, d, sp.peak_run, r.ss.rows, r.ss.knots, sp.start, st);
            r.fold_from = first + n;
        }
        launches++;
    }
    if (e == hipSuccess && r.L > 0 && !is_last) {
        e = launch_stream_carry(r.ss.carry[r.gen], x, x_pitch, (int)n, r.L, B, r.ss.carry[r.gen ^ 1], st);
        r.gen ^= 1;
        launches++;
    }
    return e;
}

}  // namespace vitsmi
