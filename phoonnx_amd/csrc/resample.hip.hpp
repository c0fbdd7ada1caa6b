// resample.hip.hpp — the output-rate resampler on the device (include/vitsmi.h, "Output rate"; plan: resample.hpp).
//
// One workgroup renders a tile of consecutive output samples of one row.  The input span the tile needs - about
// tile * M / L + K floats, each of which is read by K * L / M of the tile's samples - is staged once in LDS, already
// masked to the row's valid samples.  The table is NOT staged: a sample uses its K coefficients once, and the
// tile's samples walk the phases with stride M mod L, so a tile reuses a table row only when it is longer than L.
// Staging would put one LDS write and one LDS read on top of every coefficient's one read from memory; instead each
// lane streams its own row h[p][0..K) with 16-byte loads (rows are padded to whole 16 bytes) through L1 / L2, where the
// table - 65 KB for the largest common pair, 1 MiB at the admitted limit - stays resident ("Output rate").
//
// Three entries, one function for a sample (resample_sample): resample_kernel reads a whole row, resample_piece_kernel
// reads "carry | new piece" - the last K input samples of every row kept between the chunks of a chunked run, then the
// chunk -, resample_rows_kernel reads a whole row at the row's OWN plan (a rate per row).  All accumulate in fp32 with fmaf in ascending j from 0.0f, so a sample has the same bits whichever entry,
// tile or input path (LDS, or straight from memory where the span does not fit) rendered it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample.hpp"

namespace vitsmi {

constexpr int kResampleBlock = 256;         // output samples (= threads) per workgroup; 64 where that span does not fit
constexpr int kResampleLdsFloats = 16000;   // the span a workgroup may stage (64 000 bytes)

struct ResampleArgs {
    const float *table;  // h[p][j] at table[p * Kp + j]
    int Kp, K;
    int64_t L, M;
    const float *x;      // input samples [x_first, x_first + x_n) of row b at x + b * x_pitch
    int64_t x_pitch;
    int x_first, x_n;
    const float *carry;  // piece entry: input samples [x_first - K, x_first) of row b at carry + b * K
    const int *n_in;     // [B] valid input samples of a row: what lies behind reads 0
    const int *n_out;    // [B] its output samples: what lies behind is written as 0
    float *y;            // output sample n of row b goes to y[b * y_pitch + n - y_first]
    int64_t y_pitch;
    int y_first;
    int n_lo, n_hi;      // the output samples this launch renders
    int span;            // LDS floats per workgroup; 0: the input is read through L1 / L2
};

// input sample m of row b: 0 in front of the row, behind its valid samples and outside what the launch was given
template <bool kCarry>
__device__ __forceinline__ float resample_input(const ResampleArgs &a, int b, int n_valid, int64_t m) {
    if (m < 0 || m >= n_valid) return 0.f;
    const int64_t q = m - a.x_first;
    if (q >= 0) return q < a.x_n ? a.x[(int64_t)b * a.x_pitch + q] : 0.f;
    if (kCarry && q >= -(int64_t)a.K) return a.carry[(int64_t)b * a.K + q + a.K];
    return 0.f;
}

// THE output sample: sum_j h[p][j] * x[m0 + j], fp32, fmaf in ascending j from 0.0f.  hrow is 16-byte aligned.
template <class X>
__device__ __forceinline__ float resample_sample(const float *hrow, int K, X x) {
    float acc = 0.f;
    int j = 0;
    for (; j + 4 <= K; j += 4) {
        const float4 hv = *reinterpret_cast<const float4 *>(hrow + j);
        acc = fmaf(hv.x, x(j), acc);
        acc = fmaf(hv.y, x(j + 1), acc);
        acc = fmaf(hv.z, x(j + 2), acc);
        acc = fmaf(hv.w, x(j + 3), acc);
    }
    for (; j < K; j++) acc = fmaf(hrow[j], x(j), acc);
    return acc;
}

template <bool kCarry>
__device__ __forceinline__ void resample_tile(const ResampleArgs &a) {
    extern __shared__ float xs[];
    const int b = blockIdx.y;
    const int64_t n0 = (int64_t)a.n_lo + (int64_t)blockIdx.x * blockDim.x;
    const int64_t n_end = n0 + blockDim.x < a.n_hi ? n0 + blockDim.x : a.n_hi;
    const int n_valid = a.n_in[b];
    const int64_t N = a.n_out[b];
    const int half = a.K / 2;
    const int64_t i0 = n0 * a.M / a.L;
    if (a.span && n0 < N) {  // (a tile behind the row's end writes zeros: nothing to stage)
        const int64_t i_last = ((n_end < N ? n_end : N) - 1) * a.M / a.L;
        const int len = (int)(i_last - i0) + a.K;  // <= span: consecutive tile samples advance by at most ceil(M / L)
        const int64_t m_base = i0 - half + 1;
        for (int q = threadIdx.x; q < len; q += blockDim.x) xs[q] = resample_input<kCarry>(a, b, n_valid, m_base + q);
    }
    __syncthreads();
    const int64_t n = n0 + threadIdx.x;
    if (n >= n_end) return;
    float v = 0.f;
    if (n < N) {
        const int64_t t = n * a.M, i = t / a.L, p = t - i * a.L;
        const float *hrow = a.table + p * a.Kp;
        if (a.span) {
            const float *w = xs + (i - i0);
            v = resample_sample(hrow, a.K, [&](int j) { return w[j]; });
        } else {
            const int64_t m0 = i - half + 1;
            v = resample_sample(hrow, a.K, [&](int j) { return resample_input<kCarry>(a, b, n_valid, m0 + j); });
        }
    }
    a.y[(int64_t)b * a.y_pitch + (n - a.y_first)] = v;
}

// a whole row in, its resampled row out
__global__ void __launch_bounds__(kResampleBlock) resample_kernel(ResampleArgs a) { resample_tile<false>(a); }
// chunked rendering: "carry | new piece" in, the output samples that piece completes out
__global__ void __launch_bounds__(kResampleBlock) resample_piece_kernel(ResampleArgs a) { resample_tile<true>(a); }

// valid input samples and output samples per row: ylen[b] * hop (no frame counts: n_all) and ceil(n * L / M)
__global__ void resample_counts_kernel(const int *ylen, int hop, int n_all, int64_t L, int64_t M, int *n_in, int *n_out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t n = ylen ? (int64_t)ylen[b] * hop : n_all;
    n = n < 0 ? 0 : (n > n_all ? n_all : n);
    n_in[b] = (int)n;
    n_out[b] = (int)((n * L + M - 1) / M);
}

// ---- a rate per row (include/vitsmi.h, "Output rate per row"): every row of one launch has a plan record of its own
//
// resample_rows_kernel is resample_kernel with the plan looked up by row: the workgroup reads its row's record, fills the
// ResampleArgs a single-rate launch would have been given and runs resample_tile - so row b of a mixed launch is row b of
// a launch at its rate alone, bit for bit, by construction.  A native row (no table) is a masked copy; a tile wholly behind
// its row's end writes zeros and stages nothing.  Everything in front of resample_tile's __syncthreads is uniform over the
// workgroup: it depends on blockIdx and on values indexed by it alone.
struct ResampleRowPlan {
    const float *table;  // nullptr: a native row, y = x
    int Kp, K;
    int64_t L, M;        // (a native row: 1, 1)
    int span;            // LDS floats a tile of kResampleBlock samples stages; 0: read through L1 / L2
};

struct ResampleRowsArgs {
    const ResampleRowPlan *plans;  // [B], on the device
    const float *x;                // input samples [0, x_n) of row b at x + b * x_pitch
    int64_t x_pitch;
    int x_n;
    const int *n_in, *n_out;       // [B], as in ResampleArgs
    float *y;                      // [B][y_pitch]
    int64_t y_pitch;
    int n_hi;                      // S_out: the launch renders output samples [0, n_hi) of every row
};

__global__ void __launch_bounds__(kResampleBlock) resample_rows_kernel(ResampleRowsArgs r) {
    const int b = blockIdx.y;
    const ResampleRowPlan p = r.plans[b];
    const int64_t n0 = (int64_t)blockIdx.x * blockDim.x, n = n0 + threadIdx.x;
    const int64_t N = r.n_out[b];
    if (n0 >= N || !p.table) {  // behind the row's end: zeros; a native row: its valid samples, zeros behind them
        if (n < r.n_hi) r.y[(int64_t)b * r.y_pitch + n] = n < N ? r.x[(int64_t)b * r.x_pitch + n] : 0.f;
        return;
    }
    ResampleArgs a{};
    a.table = p.table;
    a.Kp = p.Kp;
    a.K = p.K;
    a.L = p.L;
    a.M = p.M;
    a.x = r.x;
    a.x_pitch = r.x_pitch;
    a.x_n = r.x_n;
    a.n_in = r.n_in;
    a.n_out = r.n_out;
    a.y = r.y;
    a.y_pitch = r.y_pitch;
    a.n_hi = r.n_hi;
    a.span = p.span;
    resample_tile<false>(a);
}

// resample_counts_kernel with every row's own L and M (a native row: n_out = n_in)
__global__ void resample_rows_counts_kernel(const int *ylen, int hop, int n_all, const ResampleRowPlan *plans, int *n_in, int *n_out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t n = ylen ? (int64_t)ylen[b] * hop : n_all;
    n = n < 0 ? 0 : (n > n_all ? n_all : n);
    n_in[b] = (int)n;
    n_out[b] = (int)((n * plans[b].L + plans[b].M - 1) / plans[b].M);
}

// the carry behind a piece of x_n samples: the last K samples of "old carry | piece" (unmasked: readers mask by position)
__global__ void resample_carry_kernel(const float *old, const float *x, int64_t x_pitch, int x_n, int K, float *nw) {
    const int b = blockIdx.y, q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= K) return;
    const int64_t r = (int64_t)x_n - K + q;  // position relative to the piece's first sample
    nw[(int64_t)b * K + q] = r >= 0 ? x[(int64_t)b * x_pitch + r] : old[(int64_t)b * K + r + K];
}

// the table of a plan on the device: rows padded to whole 16 bytes
struct ResampleDev {
    ResamplePlan plan;
    float *table = nullptr;
    int Kp = 0;
};

inline int resample_pitch(const ResamplePlan &p) { return (int)((p.K + 3) & ~int64_t(3)); }

// launch either entry over output samples [a.n_lo, a.n_hi) of B rows; everything but span is the caller's
inline hipError_t launch_resample(ResampleArgs a, int B, bool piece, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo) return hipSuccess;
    int block = kResampleBlock;
    auto span_of = [&](int tile) { return (int64_t)(tile - 1) * a.M / a.L + 2 + a.K; };
    int64_t span = span_of(block);
    if (span > kResampleLdsFloats) {
        block = 64;
        span = span_of(block);
    }
    if (span > kResampleLdsFloats) span = 0;
    a.span = (int)span;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + block - 1) / block), (unsigned)B);
    if (piece) resample_piece_kernel<<<grid, block, (size_t)span * sizeof(float), st>>>(a);
    else resample_kernel<<<grid, block, (size_t)span * sizeof(float), st>>>(a);
    return hipGetLastError();
}

// The record of a row at plan d (nullptr: a native row).  The block size is uniform over a rows launch, so a plan whose
// kResampleBlock-sample span exceeds what a workgroup may stage is read unstaged: it does not shrink the block.
inline ResampleRowPlan resample_row_plan(const ResampleDev *d) {
    ResampleRowPlan r{nullptr, 0, 0, 1, 1, 0};
    if (!d) return r;
    r.table = d->table;
    r.Kp = d->Kp;
    r.K = (int)d->plan.K;
    r.L = d->plan.L;
    r.M = d->plan.M;
    const int64_t span = (int64_t)(kResampleBlock - 1) * r.M / r.L + 2 + r.K;
    r.span = span > kResampleLdsFloats ? 0 : (int)span;
    return r;
}

// launch the rows entry over output samples [0, r.n_hi) of B rows; lds_floats: the largest span among the rows' records
inline hipError_t launch_resample_rows(const ResampleRowsArgs &r, int B, int lds_floats, hipStream_t st) {
    if (B <= 0 || r.n_hi <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)r.n_hi + kResampleBlock - 1) / kResampleBlock), (unsigned)B);
    resample_rows_kernel<<<grid, kResampleBlock, (size_t)lds_floats * sizeof(float), st>>>(r);
    return hipGetLastError();
}

inline ResampleArgs resample_args(const ResampleDev &d) {
    ResampleArgs a{};
    a.table = d.table;
    a.Kp = d.Kp;
    a.K = (int)d.plan.K;
    a.L = d.plan.L;
    a.M = d.plan.M;
    return a;
}

}  // namespace vitsmi
