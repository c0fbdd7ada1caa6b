// stream_trim.hip.hpp — the scan of a trimmed encoded stream (include/vitsmi.h, "trimmed streaming"; the rule and the records:
// stream_shape.hpp).
//
// stream_onset_kernel runs per rendered piece, in front of the pack launch (stream_run.hip.hpp, stream_pack_piece) - also for a
// piece that completes nothing: its samples are rendered all the same.  Grid (B), ONE workgroup per row, so that "the row's
// start is known" is read and written by the same workgroup and never races with another one.  For a trimmed row whose start
// is unknown it finds the smallest index i in [first, first + n) ∩ [0, n_b) with |x[b][i]| > thr - the comparison is strict
// and on the raw sample - and writes a_b = max(i - keep_lead, D) once, D the first sample the piece delivers.  A row that is
// not trimmed has start 0 from the upload on; a row whose start is known returns at once.
// The workgroup walks the piece in windows of kOnsetWindow samples (4096) in ascending order; a lane's indices within a window
// ascend, so its first hit is its smallest, and the window that holds a hit ends the walk (a barrier's answer: uniform).  The
// minimum over the lanes is an integer minimum through shuffles and LDS: order-independent, no atomics at all.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "stream_shape.hip.hpp"
#include "stream_shape.hpp"

namespace vitsmi {

constexpr int kOnsetThreads = 256;
constexpr int kOnsetLoads = 16;  // samples of a window per lane
constexpr int kOnsetWindow = kOnsetLoads * kOnsetThreads;

__global__ __launch_bounds__(kOnsetThreads) void stream_onset_kernel(const float *x, int64_t x_pitch, StreamPackRows rows, int first, int n,
                                                                      int D, const StreamOnsetRow *onsets, int32_t *start) {
    __shared__ int wave_min[kOnsetThreads / 64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const StreamOnsetRow o = onsets[b];
    if (!o.on || start[b] != kStreamNoStart) return;  // (uniform over the workgroup; nobody else writes start[b])
    const int nb = stream_row_count(rows, b);
    const int64_t vl = (int64_t)nb - first;
    const int valid = vl < 0 ? 0 : (vl > n ? n : (int)vl);  // the piece's samples of this row: r < valid <= n
    const float *xr = x + (int64_t)b * x_pitch;
    int f = INT_MAX;
    for (int base = 0; base < valid; base += kOnsetWindow) {
        float v[kOnsetLoads];  // a window's loads are issued together; behind the row's samples of the piece: 0, never active (thr >= 0)
#pragma unroll
        for (int k = 0; k < kOnsetLoads; k++) {
            const int r = base + k * kOnsetThreads + lane;
            v[k] = r < valid ? xr[r] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kOnsetLoads; k++)
            if (f == INT_MAX && fabsf(v[k]) > o.thr) f = base + k * kOnsetThreads + lane;
        if (__syncthreads_or(f != INT_MAX)) break;
    }
    for (int s = 32; s > 0; s >>= 1) {
        const int other = __shfl_xor(f, s);
        f = other < f ? other : f;
    }
    if ((lane & 63) == 0) wave_min[lane >> 6] = f;
    __syncthreads();
    if (lane == 0) {
        for (int w = 1; w < kOnsetThreads / 64; w++) f = wave_min[w] < f ? wave_min[w] : f;
        if (f != INT_MAX) {
            const int a = first + f - o.keep_lead;  // (first + f < n_b <= INT_MAX, keep_lead >= 0: no overflow)
            start[b] = a > D ? a : D;
        }
    }
}

// the scan of the piece x [B][n] at `first`, which delivers from D on
inline hipError_t launch_stream_onset(const float *x, int64_t x_pitch, const StreamPackRows &rows, int B, int first, int n, int D,
                                      const StreamOnsetRow *onsets, int32_t *start, hipStream_t st) {
    stream_onset_kernel<<<dim3((unsigned)B), kOnsetThreads, 0, st>>>(x, x_pitch, rows, first, n, D, onsets, start);
    return hipGetLastError();
}

}  // namespace vitsmi
