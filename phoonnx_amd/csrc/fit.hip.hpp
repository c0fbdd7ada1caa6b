// fit.hip.hpp — fitted durations on the device (include/vitsmi.h, "fitted durations"; arithmetic and search: fit.hpp).
//
// fit_weight_kernel writes w[b][t], the fp32 value duration_kernel hands to ceilf, through the one function both call
// (duration_weight, kernels.hip.hpp).  fit_duration_kernel then takes one workgroup of four waves per group: it keeps the
// group's cleaned weights in LDS (the first kFitCache of them; a longer group reads the rest from memory at every count),
// runs fit.hpp's search with a count that is an int64 sum over the workgroup - a cross-lane reduction per wave, the four
// wave sums through LDS, one barrier per count -, and walks the group's rows once more in (b, t) order, 256 tokens a pass:
// a prefix count over the candidates decides who takes one of the R remaining frames, an integer scan gives cum.  Every
// sum is an integer sum, so no order the hardware chooses can show; all stores are plain vector stores.  Rows of other
// groups, and rows of no group, are neither read nor written.
#pragma once
#include <hip/hip_runtime.h>

#include "fit.hpp"
#include "kernels.hip.hpp"

namespace vitsmi {

constexpr int kFitCache = 8192;  // cleaned weights of a group kept in LDS (32 KiB)

// w[b][t] = duration_kernel's ceilf argument (0 behind len[b]); grid (ceil(T / 256), B)
__global__ __launch_bounds__(256) void fit_weight_kernel(const float *logw, const int *len, float length_scale_all, const float *rows,
                                                         const float *token_rate, float *w, int T) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t i = (int64_t)b * T + t;
    w[i] = duration_weight(logw, token_rate, i, t < len[b], row_setting(rows, b, 1, length_scale_all));
}

// the group's frame count at a multiplier: the same value in every thread of the workgroup
struct FitCount {
    const float *w, *cache;
    const int *len, *group;
    long long *red;  // [2][4]: the wave sums, two sets in turn so that a count needs one barrier
    int B, T, g, n, tid;
    int parity;
    __device__ int64_t operator()(uint64_t bits) {
        const double s = fit_scale(bits);
        long long acc = 0;
        const int nc = n < kFitCache ? n : kFitCache;
#pragma unroll 8
        for (int i = tid; i < nc; i += 256) acc += fit_term(cache[i], s);  // (unrolled: the LDS reads of eight terms in flight)
        if (n > kFitCache) {  // the tokens behind the cached ones, from memory
            int off = 0;
            for (int b = 0; b < B; b++) {
                if (group[b] != g) continue;
                const int L = len[b];
                if (off + L > kFitCache)
                    for (int t = tid; t < L; t += 256)
                        if (off + t >= kFitCache) acc += fit_term(fit_clean(w[(int64_t)b * T + t]), s);
                off += L;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        long long *r = red + parity * 4;
        parity ^= 1;
        if ((tid & 63) == 0) r[tid >> 6] = acc;
        __syncthreads();
        return (int64_t)(r[0] + r[1] + r[2] + r[3]);
    }
};

// One workgroup per group g = blockIdx.x.  w [B][T] fp32, len [B] in [0, T], group [B] in [-1, G), target / mode [G]
// (validated on the host).  Writes w_ceil, cum (all t < T) and y_len of the group's rows, and res[g].
__global__ __launch_bounds__(256) void fit_duration_kernel(const float *w, const int *len, const int *group, const int64_t *target,
                                                           const int *mode, int B, int T, float *w_ceil, int *cum, int *y_len,
                                                           FitResult *res) {
    __shared__ float cache[kFitCache];
    __shared__ long long red[8];
    __shared__ int cand_sum[4], dur_sum[4];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the group's cleaned weights, (b, t) ascending
    int n = 0;
    for (int b = 0; b < B; b++) {
        if (group[b] != g) continue;
        const int L = len[b];
        for (int t = tid; t < L; t += 256)
            if (n + t < kFitCache) cache[n + t] = fit_clean(w[(int64_t)b * T + t]);
        n += L;
    }
    __syncthreads();
    FitCount count{w, cache, len, group, red, B, T, g, n, tid, 0};
    const int64_t F = target[g];
    uint64_t bits;
    int64_t cnt;
    int32_t status;
    fit_search(count, F, mode[g], bits, cnt, status);
    const double s = fit_scale(bits), s_next = fit_scale(bits + 1);
    const int64_t R = status == VITS_FIT_MET ? F - cnt : 0;
    // the durations: ceil(w s*), one more for the first R candidates; cum and y_len per row
    int64_t handed = 0, frames = 0;  // candidates seen, frames written: the same in every thread
    int off = 0;
    for (int b = 0; b < B; b++) {
        if (group[b] != g) continue;
        const int L = len[b];
        int carry = 0;
        for (int base = 0; base < T; base += 256) {
            const int t = base + tid;
            const bool in = t < L;
            int d = 0;
            bool cand = false;
            if (in) {
                const int i = off + t;
                const float wc = i < kFitCache ? cache[i] : fit_clean(w[(int64_t)b * T + t]);
                d = (int)fit_term(wc, s);
                cand = R > 0 && fit_term(wc, s_next) > (int64_t)d;
            }
            const unsigned long long m = __ballot(cand);
            if (lane == 0) cand_sum[wv] = __popcll(m);
            __syncthreads();
            int64_t before = handed + __popcll(m & ((1ull << lane) - 1ull));
            int total_c = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = cand_sum[k];
                before += k < wv ? c : 0;
                total_c += c;
            }
            if (cand && before < R) d++;
            handed += total_c;
            int sc = d;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(sc, o, 64);
                if (lane >= o) sc += v;
            }
            if (lane == 63) dur_sum[wv] = sc;
            __syncthreads();
            int pre = carry, total = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int v = dur_sum[k];
                pre += k < wv ? v : 0;
                total += v;
            }
            if (t < T) {
                w_ceil[(int64_t)b * T + t] = (float)d;
                cum[(int64_t)b * T + t] = pre + sc;
            }
            carry += total;
        }
        if (tid == 0) y_len[b] = carry < 1 ? 1 : carry;
        frames += carry;
        off += L;
    }
    if (tid == 0) {
        FitResult r;
        r.scale = s;
        r.frames = frames;
        r.status = status;
        r.pad_ = 0;
        res[g] = r;
    }
}

}  // namespace vitsmi
