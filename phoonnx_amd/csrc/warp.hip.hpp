// warp.hip.hpp — the per-token time warp on the device (include/vitsmi.h, "Intonation"; plan: warp.hpp).
//
// One workgroup renders kWarpBlock consecutive output samples of one row.  Input positions never decrease along a row and
// advance by at most two samples per output, so the tile reads at most 255 * 2 + 2 + 76 input floats: they are staged once
// in LDS, already masked to the row's valid samples.  The workgroup finds the segments of its first and of its last sample
// by binary search over the row's n0 - both uniform - and every lane walks forward from the first to its own: a tile may
// straddle many short segments.  The prototype table G (32 KB) is staged in LDS too: a wave's 64 lanes read 64 different
// table lines per tap (neighbouring outputs lie some 435 entries apart in G), which LDS serves at full rate and L1 does not
// - 245 us against 375 us for the launch of a 32-row batch, measured with both placements.
//
// One function renders a sample (warp_sample): fp32, fmaf in ascending m from 0.0f, so a sample has the same bits
// whichever tile or batch rendered it.  Everything in front of the barrier is uniform over the workgroup:
// it depends on blockIdx and on values indexed by it alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "resample.hip.hpp"
#include "warp.hpp"

namespace vitsmi {

constexpr int kWarpBlock = 256;                                        // output samples (= threads) per workgroup
constexpr int kWarpSpan = (kWarpBlock - 1) * 2 + 2 + 2 * kWarpMaxHalf;  // the input floats a tile stages at most (588)

template <class Seg>
struct WarpArgsT {
    const Seg *segs;
    const WarpRow *rows;  // [B]
    const float *G;       // [kWarpTable]
    const float *x;       // input samples of row b at x + b * x_pitch
    int64_t x_pitch;
    float *y;             // [B][y_pitch]: row b's output sample n_lo at y + b * y_pitch
    int64_t y_pitch;
    int n_hi;             // the launch renders output samples [n_lo, n_hi) of every row; a whole run: [0, S_w)
    int n_lo;             // a window of a streamed run ("streamed pitch"): tile i covers [n_lo + 256 i, ...), clipped by n_hi
};
using WarpArgs = WarpArgsT<vits_warp_seg>;
using GlideArgs = WarpArgsT<vits_glide_seg>;  // "pitch contours": the same launch over gliding records

// the last segment whose n0 <= n (segments without an output sample share the n0 of the one behind them)
template <class Seg>
__device__ __forceinline__ int warp_find(const Seg *sg, int n_segs, int64_t n) {
    int lo = 0, hi = n_segs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg[mid].n0 <= n) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// THE output sample at input position pos (Q16): taps m = i0 - Kh + 1 .. i0 + Kh, weight G at |m - pos| * c by linear
// interpolation, x(d) = the input at m = i0 + d
template <class X>
__device__ __forceinline__ float warp_sample(const float *G, int64_t pos, int32_t c, int32_t Kh, X x) {
    const int32_t frac = (int32_t)(pos & (kWarpOne - 1));
    float acc = 0.f;
    for (int d = 1 - Kh; d <= Kh; d++) {
        const int32_t t = d * (int32_t)kWarpOne - frac;  // (m << FB) - pos: within +-38 * 2^16
        const uint64_t v = (uint64_t)(uint32_t)(t < 0 ? -t : t) * (uint32_t)c;
        const uint32_t i = (uint32_t)(v >> 23);
        const float f = (float)(uint32_t)(v & 0x7FFFFFu) * 0x1p-23f;
        float w = 0.f;
        if (i < (uint32_t)(kWarpZ * kWarpR)) {
            const float g0 = G[i], g1 = G[i + 1];
            w = fmaf(f, g1 - g0, g0);
        }
        acc = fmaf(w, x(d), acc);
    }
    return ((float)c * 0x1p-16f) * acc;  // (float)(c / 65536.0): c <= 2^16, the scaling is exact
}

__global__ void __launch_bounds__(kWarpBlock) warp_kernel(WarpArgs a) {
    __shared__ float xs[kWarpSpan];
    __shared__ float gs[kWarpTable];
    const int b = blockIdx.y;
    const WarpRow r = a.rows[b];
    const int64_t n0 = a.n_lo + (int64_t)blockIdx.x * kWarpBlock, n = n0 + threadIdx.x;
    const float *xrow = a.x + (int64_t)b * a.x_pitch;
    float *yrow = a.y + (int64_t)b * a.y_pitch - a.n_lo;  // indexed by n
    if (n0 >= r.n_out || r.identity || r.n_segs <= 0) {  // behind the row's end: zeros; an identity row: its valid samples
        if (n < a.n_hi) yrow[n] = (r.identity && n < r.n_out && n < r.n_in) ? xrow[n] : 0.f;
        return;
    }
    const vits_warp_seg *sg = a.segs + r.seg0;
    // the tile's last sample: clipped by the row and by the window, so that nothing behind the window's last position is staged
    const int64_t n_end = n0 + kWarpBlock < a.n_hi ? n0 + kWarpBlock : (int64_t)a.n_hi;
    const int64_t n_last = (n_end < r.n_out ? n_end : (int64_t)r.n_out) - 1;
    const int j0 = warp_find(sg, r.n_segs, n0), j1 = warp_find(sg, r.n_segs, n_last);
    const int64_t i_lo = (sg[j0].pos0 + (n0 - sg[j0].n0) * sg[j0].step) >> kWarpFB;
    const int64_t i_hi = (sg[j1].pos0 + (n_last - sg[j1].n0) * sg[j1].step) >> kWarpFB;
    const int64_t m_base = i_lo - kWarpMaxHalf + 1;
    int64_t len = i_hi - i_lo + 2 * kWarpMaxHalf;
    len = len > kWarpSpan ? kWarpSpan : len;  // (never: positions advance by at most two samples an output)
    for (int q = threadIdx.x; q < (int)len; q += kWarpBlock) {
        const int64_t m = m_base + q;
        xs[q] = m >= 0 && m < r.n_in ? xrow[m] : 0.f;
    }
    for (int q = threadIdx.x; q < kWarpTable; q += kWarpBlock) gs[q] = a.G[q];
    __syncthreads();
    if (n >= a.n_hi) return;
    float v = 0.f;
    if (n < r.n_out) {
        int j = j0;
        while (j < j1 && sg[j + 1].n0 <= n) j++;
        const vits_warp_seg g = sg[j];
        const int64_t pos = g.pos0 + (n - g.n0) * g.step;
        const int64_t at = (pos >> kWarpFB) - m_base;  // the tap m = i0 in the staged span
        if (at - g.half_taps + 1 >= 0 && at + g.half_taps < len) {
            const float *w = xs + at;
            v = warp_sample(gs, pos, g.c, g.half_taps, [&](int d) { return w[d]; });
        }
    }
    yrow[n] = v;
}

// launch over output samples [a.n_lo, a.n_hi) of B rows
inline hipError_t launch_warp(const WarpArgs &a, int B, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo || a.n_lo < 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + kWarpBlock - 1) / kWarpBlock), (unsigned)B);
    warp_kernel<<<grid, kWarpBlock, 0, st>>>(a);
    return hipGetLastError();
}

// ---- pitch contours (include/vitsmi.h, "pitch contours"): warp_kernel's sibling for rows with a gliding token.
//
// Geometry, staging and the copy branch are warp_kernel's.  What differs is per lane behind the barrier: the position and
// the speed of a sample come from the closed forms of the definition (glide_pos, glide_step: warp.hpp), the cutoff and the
// half-taps from the speed (glide_cutoff), then the shared warp_sample.  The divisions are plain unsigned 64-bit divisions
// by k and by 2k, and one by 20s in the cutoff - the compiler's expansion, three a lane: the numerators reach 2^63, so
// neither a 32-bit nor a floating-point reciprocal gives the definition's integers for every input, and against the
// 38..76 taps of a sample the three divisions are a few per cent.  Lanes of one wave now differ in Kh inside a token: the
// tap loop runs to the wave's longest.  The staging bound holds as it is because every increment of the position lies in
// [min(a, b), max(a, b)] <= 2 * ONE, across segment boundaries too (a token starts at the pos_k of the one before it).
__global__ void __launch_bounds__(kWarpBlock) glide_kernel(GlideArgs a) {
    __shared__ float xs[kWarpSpan];
    __shared__ float gs[kWarpTable];
    const int b = blockIdx.y;
    const WarpRow r = a.rows[b];
    const int64_t n0 = a.n_lo + (int64_t)blockIdx.x * kWarpBlock, n = n0 + threadIdx.x;
    const float *xrow = a.x + (int64_t)b * a.x_pitch;
    float *yrow = a.y + (int64_t)b * a.y_pitch - a.n_lo;  // indexed by n
    if (n0 >= r.n_out || r.identity || r.n_segs <= 0) {  // behind the row's end: zeros; an identity row: its valid samples
        if (n < a.n_hi) yrow[n] = (r.identity && n < r.n_out && n < r.n_in) ? xrow[n] : 0.f;
        return;
    }
    const vits_glide_seg *sg = a.segs + r.seg0;
    // the tile's last sample: clipped by the row and by the window, so that nothing behind the window's last position is staged
    const int64_t n_end = n0 + kWarpBlock < a.n_hi ? n0 + kWarpBlock : (int64_t)a.n_hi;
    const int64_t n_last = (n_end < r.n_out ? n_end : (int64_t)r.n_out) - 1;
    const int j0 = warp_find(sg, r.n_segs, n0), j1 = warp_find(sg, r.n_segs, n_last);
    const int64_t i_lo = glide_pos(sg[j0].pos0, sg[j0].k, sg[j0].step0, sg[j0].step1, n0 - sg[j0].n0) >> kWarpFB;
    const int64_t i_hi = glide_pos(sg[j1].pos0, sg[j1].k, sg[j1].step0, sg[j1].step1, n_last - sg[j1].n0) >> kWarpFB;
    const int64_t m_base = i_lo - kWarpMaxHalf + 1;
    int64_t len = i_hi - i_lo + 2 * kWarpMaxHalf;
    len = len > kWarpSpan ? kWarpSpan : len;  // (never: positions advance by at most two samples an output)
    for (int q = threadIdx.x; q < (int)len; q += kWarpBlock) {
        const int64_t m = m_base + q;
        xs[q] = m >= 0 && m < r.n_in ? xrow[m] : 0.f;
    }
    for (int q = threadIdx.x; q < kWarpTable; q += kWarpBlock) gs[q] = a.G[q];
    __syncthreads();
    if (n >= a.n_hi) return;
    float v = 0.f;
    if (n < r.n_out) {
        int j = j0;
        while (j < j1 && sg[j + 1].n0 <= n) j++;
        const vits_glide_seg g = sg[j];
        const int64_t pos = glide_pos(g.pos0, g.k, g.step0, g.step1, n - g.n0);
        int32_t c, Kh;
        glide_cutoff(glide_step(g.k, g.step0, g.step1, n - g.n0), c, Kh);
        const int64_t at = (pos >> kWarpFB) - m_base;  // the tap m = i0 in the staged span
        // Dead code, kept as the fence it is in warp_kernel: positions never decrease along a row, so i_lo <= pos >> FB <= i_hi,
        // and Kh <= kWarpMaxHalf because s_j <= max(a, b) <= 2 * ONE; hence 0 <= at - Kh + 1 and at + Kh <= i_hi - i_lo + 75 < len
        // - len is never clipped, the tile's span being at most 255 increments of at most two samples.
        if (at - Kh + 1 >= 0 && at + Kh < len) {
            const float *w = xs + at;
            v = warp_sample(gs, pos, c, Kh, [&](int d) { return w[d]; });
        }
    }
    yrow[n] = v;
}

inline hipError_t launch_glide(const GlideArgs &a, int B, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo || a.n_lo < 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + kWarpBlock - 1) / kWarpBlock), (unsigned)B);
    glide_kernel<<<grid, kWarpBlock, 0, st>>>(a);
    return hipGetLastError();
}

// ---- pitch at an output rate (include/vitsmi.h, "pitch at an output rate"): the two kernels' wide siblings.
//
// The rate is folded into the records' steps (warp.hpp), so positions advance by up to eight input samples an output and a
// sample has up to 2 * 151 taps: a tile stages at most 255 * 8 + 2 + 2 * 151 floats, sized statically - 9.4 KB beside the
// 32 KB of G.  What it stages on either side of its positions is the ROW's largest Kh (WarpRateRow::half_max), not the
// family's: a row delivered upwards has some 19 half-taps, and staging 151 for it would read eight times what it uses.
// Geometry, the two searches, the walk to a lane's segment, the per-lane fence and warp_sample are the kernels' above.
//
// An identity row - every token at 0 semitones - is not rendered by its records but by the resampler's rule, so that it is
// resample_kernel's / resample_rows_kernel's row bit for bit: resample_sample over the row's table line h[p], t = n * M,
// i = t / L, p = t - i * L, the masked native row read straight from memory (the function gives the same bits on every input
// path: resample.hip.hpp).  Without a table (L == M) it is the masked copy.  That branch, like the zeros behind a row's end,
// returns in front of the barrier: whether a workgroup takes it depends on blockIdx and values indexed by it alone.
constexpr int kWarpRateSpan = (kWarpBlock - 1) * 8 + 2 + 2 * kWarpRateMaxHalf;  // 2344

template <class Seg>
struct WarpRateArgsT {
    const Seg *segs;
    const WarpRateRow *rows;  // [B]: the row's records, counts, largest Kh and its resampler plan (table, Kp, K, L, M)
    const float *G;           // [kWarpTable]
    const float *x;           // native input samples of row b at x + b * x_pitch
    int64_t x_pitch;
    float *y;                 // [B][y_pitch]: row b's output sample n_lo at y + b * y_pitch
    int64_t y_pitch;
    int n_hi, n_lo;           // the launch renders output samples [n_lo, n_hi) of every row, as WarpArgsT
};
using WarpRateArgs = WarpRateArgsT<vits_warp_seg>;
using GlideRateArgs = WarpRateArgsT<vits_glide_seg>;

// position, cutoff and half-taps of sample j of a record, by the closed forms of its family
__device__ __forceinline__ int64_t warp_rate_at(const vits_warp_seg &g, int64_t j, int32_t &c, int32_t &Kh) {
    c = g.c;
    Kh = g.half_taps;
    return g.pos0 + j * (int64_t)g.step;
}
__device__ __forceinline__ int64_t warp_rate_at(const vits_glide_seg &g, int64_t j, int32_t &c, int32_t &Kh) {
    glide_cutoff(glide_step(g.k, g.step0, g.step1, j), c, Kh);
    return glide_pos(g.pos0, g.k, g.step0, g.step1, j);
}

template <class Seg>
__device__ __forceinline__ void warp_rate_tile(const WarpRateArgsT<Seg> &a) {
    __shared__ float xs[kWarpRateSpan];
    __shared__ float gs[kWarpTable];
    const int b = blockIdx.y;
    const WarpRateRow r = a.rows[b];
    const int64_t n0 = a.n_lo + (int64_t)blockIdx.x * kWarpBlock, n = n0 + threadIdx.x;
    const float *xrow = a.x + (int64_t)b * a.x_pitch;
    float *yrow = a.y + (int64_t)b * a.y_pitch - a.n_lo;  // indexed by n
    if (n0 >= r.n_out || r.identity || r.n_segs <= 0) {  // behind the row's end: zeros; an identity row: the resampler's sample
        if (n >= a.n_hi) return;
        float v = 0.f;
        if (r.identity && n < r.n_out) {
            if (!r.table) v = n < r.n_in ? xrow[n] : 0.f;
            else {
                const int64_t t = n * r.M, i = t / r.L, p = t - i * r.L;
                const int64_t m0 = i - r.K / 2 + 1;
                const int n_in = r.n_in;
                v = resample_sample(r.table + p * r.Kp, r.K, [&](int j) {
                    const int64_t m = m0 + j;
                    return m >= 0 && m < n_in ? xrow[m] : 0.f;
                });
            }
        }
        yrow[n] = v;
        return;
    }
    const Seg *sg = a.segs + r.seg0;
    // the tile's last sample: clipped by the row and by the window, so that nothing behind the window's last position is staged
    const int64_t n_end = n0 + kWarpBlock < a.n_hi ? n0 + kWarpBlock : (int64_t)a.n_hi;
    const int64_t n_last = (n_end < r.n_out ? n_end : (int64_t)r.n_out) - 1;
    const int j0 = warp_find(sg, r.n_segs, n0), j1 = warp_find(sg, r.n_segs, n_last);
    int32_t c, Kh;
    const int64_t i_lo = warp_rate_at(sg[j0], n0 - sg[j0].n0, c, Kh) >> kWarpFB;
    const int64_t i_hi = warp_rate_at(sg[j1], n_last - sg[j1].n0, c, Kh) >> kWarpFB;
    const int64_t m_base = i_lo - r.half_max + 1;
    int64_t len = i_hi - i_lo + 2 * (int64_t)r.half_max;
    len = len > kWarpRateSpan ? kWarpRateSpan : len;  // (never: positions advance by at most eight samples an output, half_max <= 151)
    for (int q = threadIdx.x; q < (int)len; q += kWarpBlock) {
        const int64_t m = m_base + q;
        xs[q] = m >= 0 && m < r.n_in ? xrow[m] : 0.f;
    }
    for (int q = threadIdx.x; q < kWarpTable; q += kWarpBlock) gs[q] = a.G[q];
    __syncthreads();
    if (n >= a.n_hi) return;
    float v = 0.f;
    if (n < r.n_out) {
        int j = j0;
        while (j < j1 && sg[j + 1].n0 <= n) j++;
        const Seg g = sg[j];
        const int64_t pos = warp_rate_at(g, n - g.n0, c, Kh);
        const int64_t at = (pos >> kWarpFB) - m_base;  // the tap m = i0 in the staged span
        // the fence of warp_kernel: a record whose Kh exceeds the row's half_max, or a clipped span, renders 0 and reads nothing outside
        if (at - Kh + 1 >= 0 && at + Kh < len) {
            const float *w = xs + at;
            v = warp_sample(gs, pos, c, Kh, [&](int d) { return w[d]; });
        }
    }
    yrow[n] = v;
}

__global__ void __launch_bounds__(kWarpBlock) warp_rate_kernel(WarpRateArgs a) { warp_rate_tile(a); }
__global__ void __launch_bounds__(kWarpBlock) glide_rate_kernel(GlideRateArgs a) { warp_rate_tile(a); }

inline hipError_t launch_warp_rate(const WarpRateArgs &a, int B, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo || a.n_lo < 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + kWarpBlock - 1) / kWarpBlock), (unsigned)B);
    warp_rate_kernel<<<grid, kWarpBlock, 0, st>>>(a);
    return hipGetLastError();
}
inline hipError_t launch_glide_rate(const GlideRateArgs &a, int B, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo || a.n_lo < 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + kWarpBlock - 1) / kWarpBlock), (unsigned)B);
    glide_rate_kernel<<<grid, kWarpBlock, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace vitsmi
