// warp.hip.hpp — the per-token time warp on the device (include/vitsmi.h, "Intonation"; plan: warp.hpp).
//
// One workgroup renders kWarpBlock consecutive output samples of one row (warp_tile: one body for constant and gliding tokens,
// at the native and at a folded output rate).  Input positions never decrease along a row and advance by at most two samples
// per output, so the tile reads at most 255 * 2 + 2 + 76 input floats (a folded rate: eight and 255 * 8 + 2 + 302, below): they
// are staged once in LDS, already masked to the row's valid samples.  The workgroup finds the segments of its first and of its last sample
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
#include <type_traits>

#include "resample.hip.hpp"
#include "warp.hpp"

namespace vitsmi {

constexpr int kWarpBlock = 256;                                        // output samples (= threads) per workgroup
constexpr int kWarpSpan = (kWarpBlock - 1) * 2 + 2 + 2 * kWarpMaxHalf;  // the input floats a tile stages at most (588)
constexpr int kWarpRateSpan = (kWarpBlock - 1) * 8 + 2 + 2 * kWarpRateMaxHalf;  // ... of a folded launch (2344: below)

// One launch over records of either family (Seg: vits_warp_seg, or vits_glide_seg - "pitch contours") and rows of either
// width (Row: WarpRow, or WarpRateRow - "pitch at an output rate")
template <class Seg, class Row>
struct WarpArgsT {
    const Seg *segs;
    const Row *rows;  // [B]; a WarpRateRow adds the row's largest Kh and its resampler plan (table, Kp, K, L, M)
    const float *G;   // [kWarpTable]
    const float *x;   // (native) input samples of row b at x + b * x_pitch
    int64_t x_pitch;
    float *y;         // [B][y_pitch]: row b's output sample n_lo at y + b * y_pitch
    int64_t y_pitch;
    int n_hi;         // the launch renders output samples [n_lo, n_hi) of every row; a whole run: [0, S_w)
    int n_lo;         // a window of a streamed run ("streamed pitch"): tile i covers [n_lo + 256 i, ...), clipped by n_hi
};
using WarpArgs = WarpArgsT<vits_warp_seg, WarpRow>;
using GlideArgs = WarpArgsT<vits_glide_seg, WarpRow>;
using WarpRateArgs = WarpArgsT<vits_warp_seg, WarpRateRow>;
using GlideRateArgs = WarpArgsT<vits_glide_seg, WarpRateRow>;

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

// ---- what differs per record family.  The position of sample j of a record is warp_seg_pos (warp.hpp); its cutoff and half-taps:
// a constant token carries them, a gliding one ("pitch contours") has them from its speed by the closed forms of the definition
// (glide_step, glide_cutoff).  With glide_pos that is three plain unsigned 64-bit divisions a lane - by k, by 2k, by 20s - in
// the compiler's expansion: the numerators reach 2^63, so neither a 32-bit nor a floating-point reciprocal gives the
// definition's integers for every input, and against the 38..76 taps of a sample they are a few per cent.  Lanes of one wave
// then differ in Kh inside a token: the tap loop runs to the wave's longest.
__device__ __forceinline__ void warp_seg_cutoff(const vits_warp_seg &g, int64_t, int32_t &c, int32_t &Kh) {
    c = g.c;
    Kh = g.half_taps;
}
__device__ __forceinline__ void warp_seg_cutoff(const vits_glide_seg &g, int64_t j, int32_t &c, int32_t &Kh) {
    glide_cutoff(glide_step(g.k, g.step0, g.step1, j), c, Kh);
}

// ---- what differs per row width.  A native row's positions advance by at most two samples an output - a gliding token's too:
// every increment lies in [min(a, b), max(a, b)] <= 2 * ONE, across segment boundaries as well (a token starts at the pos_k of
// the one before it) - and a sample has at most 2 * 38 taps.  A folded row ("pitch at an output rate": the rate is in the
// records' steps, warp.hpp) advances by up to eight with up to 2 * 151 taps: 255 * 8 + 2 + 2 * 151 floats, 9.4 KB beside the
// 32 KB of G.  What such a tile stages on either side of its positions is the ROW's largest Kh, not the family's: a row
// delivered upwards has some 19 half-taps, and staging 151 for it would read eight times what it uses.
template <class Row>
constexpr int kWarpSpanOf = std::is_same_v<Row, WarpRateRow> ? kWarpRateSpan : kWarpSpan;

__device__ __forceinline__ int warp_row_half(const WarpRow &) { return kWarpMaxHalf; }
__device__ __forceinline__ int warp_row_half(const WarpRateRow &r) { return r.half_max; }

// Sample n < n_out of an identity row.  Native - every step the unit step -: the masked copy.  Folded - every token at 0
// semitones -: not its records' but the resampler's, so that it is resample_kernel's / resample_rows_kernel's row bit for bit:
// resample_sample over the row's table line h[p], t = n * M, i = t / L, p = t - i * L, the masked native row read straight from
// memory (the function gives the same bits on every input path: resample.hip.hpp); without a table (L == M) the masked copy.
__device__ __forceinline__ float warp_identity_sample(const WarpRow &r, const float *xrow, int64_t n) { return n < r.n_in ? xrow[n] : 0.f; }
__device__ __forceinline__ float warp_identity_sample(const WarpRateRow &r, const float *xrow, int64_t n) {
    if (!r.table) return n < r.n_in ? xrow[n] : 0.f;
    const int64_t t = n * r.M, i = t / r.L, p = t - i * r.L;
    const int64_t m0 = i - r.K / 2 + 1;
    const int n_in = r.n_in;
    return resample_sample(r.table + p * r.Kp, r.K, [&](int j) {
        const int64_t m = m0 + j;
        return m >= 0 && m < n_in ? xrow[m] : 0.f;
    });
}

// THE tile: kWarpBlock consecutive output samples of row blockIdx.y, for every family and width (the header's account).
template <class Seg, class Row>
__device__ __forceinline__ void warp_tile(const WarpArgsT<Seg, Row> &a) {
    constexpr int kSpan = kWarpSpanOf<Row>;
    __shared__ float xs[kSpan];
    __shared__ float gs[kWarpTable];
    const int b = blockIdx.y;
    const Row r = a.rows[b];
    const int64_t n0 = a.n_lo + (int64_t)blockIdx.x * kWarpBlock, n = n0 + threadIdx.x;
    const float *xrow = a.x + (int64_t)b * a.x_pitch;
    float *yrow = a.y + (int64_t)b * a.y_pitch - a.n_lo;  // indexed by n
    // behind the row's end: zeros; an identity row: its own sample.  Like everything in front of the barrier the branch is
    // uniform: whether a workgroup takes it depends on blockIdx and values indexed by it alone.
    if (n0 >= r.n_out || r.identity || r.n_segs <= 0) {
        if (n < a.n_hi) yrow[n] = r.identity && n < r.n_out ? warp_identity_sample(r, xrow, n) : 0.f;
        return;
    }
    const Seg *sg = a.segs + r.seg0;
    // the tile's last sample: clipped by the row and by the window, so that nothing behind the window's last position is staged
    const int64_t n_end = n0 + kWarpBlock < a.n_hi ? n0 + kWarpBlock : (int64_t)a.n_hi;
    const int64_t n_last = (n_end < r.n_out ? n_end : (int64_t)r.n_out) - 1;
    const int j0 = warp_find(sg, r.n_segs, n0), j1 = warp_find(sg, r.n_segs, n_last);
    const int64_t i_lo = warp_seg_pos(sg[j0], n0 - sg[j0].n0) >> kWarpFB;
    const int64_t i_hi = warp_seg_pos(sg[j1], n_last - sg[j1].n0) >> kWarpFB;
    const int half = warp_row_half(r);
    const int64_t m_base = i_lo - half + 1;
    int64_t len = i_hi - i_lo + 2 * (int64_t)half;
    len = len > kSpan ? kSpan : len;  // (never: positions advance by at most two - folded: eight - samples an output, half <= 38 - 151)
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
        const int64_t pos = warp_seg_pos(g, n - g.n0);
        int32_t c, Kh;
        warp_seg_cutoff(g, n - g.n0, c, Kh);
        const int64_t at = (pos >> kWarpFB) - m_base;  // the tap m = i0 in the staged span
        // A fence, and for a checked plan dead code: positions never decrease along a row, so i_lo <= pos >> FB <= i_hi, and
        // Kh <= half (a native record's s_j <= max(a, b) <= 2 * ONE, a folded row's half_max is the largest of its records');
        // hence 0 <= at - Kh + 1 and at + Kh <= i_hi - i_lo + 2 * half - 1 < len - len is never clipped, the tile's span being
        // at most 255 increments of at most two (eight) samples.  A record that breaks this renders 0 and reads nothing outside.
        if (at - Kh + 1 >= 0 && at + Kh < len) {
            const float *w = xs + at;
            v = warp_sample(gs, pos, c, Kh, [&](int d) { return w[d]; });
        }
    }
    yrow[n] = v;
}

// One entry per family and width, each with its own LDS: the native pair stages kWarpSpan floats beside G (35 136 bytes a
// workgroup), the folded pair kWarpRateSpan (42 160) - a native launch through the wide body would pay a workgroup per CU.
__global__ void __launch_bounds__(kWarpBlock) warp_kernel(WarpArgs a) { warp_tile(a); }
__global__ void __launch_bounds__(kWarpBlock) glide_kernel(GlideArgs a) { warp_tile(a); }
__global__ void __launch_bounds__(kWarpBlock) warp_rate_kernel(WarpRateArgs a) { warp_tile(a); }
__global__ void __launch_bounds__(kWarpBlock) glide_rate_kernel(GlideRateArgs a) { warp_tile(a); }

inline auto warp_entry(const WarpArgs &) { return warp_kernel; }
inline auto warp_entry(const GlideArgs &) { return glide_kernel; }
inline auto warp_entry(const WarpRateArgs &) { return warp_rate_kernel; }
inline auto warp_entry(const GlideRateArgs &) { return glide_rate_kernel; }

// launch over output samples [a.n_lo, a.n_hi) of B rows
template <class Seg, class Row>
inline hipError_t launch_warp_tile(const WarpArgsT<Seg, Row> &a, int B, hipStream_t st) {
    if (B <= 0 || a.n_hi <= a.n_lo || a.n_lo < 0) return hipSuccess;
    const dim3 grid((unsigned)(((int64_t)a.n_hi - a.n_lo + kWarpBlock - 1) / kWarpBlock), (unsigned)B);
    warp_entry(a)<<<grid, kWarpBlock, 0, st>>>(a);
    return hipGetLastError();
}

}  // namespace vitsmi
