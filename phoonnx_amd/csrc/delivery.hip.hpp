// delivery.hip.hpp — the kernels of a delivery (include/vitsmi.h, "delivery"; the plan: delivery.hpp).
//
// Two launches.  delivery_peak_kernel (skipped when no segment normalises) folds max |x| of every normalising segment's row
// into its peak slot - the row's own, or its stream's - with atomicMax on the float bits, which is order-independent.
// delivery_pack_kernel runs over the PACKED elements (the rows' valid samples only, in dst order), not over B x S_max: a
// workgroup owns 256 cells of 16 output bytes, finds the segment of its first element by binary search in the segment table
// and walks forward from there.  Every lane loads element base + i * 256 + lane of the tile (coalesced fp32), encodes it and
// parks it in LDS; after the barrier each lane stores its 16-byte cell.  The packed buffer starts 256-byte aligned and
// holds whole cells, so every store is a full 16-byte one wherever the segment boundaries fall inside a cell.
//
// A trimmed delivery (vitsmi.h, "trimmed delivery") puts delivery_trim_scan_kernel in front: the first and the last sample
// of every row above the segment's threshold, folded with atomicMin / atomicMax - order-independent like the peaks.  The host
// turns the bounds into kept ranges; the two kernels above then run over those, unchanged (a segment is src and n).
//
// A levelled delivery (vitsmi.h, "levelled delivery") measures in front of the pack (loudness.hip.hpp, and the peak kernel
// under the scan's grid); the pack kernel multiplies a levelled segment's samples by the gain in its record.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "delivery.hpp"

namespace vitsmi {

constexpr int kDeliveryThreads = 256;

template <int ENC> struct DeliveryElem { using type = int16_t; };
template <> struct DeliveryElem<VITS_ENC_ULAW> { using type = uint8_t; };
template <> struct DeliveryElem<VITS_ENC_ALAW> { using type = uint8_t; };
template <> struct DeliveryElem<VITS_ENC_F32> { using type = float; };

// the fp32 post-processing of one sample: the operations of pcm16_kernel in their order
__device__ inline float delivery_value(float v, bool norm, float peak, float volume) {
    if (norm) v = peak < 1e-8f ? 0.f : v / peak;
    if (volume != 1.0f) v = v * volume;
    return fminf(fmaxf(v, -1.0f), 1.0f);
}

__device__ inline int delivery_q16(float v) { return (int)(int16_t)fminf(fmaxf(v * 32767.0f, -32767.0f), 32767.0f); }

__device__ inline unsigned delivery_ulaw(int q) {
    const int s = q >> 2;
    const bool neg = s < 0;
    const int m = (neg ? -s : s) + 33;  // >= 33
    int seg = (31 - __clz(m)) - 5;
    seg = seg > 8 ? 8 : seg;
    const unsigned u = seg == 8 ? 0x7Fu : (unsigned)((seg << 4) | ((m >> (seg + 1)) & 15));
    return (u ^ (neg ? 0x7Fu : 0xFFu)) & 0xFFu;
}

__device__ inline unsigned delivery_alaw(int q) {
    const int s = q >> 3;
    const bool neg = s < 0;
    const int m = neg ? -s - 1 : s;
    int seg = (31 - __clz(m > 1 ? m : 1)) - 4;
    seg = seg < 0 ? 0 : (seg > 7 ? 7 : seg);
    const unsigned a = (unsigned)((seg << 4) | ((seg < 2 ? m >> 1 : m >> seg) & 15));
    return (a ^ (neg ? 0x55u : 0xD5u)) & 0xFFu;
}

template <int ENC>
__device__ inline typename DeliveryElem<ENC>::type delivery_encode(float v) {
    if constexpr (ENC == VITS_ENC_F32) return v;
    else if constexpr (ENC == VITS_ENC_PCM16) return (int16_t)delivery_q16(v);
    else if constexpr (ENC == VITS_ENC_ULAW) return (uint8_t)delivery_ulaw(delivery_q16(v));
    else return (uint8_t)delivery_alaw(delivery_q16(v));
}

// grid (gx, G): segment blockIdx.y's row, folded into its slot
__global__ __launch_bounds__(kDeliveryThreads) void delivery_peak_kernel(const float *x, const DeliverySeg *segs, unsigned *peak_bits) {
    const DeliverySeg s = segs[blockIdx.y];
    if (s.peak < 0) return;
    float m = 0.f;
    for (int i = blockIdx.x * kDeliveryThreads + threadIdx.x; i < s.n; i += gridDim.x * kDeliveryThreads)
        m = fmaxf(m, fabsf(x[s.src + i]));
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && s.n > 0) atomicMax(&peak_bits[s.peak], __float_as_uint(m));  // non-negative floats order as uints
}

// grid (gx, G) over a SCAN table: segment blockIdx.y's row [src, src + n) as in the plan, with `pad` = the trim's mode,
// `volume` = its threshold and `peak` = the slot of peak_all that holds the row's max |x| (mode 2), or -1.  bounds [G][2]
// must read {INT_MAX, -1}: they receive the smallest and the largest i < n with |x[i]| > thr (strictly; a NaN is not active).
__global__ __launch_bounds__(kDeliveryThreads) void delivery_trim_scan_kernel(const float *x, const DeliverySeg *segs, const unsigned *peak_all,
                                                                              int *bounds) {
    const DeliverySeg s = segs[blockIdx.y];
    if (s.pad == 0) return;
    float thr = s.volume;
    if (s.peak >= 0) thr = thr * __uint_as_float(peak_all[s.peak]);
    int lo = INT_MAX, hi = -1;
    // (an int64 index: i + the grid's stride may pass INT_MAX for n close to it)
    for (int64_t i = (int64_t)blockIdx.x * kDeliveryThreads + threadIdx.x; i < s.n; i += (int64_t)gridDim.x * kDeliveryThreads)
        if (fabsf(x[s.src + i]) > thr) {
            lo = (int)i < lo ? (int)i : lo;
            hi = (int)i;  // (a lane's indices ascend)
        }
    for (int o = 32; o > 0; o >>= 1) {
        const int l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && hi >= 0) {
        atomicMin(&bounds[2 * blockIdx.y], lo);
        atomicMax(&bounds[2 * blockIdx.y + 1], hi);
    }
}

// the scan of a trimmed delivery on `st`: d_scan [G] the scan table, bounds [G][2] preset, peak_all [G] zero when any_rel
// (some segment's threshold is relative: the peak launch over the untrimmed rows goes in front).  G > 0.
// Grid: a lane walks about kTrimSpan samples, at most 64 workgroups a row.  Every wave ends in atomics on its row's slots,
// and those serialise; the fewer waves, the fewer of them.  Measured in DESIGN.md 5.10 (kernel trace, 32 rows of 215 040
// samples): delivery_peak_kernel 0.299 ms under launch_delivery's grid (a sample per lane, up to 256 workgroups a row),
// 0.032 ms under this one; this scan 0.045 ms.
constexpr int kTrimSpan = 32;
inline int trim_scan_gx(int max_n) {
    const int gx = (max_n + kDeliveryThreads * kTrimSpan - 1) / (kDeliveryThreads * kTrimSpan);
    return gx > 64 ? 64 : (gx < 1 ? 1 : gx);
}
inline hipError_t launch_trim_scan(const float *x, const DeliverySeg *d_scan, int G, int max_n, bool any_rel, unsigned *d_peak_all, int *d_bounds,
                                   hipStream_t st) {
    const int gx = trim_scan_gx(max_n);
    if (any_rel) delivery_peak_kernel<<<dim3(gx, G), kDeliveryThreads, 0, st>>>(x, d_scan, d_peak_all);
    delivery_trim_scan_kernel<<<dim3(gx, G), kDeliveryThreads, 0, st>>>(x, d_scan, d_peak_all, d_bounds);
    return hipGetLastError();
}

// the sample peaks of a levelled delivery on `st`: d_table [G] the plan's table with `peak` = the slot of every levelled
// segment (-1: not measured), d_peak zeroed.  The scan's grid: the measurement above.
inline hipError_t launch_level_peaks(const float *x, const DeliverySeg *d_table, int G, int max_n, unsigned *d_peak, hipStream_t st) {
    delivery_peak_kernel<<<dim3(trim_scan_gx(max_n), G), kDeliveryThreads, 0, st>>>(x, d_table, d_peak);
    return hipGetLastError();
}

// grid ceil(P / (256 * E)), E = 16 / sizeof(element): packed elements [0, P) -> cells of 16 bytes; the last cell is
// written whole (zeros behind P: the packed buffer holds whole cells)
template <int ENC>
__global__ __launch_bounds__(kDeliveryThreads) void delivery_pack_kernel(const float *x, const DeliverySeg *segs, int G,
                                                                         const unsigned *peak_bits, int64_t P, uint4 *packed) {
    using T = typename DeliveryElem<ENC>::type;
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ uint4 tile[kDeliveryThreads];
    T *lt = reinterpret_cast<T *>(tile);
    const int64_t base = (int64_t)blockIdx.x * (kDeliveryThreads * E);
    // the last segment that starts at or in front of the tile (segs[0].start == 0; empty segments share a start with their
    // successor and are passed over)
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].start <= base) lo = mid;
        else hi = mid;
    }
    int g = lo, loaded = lo;
    DeliverySeg s = segs[g];
    int64_t next = g + 1 < G ? segs[g + 1].start : P;
    // (unrolled by four: the passes' loads do not depend on one another, so the compiler may issue them together instead of
    // waiting out one latency per pass; the kernel's own time has not been profiled)
#pragma unroll 4
    for (int i = 0; i < E; i++) {
        const int64_t e = base + (int64_t)i * kDeliveryThreads + threadIdx.x;
        T o = T(0);
        if (e < P) {
            while (e >= next) {  // (e < P: ends at the segment that holds e)
                g++;
                next = g + 1 < G ? segs[g + 1].start : P;
            }
            if (loaded != g) {
                s = segs[g];
                loaded = g;
            }
            const float peak = s.peak >= 0 ? __uint_as_float(peak_bits[s.peak]) : 1.f;
            float v = x[s.src + (e - s.start)];
            if (s.peak == kDeliveryLevelled) v = v * __int_as_float(s.pad);  // (one fp32 product, in front of the volume's)
            o = delivery_encode<ENC>(delivery_value(v, s.peak >= 0, peak, s.volume));
        }
        lt[i * kDeliveryThreads + threadIdx.x] = o;
    }
    __syncthreads();
    const int64_t cell = base / E + threadIdx.x;
    if (cell * E < P) packed[cell] = tile[threadIdx.x];
}

// what every delivery launches in front of its pack: the peak launch on `st` where a segment normalises (a sample per lane, up
// to 256 workgroups a row) -> the pack launch's grid, plain or shaped (shape.hip.hpp)
inline dim3 launch_delivery_peaks(const float *x, const DeliveryPlan &p, const DeliverySeg *d_segs, unsigned *d_peak, hipStream_t st) {
    if (p.any_norm) {
        int gx = (p.max_n + kDeliveryThreads - 1) / kDeliveryThreads;
        gx = gx > 256 ? 256 : (gx < 1 ? 1 : gx);
        delivery_peak_kernel<<<dim3(gx, (unsigned)p.segs.size()), kDeliveryThreads, 0, st>>>(x, d_segs, d_peak);
    }
    const int64_t per = (int64_t)kDeliveryThreads * (16 / p.width);
    return dim3((unsigned)((p.packed_elems + per - 1) / per));
}

// both launches on `st`; peak_bits [2B] must read 0 (the caller's memset in front).  P > 0.
inline hipError_t launch_delivery(const float *x, const DeliveryPlan &p, const DeliverySeg *d_segs, unsigned *d_peak, void *d_packed,
                                  hipStream_t st) {
    const int G = (int)p.segs.size();
    const int64_t P = p.packed_elems;
    const dim3 grid = launch_delivery_peaks(x, p, d_segs, d_peak, st);
    uint4 *out = static_cast<uint4 *>(d_packed);
    switch (p.encoding) {
        case VITS_ENC_PCM16: delivery_pack_kernel<VITS_ENC_PCM16><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out); break;
        case VITS_ENC_ULAW: delivery_pack_kernel<VITS_ENC_ULAW><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out); break;
        case VITS_ENC_ALAW: delivery_pack_kernel<VITS_ENC_ALAW><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out); break;
        default: delivery_pack_kernel<VITS_ENC_F32><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out); break;
    }
    return hipGetLastError();
}

}  // namespace vitsmi
