// shape.hip.hpp — the pack launch of a shaped delivery (include/vitsmi.h, "shaped delivery"; the plan: shape.hpp).
//
// delivery_pack_shaped_kernel<ENC> is a kernel of its own beside delivery_pack_kernel<ENC> (delivery.hip.hpp), not a template
// switch on it: a delivery without shapes launches exactly the instantiation it launched before, and this file does not
// touch that one's code.  The structure is the same - 256 lanes, a tile of 256 cells of 16 output bytes through LDS, a
// binary search in the segment table for the tile's first segment, a walk forward from there - and so is every operation
// of the sample formula up to the volume's product; then comes v = v * mul, then the clip and the encoder.
//
// The multiplier is shape.hpp's, the same functions the host rule runs (each product, sum and quotient in a function compiled
// with contraction off: shape.hpp says why __fmul_rn and its kin do not serve).  New per element is finding the breakpoint
// interval of row sample i.  A lane's elements in successive passes are 256 apart and ascend, so: ONE binary search per
// (lane, segment) - the first element of the lane in that segment - and from then on a forward walk, `while i has reached
// the next knot`, which steps over as many points as lie between two passes.  The envelope is read as KNOTS (shape.hpp): one
// 16-byte record per interval that carries all an element needs, its successor's position included - so an element whose
// lane stays in its interval loads nothing, and one that moves on loads one record per point passed.  (Points and slopes
// read as the caller gives them are four dependent loads per element: measured, 36 us against 27.6 for 510 points a row;
// DESIGN.md 5.12.)  A segment without points has one knot of gain 1; a segment without a shape therefore multiplies by
// 1.0f, which changes no bit.
// The knots are NOT staged in LDS: they are few (two per token boundary at most: some hundreds per row), every lane of a
// wave reads the same or neighbouring ones, and they stay in L2; DESIGN.md 5.12 has the measurement.
#pragma once
#include <hip/hip_runtime.h>

#include "delivery.hip.hpp"
#include "shape.hpp"

namespace vitsmi {

template <int ENC>
__global__ __launch_bounds__(kDeliveryThreads) void delivery_pack_shaped_kernel(const float *x, const DeliverySeg *segs, int G,
                                                                                const unsigned *peak_bits, int64_t P, uint4 *packed,
                                                                                const ShapeSeg *shapes, const ShapeKnot *knots) {
    using T = typename DeliveryElem<ENC>::type;
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ uint4 tile[kDeliveryThreads];
    T *lt = reinterpret_cast<T *>(tile);
    const int64_t base = (int64_t)blockIdx.x * (kDeliveryThreads * E);
    // the last segment that starts at or in front of the tile (delivery_pack_kernel's search)
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].start <= base) lo = mid;
        else hi = mid;
    }
    int g = lo, loaded = -1;
    DeliverySeg s{};
    ShapeSeg sh{};
    ShapeKnot kn{};        // the knot of this lane's last element in segment `loaded`
    int kp = 0;            // ... and its index among the segment's
    bool located = false;  // ... once the binary search has run for it
    int64_t next = g + 1 < G ? segs[g + 1].start : P;
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
                sh = shapes[g];
                loaded = g;
                located = false;
            }
            const int32_t j = (int32_t)(e - s.start);  // < s.n == sh.c
            const int32_t ir = sh.a + j;               // the row sample: breakpoints count from the row's start
            if (!located) {
                kp = shape_knot_locate(knots + sh.first, sh.n_points, ir);
                kn = knots[sh.first + kp];
                located = true;
            }
            while (ir >= kn.next) kn = knots[sh.first + ++kp];  // (the last knot's next is INT_MAX: kp stays <= n_points)
            const float mul = shape_combine(shape_knot_env(kn, ir), shape_w_in(j, sh.fade_in, sh.curve), shape_w_out(j, sh.c, sh.fade_out, sh.curve));
            const float peak = s.peak >= 0 ? __uint_as_float(peak_bits[s.peak]) : 1.f;
            float v = x[s.src + j];
            if (s.peak == kDeliveryLevelled) v = v * __int_as_float(s.pad);
            if (s.peak >= 0) v = peak < 1e-8f ? 0.f : v / peak;
            if (s.volume != 1.0f) v = v * s.volume;
            v = shape_mul(v, mul);
            o = delivery_encode<ENC>(fminf(fmaxf(v, -1.0f), 1.0f));
        }
        lt[i * kDeliveryThreads + threadIdx.x] = o;
    }
    __syncthreads();
    const int64_t cell = base / E + threadIdx.x;
    if (cell * E < P) packed[cell] = tile[threadIdx.x];
}

// launch_delivery with the shaped pack: d_shapes [G] parallel to d_segs, d_knots the knots of all of them.  P > 0.
inline hipError_t launch_delivery_shaped(const float *x, const DeliveryPlan &p, const DeliverySeg *d_segs, unsigned *d_peak, void *d_packed,
                                         const ShapeSeg *d_shapes, const ShapeKnot *d_knots, hipStream_t st) {
    const int G = (int)p.segs.size();
    const int64_t P = p.packed_elems;
    const dim3 grid = launch_delivery_peaks(x, p, d_segs, d_peak, st);
    uint4 *out = static_cast<uint4 *>(d_packed);
#define VITSMI_SHAPED(ENC) \
    delivery_pack_shaped_kernel<ENC><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out, d_shapes, d_knots)
    switch (p.encoding) {
        case VITS_ENC_PCM16: VITSMI_SHAPED(VITS_ENC_PCM16); break;
        case VITS_ENC_ULAW: VITSMI_SHAPED(VITS_ENC_ULAW); break;
        case VITS_ENC_ALAW: VITSMI_SHAPED(VITS_ENC_ALAW); break;
        default: VITSMI_SHAPED(VITS_ENC_F32); break;
    }
#undef VITSMI_SHAPED
    return hipGetLastError();
}

}  // namespace vitsmi
