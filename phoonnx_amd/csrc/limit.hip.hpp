// limit.hip.hpp — the two launches of a limited delivery (include/vitsmi.h, "limited delivery"; the plan: limit.hpp).
//
// They stand beside the existing ones and run only when some segment is limited: delivery_pack_kernel and
// delivery_pack_shaped_kernel are not touched, and a delivery without limits launches exactly what it launched before.
//
// limit_gain_kernel writes g for every packed element into an fp32 buffer [packed_elems]; delivery_pack_limited_kernel<ENC>
// is the shaped pack's body with v = v * g[e] and the clamp to +-ceiling in front of the clip.  Both form the unlimited
// value u of a sample with ONE function, limit_value: the shaped pack's operations up to and including v = v * mul, in its
// order (a segment without a shape has the one-knot envelope of gain 1).
//
// The gain kernel.  A workgroup of 256 lanes owns a tile of kLimitTile packed elements; for each piece [j0, j1) of a limited
// segment inside the tile:
//   stage  q[j] for j in [j0 - L, j1 + L) in LDS, 65536 outside [0, c) - so no read of x leaves the kept range, and a
//          segment never sees its neighbours;
//   minima M[j] = min q[j .. j + L] by doubling: m_1 = q, m_2s[t] = min(m_s[t], m_s[t + s]) while 2s <= L + 1, between two
//          LDS buffers, then M[t] = min(m_s[t], m_s[t + L + 1 - s]) - floor(log2(L + 1)) + 1 passes, every one over the whole
//          staged range and closed by a barrier;
//   sums   an exclusive prefix sum E of M over the workgroup (a run of consecutive entries per lane, a shuffle scan of the
//          lanes' totals in each wave, the four wave totals through LDS), S[j] = E[j + 1] - E[j - L];
//   gain   g = (float)S / (float)((L + 1) * 65536), limit.hpp's limit_g.
// A piece with nothing above the ceiling within L of it skips minima and sums: every q is 65536, so g is 1.0f by the rule.
// Everything in front of the division is int32 (E <= 3072 * 65536 < 2^31), so the scheme cannot show in the bits.  Every
// loop that holds a barrier runs a trip count that depends on the block and the segment alone: the pieces of the tile, and
// the passes of L.  LDS is static: two buffers of kLimitTile + 2 * VITS_LIMIT_MAX_LOOKAHEAD ints, 32 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include "delivery.hip.hpp"
#include "limit.hpp"
#include "shape.hpp"

namespace vitsmi {

constexpr int kLimitTile = 2048;                                     // packed elements of a workgroup of the gain kernel
constexpr int kLimitStage = kLimitTile + 2 * VITS_LIMIT_MAX_LOOKAHEAD;  // staged q of a piece with its halos

// a lane's place in a segment's knots: the shaped pack's walk (shape.hip.hpp) - one binary search per (lane, segment), then
// forward, since a lane's samples within a segment ascend
struct LimitKnotWalk {
    ShapeKnot kn{};
    int kp = 0;
    bool located = false;
};

// u of kept sample j of segment s / sh: the shaped pack's operations up to and including v = v * mul
__device__ inline float limit_value(const float *x, const DeliverySeg &s, const ShapeSeg &sh, const ShapeKnot *knots, const unsigned *peak_bits,
                                    int32_t j, LimitKnotWalk &w) {
    const int32_t ir = sh.a + j;  // the row sample: breakpoints count from the row's start
    if (!w.located) {
        w.kp = shape_knot_locate(knots + sh.first, sh.n_points, ir);
        w.kn = knots[sh.first + w.kp];
        w.located = true;
    }
    while (ir >= w.kn.next) w.kn = knots[sh.first + ++w.kp];  // (the last knot's next is INT_MAX: kp stays <= n_points)
    const float mul = shape_combine(shape_knot_env(w.kn, ir), shape_w_in(j, sh.fade_in, sh.curve), shape_w_out(j, sh.c, sh.fade_out, sh.curve));
    const float peak = s.peak >= 0 ? __uint_as_float(peak_bits[s.peak]) : 1.f;
    float v = x[s.src + j];
    if (s.peak == kDeliveryLevelled) v = v * __int_as_float(s.pad);
    if (s.peak >= 0) v = peak < 1e-8f ? 0.f : v / peak;
    if (s.volume != 1.0f) v = v * s.volume;
    return shape_mul(v, mul);
}

// The parallel form of the rule, stated once for every kernel that stages q (limit_gain_kernel here, the limited stream pack
// of stream_shape.hip.hpp): buf[0][t], t < n + 2 L, holds q of a piece of n samples with its halos, visible to the whole
// workgroup (a barrier lies behind the staging).  Returns E, the exclusive prefix sums of M[0 .. n + L], in one of the two
// buffers: S of the piece's sample i is E[i + L + 1] - E[i].  Every lane of the workgroup calls it with the same arguments;
// its loops run trip counts that depend on n and L alone, and it ends behind a barrier.
__device__ inline const int32_t *limit_window_sums(int32_t (*buf)[kLimitStage], int32_t *wave_sum, int32_t n, int32_t L) {
    const int lane = threadIdx.x;
    const int32_t W = L + 1, nq = n + 2 * L, nm = n + L;
    int cur = 0, span = 1;  // buf[cur][t] = min q over [t, t + span)
    while (2 * span <= W) {
        for (int t = lane; t < nq; t += kDeliveryThreads) {
            const int32_t a = buf[cur][t];
            const int32_t b = t + span < nq ? buf[cur][t + span] : kLimitUnity;
            buf[cur ^ 1][t] = b < a ? b : a;
        }
        __syncthreads();
        cur ^= 1;
        span *= 2;
    }
    // M[t] = min over [t, t + W) from two spans; M[nm] = 0 closes the prefix sums (t + W - span + span - 1 = t + L < nq)
    int32_t *const M = buf[cur ^ 1];
    for (int t = lane; t <= nm; t += kDeliveryThreads) {
        int32_t m = 0;
        if (t < nm) {
            const int32_t a = buf[cur][t], b = buf[cur][t + W - span];
            m = b < a ? b : a;
        }
        M[t] = m;
    }
    __syncthreads();
    // exclusive prefix sums of M[0 .. nm] in place: lane owns [lane * K, lane * K + K)
    const int K = (nm + 1 + kDeliveryThreads - 1) / kDeliveryThreads;
    const int t0 = lane * K, t1 = t0 + K < nm + 1 ? t0 + K : nm + 1;
    int32_t mine = 0;
    for (int t = t0; t < t1; t++) mine += M[t];
    int32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t up = __shfl_up(incl, o);
        if ((lane & 63) >= o) incl += up;
    }
    if ((lane & 63) == 63) wave_sum[lane >> 6] = incl;
    __syncthreads();
    int32_t run = incl - mine;
    for (int wv = 0; wv < (lane >> 6); wv++) run += wave_sum[wv];
    for (int t = t0; t < t1; t++) {
        const int32_t m = M[t];
        M[t] = run;
        run += m;
    }
    __syncthreads();
    return M;
}

// grid ceil(P / kLimitTile): gain [P] receives g of every packed element (1.0f in a segment that is not limited)
__global__ __launch_bounds__(kDeliveryThreads) void limit_gain_kernel(const float *x, const DeliverySeg *segs, int G, const unsigned *peak_bits,
                                                                      int64_t P, const ShapeSeg *shapes, const ShapeKnot *knots,
                                                                      const LimitSeg *limits, float *gain) {
    __shared__ int32_t buf[2][kLimitStage];
    __shared__ int32_t wave_sum[kDeliveryThreads / 64];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kLimitTile;
    const int64_t end = base + kLimitTile < P ? base + kLimitTile : P;
    // the last segment that starts at or in front of the tile (delivery_pack_kernel's search)
    int lo = 0, hi = G;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (segs[mid].start <= base) lo = mid;
        else hi = mid;
    }
    // (g, and with it every condition below that does not name `lane`, is uniform over the workgroup)
    for (int g = lo; g < G; g++) {
        const DeliverySeg s = segs[g];
        if (s.start >= end) break;
        const int64_t p0 = s.start > base ? s.start : base, p1 = s.start + s.n < end ? s.start + s.n : end;
        if (p1 <= p0) continue;  // an empty segment, or one that ends in front of the tile
        const LimitSeg lm = limits[g];
        const int32_t j0 = (int32_t)(p0 - s.start), n = (int32_t)(p1 - p0);  // the piece: kept samples [j0, j0 + n), n <= kLimitTile
        if (!lm.on) {
            for (int t = lane; t < n; t += kDeliveryThreads) gain[p0 + t] = 1.0f;
            continue;
        }
        const int32_t L = lm.L;
        const int32_t nq = n + 2 * L;  // staged q: j = j0 - L + t, t < nq
        const ShapeSeg sh = shapes[g];
        LimitKnotWalk walk;
        bool ducks = false;  // some staged sample of this lane is above the ceiling
        for (int t = lane; t < nq; t += kDeliveryThreads) {
            const int32_t j = j0 - L + t;
            const int32_t q = j < 0 || j >= s.n ? kLimitUnity : limit_q(limit_value(x, s, sh, knots, peak_bits, j, walk), lm.ceiling);
            buf[0][t] = q;
            ducks = ducks || q < kLimitUnity;
        }
        // (the barrier's answer is the workgroup's: uniform.)  Nothing above the ceiling within L of the piece: every M is
        // 65536, S = (L + 1) * 65536 and g = S / S = 1.0f - the rule's own value, without the passes
        if (!__syncthreads_or(ducks)) {
            for (int t = lane; t < n; t += kDeliveryThreads) gain[p0 + t] = 1.0f;
            continue;
        }
        const int32_t *const M = limit_window_sums(buf, wave_sum, n, L);
        // kept sample j0 + i: M indices [i, i + L]
        for (int i = lane; i < n; i += kDeliveryThreads) gain[p0 + i] = limit_g(M[i + L + 1] - M[i], L);
        __syncthreads();  // (the next piece stages into the same buffers)
    }
}

template <int ENC>
__global__ __launch_bounds__(kDeliveryThreads) void delivery_pack_limited_kernel(const float *x, const DeliverySeg *segs, int G,
                                                                                 const unsigned *peak_bits, int64_t P, uint4 *packed,
                                                                                 const ShapeSeg *shapes, const ShapeKnot *knots,
                                                                                 const LimitSeg *limits, const float *gain) {
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
    LimitSeg lm{};
    LimitKnotWalk walk;
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
                lm = limits[g];
                loaded = g;
                walk.located = false;
            }
            float v = limit_value(x, s, sh, knots, peak_bits, (int32_t)(e - s.start), walk);
            if (lm.on) v = limit_apply(v, gain[e], lm.ceiling);
            o = delivery_encode<ENC>(fminf(fmaxf(v, -1.0f), 1.0f));
        }
        lt[i * kDeliveryThreads + threadIdx.x] = o;
    }
    __syncthreads();
    const int64_t cell = base / E + threadIdx.x;
    if (cell * E < P) packed[cell] = tile[threadIdx.x];
}

// launch_delivery_shaped with the limiter: the peak launch where a segment normalises, the gain launch, the limited pack.
// d_limits [G] parallel to d_segs, d_gain [P].  P > 0.
inline hipError_t launch_delivery_limited(const float *x, const DeliveryPlan &p, const DeliverySeg *d_segs, unsigned *d_peak, void *d_packed,
                                          const ShapeSeg *d_shapes, const ShapeKnot *d_knots, const LimitSeg *d_limits, float *d_gain,
                                          hipStream_t st) {
    const int G = (int)p.segs.size();
    const int64_t P = p.packed_elems;
    const dim3 grid = launch_delivery_peaks(x, p, d_segs, d_peak, st);
    limit_gain_kernel<<<dim3((unsigned)((P + kLimitTile - 1) / kLimitTile)), kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, d_shapes, d_knots,
                                                                                                        d_limits, d_gain);
    uint4 *out = static_cast<uint4 *>(d_packed);
#define VITSMI_LIMITED(ENC) \
    delivery_pack_limited_kernel<ENC><<<grid, kDeliveryThreads, 0, st>>>(x, d_segs, G, d_peak, P, out, d_shapes, d_knots, d_limits, d_gain)
    switch (p.encoding) {
        case VITS_ENC_PCM16: VITSMI_LIMITED(VITS_ENC_PCM16); break;
        case VITS_ENC_ULAW: VITSMI_LIMITED(VITS_ENC_ULAW); break;
        case VITS_ENC_ALAW: VITSMI_LIMITED(VITS_ENC_ALAW); break;
        default: VITSMI_LIMITED(VITS_ENC_F32); break;
    }
#undef VITSMI_LIMITED
    return hipGetLastError();
}

}  // namespace vitsmi
