// loudness.hip.hpp — the kernels of a levelled delivery (include/vitsmi.h, "levelled delivery"; the host side: loudness.hpp):
// the K-weighted energy of every 100 ms sub-block of the kept range of every levelled segment.
//
// The two biquads are a linear recurrence with four state values: one lane per row would walk a row's samples one after the
// other.  The kept range is therefore cut into chunks of kLoudChunk samples, counted from its first sample, and the work
// becomes four small launches over a table of the levelled segments only (LoudSeg; unlevelled segments launch nothing):
//   loudness_state_kernel   a lane per chunk that has a successor: the recurrence from rest, its final state -> fin
//   loudness_carry_kernel   a lane per segment: init[0] = 0, init[c + 1] = M init[c] + fin[c] - the true state in front of
//                           every chunk; M is the 4x4 transition over kLoudChunk samples (built in double on the host)
//   loudness_energy_kernel  a lane per chunk: the recurrence again from init[c]; y^2 summed per sub-block in sample order,
//                           one partial sum per sub-block the chunk touches (at most kLoudParts) -> part
//   loudness_fold_kernel    a lane per sub-block: its partial sums added in ascending chunk order -> e
// No atomics and no order left to the hardware: e is bit-identical from call to call, and - every index above being relative
// to the segment's own first sample and its own slots - depends on the row's kept samples alone.  Nothing assumes an
// alignment of src.  Only whole sub-blocks count: a segment's n is n_sub * hop, what lies behind is not read.
//
// A lane walks its own chunk, so the 64 lanes of a wave touch 64 cache lines per load; a workgroup is one wave so that the
// chunks spread over the chip.  The kernels are bound by the dependent chain of a chunk, not by data: measured, with what was
// tried and what was not, in DESIGN.md 5.11.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "loudness.hpp"

namespace vitsmi {

constexpr int kLoudThreads = 64;
// samples (chunk kernels) and chunk states (carry kernel) a lane loads before it walks them: the recurrence is one dependent
// chain, so a load issued inside it would cost its whole latency per step
constexpr int kLoudBatch = 16, kLoudCarryBatch = 8;
static_assert(kLoudChunk % kLoudBatch == 0, "a chunk is whole batches");

// one sample through the two biquads, transposed direct form II (loudness.hpp, loudness_step, in fp32; the fused
// multiply-adds are written out so that every build rounds alike)
__device__ inline float loud_step(const LoudCoef &k, float x, LoudState &z) {
    const float y1 = fmaf(k.c[0], x, z.x);
    z.x = fmaf(-k.c[3], y1, fmaf(k.c[1], x, z.y));
    z.y = fmaf(-k.c[4], y1, k.c[2] * x);
    const float y = fmaf(k.c[5], y1, z.z);
    z.z = fmaf(-k.c[8], y, fmaf(k.c[6], y1, z.w));
    z.w = fmaf(-k.c[9], y, k.c[7] * y1);
    return y;
}

// grid (gx, G): chunk blockIdx.x * 64 + lane of segment blockIdx.y
__global__ __launch_bounds__(kLoudThreads) void loudness_state_kernel(const float *__restrict__ x, const LoudSeg *__restrict__ segs, LoudCoef k,
                                                                      LoudState *__restrict__ fin) {
    const LoudSeg s = segs[blockIdx.y];
    const int64_t c = (int64_t)blockIdx.x * kLoudThreads + threadIdx.x;
    if ((c + 1) * kLoudChunk >= s.n) return;  // (no chunk behind this one: nobody reads its final state)
    const float *p = x + s.src + c * kLoudChunk;
    LoudState z = LoudState{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < kLoudChunk; i += kLoudBatch) {
        float v[kLoudBatch];  // (all loads of a batch in flight before the first dependent step)
#pragma unroll
        for (int u = 0; u < kLoudBatch; u++) v[u] = p[i + u];
#pragma unroll
        for (int u = 0; u < kLoudBatch; u++) loud_step(k, v[u], z);
    }
    fin[s.chunk0 + c] = z;
}

// grid ceil(G / 64): a lane per segment
__global__ __launch_bounds__(kLoudThreads) void loudness_carry_kernel(const LoudSeg *__restrict__ segs, int G, LoudCoef k,
                                                                      const LoudState *__restrict__ fin, LoudState *__restrict__ init) {
    const int g = blockIdx.x * kLoudThreads + threadIdx.x;
    if (g >= G) return;
    const LoudSeg s = segs[g];
    const int64_t nch = ((int64_t)s.n + kLoudChunk - 1) / kLoudChunk;
    LoudState z = LoudState{0.f, 0.f, 0.f, 0.f};
    for (int64_t c = 0; c + 1 < nch; c += kLoudCarryBatch) {
        LoudState f[kLoudCarryBatch];
#pragma unroll
        for (int u = 0; u < kLoudCarryBatch; u++)
            if (c + u + 1 < nch) f[u] = fin[s.chunk0 + c + u];
#pragma unroll
        for (int u = 0; u < kLoudCarryBatch; u++) {
            if (c + u + 1 >= nch) break;
            init[s.chunk0 + c + u] = z;
            LoudState t;
            t.x = fmaf(k.m[0], z.x, fmaf(k.m[1], z.y, fmaf(k.m[2], z.z, fmaf(k.m[3], z.w, f[u].x))));
            t.y = fmaf(k.m[4], z.x, fmaf(k.m[5], z.y, fmaf(k.m[6], z.z, fmaf(k.m[7], z.w, f[u].y))));
            t.z = fmaf(k.m[8], z.x, fmaf(k.m[9], z.y, fmaf(k.m[10], z.z, fmaf(k.m[11], z.w, f[u].z))));
            t.w = fmaf(k.m[12], z.x, fmaf(k.m[13], z.y, fmaf(k.m[14], z.z, fmaf(k.m[15], z.w, f[u].w))));
            z = t;
        }
    }
    if (nch > 0) init[s.chunk0 + nch - 1] = z;
}

// grid (gx, G) as loudness_state_kernel.  A chunk's samples [i0, i0 + len) lie in the sub-blocks i0 / hop ...; partial sum
// j of the chunk belongs to sub-block i0 / hop + j.
__global__ __launch_bounds__(kLoudThreads) void loudness_energy_kernel(const float *__restrict__ x, const LoudSeg *__restrict__ segs, LoudCoef k,
                                                                       const LoudState *__restrict__ init, float *__restrict__ part) {
    const LoudSeg s = segs[blockIdx.y];
    const int64_t c = (int64_t)blockIdx.x * kLoudThreads + threadIdx.x;
    const int64_t i0 = c * kLoudChunk;
    if (i0 >= s.n) return;
    const int len = s.n - i0 < kLoudChunk ? (int)(s.n - i0) : kLoudChunk;
    const float *p = x + s.src + i0;
    float *out = part + (s.chunk0 + c) * kLoudParts;
    LoudState z = init[s.chunk0 + c];
    int next = (int)((i0 / k.hop + 1) * k.hop - i0);  // the chunk's first sample of the next sub-block
    int slot = 0;
    float acc = 0.f;
    // sub-block by sub-block: whole batches without a test inside, then one batch cut at the sub-block's (or the chunk's) end
    for (int i = 0; i < len;) {
        const int end = next < len ? next : len;
        for (; i + kLoudBatch <= end; i += kLoudBatch) {
            float v[kLoudBatch];
#pragma unroll
            for (int u = 0; u < kLoudBatch; u++) v[u] = p[i + u];
#pragma unroll
            for (int u = 0; u < kLoudBatch; u++) {
                const float y = loud_step(k, v[u], z);
                acc = fmaf(y, y, acc);
            }
        }
        if (i < end) {
            float v[kLoudBatch];
#pragma unroll
            for (int u = 0; u < kLoudBatch; u++) v[u] = i + u < end ? p[i + u] : 0.f;
#pragma unroll
            for (int u = 0; u < kLoudBatch; u++) {
                if (i + u >= end) break;
                const float y = loud_step(k, v[u], z);
                acc = fmaf(y, y, acc);
            }
            i = end;
        }
        if (i < len) {  // (hop >= kLoudMinHop: at most kLoudParts - 1 times a chunk)
            out[slot++] = acc;
            acc = 0.f;
            next += k.hop;
        }
    }
    out[slot] = acc;
}

// grid (gx, G): sub-block blockIdx.x * 64 + lane of segment blockIdx.y
__global__ __launch_bounds__(kLoudThreads) void loudness_fold_kernel(const LoudSeg *__restrict__ segs, LoudCoef k, const float *__restrict__ part,
                                                                     float *__restrict__ e) {
    const LoudSeg s = segs[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * kLoudThreads + threadIdx.x;
    if ((j + 1) * k.hop > s.n) return;
    const int64_t c0 = j * k.hop / kLoudChunk, c1 = ((j + 1) * k.hop - 1) / kLoudChunk;
    float sum = 0.f;
    for (int64_t c = c0; c <= c1; c++) sum += part[(s.chunk0 + c) * kLoudParts + (j - c * kLoudChunk / k.hop)];
    e[s.sub0 + j] = sum;
}

// the four launches on `st`: d_segs [G] levelled segments, the longest of max_n samples (> 0); k.hop >= kLoudMinHop
inline hipError_t launch_loudness(const float *x, const LoudSeg *d_segs, int G, int max_n, const LoudCoef &k, LoudState *d_fin, LoudState *d_init,
                                  float *d_part, float *d_e, hipStream_t st) {
    const int nch = (max_n + kLoudChunk - 1) / kLoudChunk, nsub = max_n / k.hop;
    const dim3 gc((nch + kLoudThreads - 1) / kLoudThreads, G), gs((nsub + kLoudThreads - 1) / kLoudThreads, G);
    if (nch > 1) loudness_state_kernel<<<gc, kLoudThreads, 0, st>>>(x, d_segs, k, d_fin);
    loudness_carry_kernel<<<(G + kLoudThreads - 1) / kLoudThreads, kLoudThreads, 0, st>>>(d_segs, G, k, d_fin, d_init);
    loudness_energy_kernel<<<gc, kLoudThreads, 0, st>>>(x, d_segs, k, d_init, d_part);
    if (nsub > 0) loudness_fold_kernel<<<gs, kLoudThreads, 0, st>>>(d_segs, k, d_part, d_e);
    return hipGetLastError();
}

}  // namespace vitsmi
