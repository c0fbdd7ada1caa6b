// stream_pack.hip.hpp — the kernel of an encoded stream (include/vitsmi.h, "encoded streaming").
//
// One launch per chunk.  A chunk is rectangular: B rows of n samples starting at `first`, row b at x + b * x_pitch, of which
// clamp(n_b - first, 0, n) are valid; n_b comes from a device array the run already holds (frame counts times hop, or the
// resampler's output counts) or is one number for every row.  So there is no segment table and no search: grid (cells of a
// row / 256, B), a workgroup owns 256 cells of 16 output bytes of ONE row.  Every lane loads element base + i * 256 + lane of
// the tile (coalesced fp32, nothing assumed about the source's alignment beyond 4 bytes), folds |x| into its running maximum,
// runs the delivery's sample functions (delivery.hip.hpp: the single definition) and parks the element in LDS; behind the
// row's valid count it parks the encoding of 0 without loading.  After the barrier each lane stores its 16-byte cell, silence
// cells included, so the host never patches a chunk.  The peak goes through a wave reduction and one atomicMax on the float
// bits per wave into peak_run[b] (zeroed once per run: the running peak over the chunks so far).
//
// The chunk buffer: [B][pitch] bytes and, right behind them at a 16-byte-aligned offset, the B running peaks, so that one
// copy carries both.  The peaks stay where they are for the whole run (workspace.hpp, carve_stream_pack): a chunk's bytes END
// at them, whatever its pitch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "delivery.hip.hpp"

namespace vitsmi {

// the rows' valid sample counts: len[b] * mul (clamped to [0, all]) or, without len, `all` for every row
struct StreamPackRows {
    const int *len;
    int mul;
    int all;
};

// fmt [B][2]: {ref_peak, volume}
template <int ENC>
__global__ __launch_bounds__(kDeliveryThreads) void stream_pack_kernel(const float *x, int64_t x_pitch, StreamPackRows rows, int first,
                                                                       int n, const float *fmt, int norm, uint4 *bytes,
                                                                       int cells_per_row, unsigned *peak_run) {
    using T = typename DeliveryElem<ENC>::type;
    constexpr int E = 16 / (int)sizeof(T);
    __shared__ uint4 tile[kDeliveryThreads];
    T *lt = reinterpret_cast<T *>(tile);
    const int b = blockIdx.y;
    int64_t nb = rows.len ? (int64_t)rows.len[b] * rows.mul : rows.all;
    nb = nb > rows.all ? rows.all : nb;
    int64_t vl = nb - first;
    const int valid = vl < 0 ? 0 : (vl > n ? n : (int)vl);
    const float ref = fmt[2 * b], volume = fmt[2 * b + 1];
    const float *xr = x + (int64_t)b * x_pitch;
    const T silence = delivery_encode<ENC>(delivery_value(0.0f, false, 1.0f, 1.0f));
    const int base = blockIdx.x * (kDeliveryThreads * E);  // (elements of a row: below 2^31 with the cell count)
    float m = 0.f;
#pragma unroll 4
    for (int i = 0; i < E; i++) {
        const int e = base + i * kDeliveryThreads + (int)threadIdx.x;
        T o = silence;
        if (e < valid) {
            const float v = xr[e];
            m = fmaxf(m, fabsf(v));
            o = delivery_encode<ENC>(delivery_value(v, norm != 0, ref, volume));
        }
        lt[i * kDeliveryThreads + threadIdx.x] = o;
    }
    __syncthreads();
    const int cell = blockIdx.x * kDeliveryThreads + (int)threadIdx.x;
    if (cell < cells_per_row) bytes[(int64_t)b * cells_per_row + cell] = tile[threadIdx.x];
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(&peak_run[b], __float_as_uint(m));  // non-negative floats order as uints
}

// row pitch of a chunk of n samples at w bytes per element
inline int64_t stream_pack_pitch(int width, int64_t n) { return (width * n + 15) & ~(int64_t)15; }

// f(std::integral_constant<int, ENC>) for a (validated) encoding: the kernels' template argument
template <class F>
inline void stream_for_encoding(int encoding, F &&f) {
    switch (encoding) {
        case VITS_ENC_PCM16: return f(std::integral_constant<int, VITS_ENC_PCM16>{});
        case VITS_ENC_ULAW: return f(std::integral_constant<int, VITS_ENC_ULAW>{});
        case VITS_ENC_ALAW: return f(std::integral_constant<int, VITS_ENC_ALAW>{});
        default: return f(std::integral_constant<int, VITS_ENC_F32>{});
    }
}

// one chunk on `st`: bytes [B][pitch] (16-byte aligned), pitch = stream_pack_pitch(width of encoding, n); n >= 1
inline hipError_t launch_stream_pack(int encoding, const float *x, int64_t x_pitch, const StreamPackRows &rows, int B, int first, int n,
                                     const float *fmt, bool norm, void *bytes, unsigned *peak_run, hipStream_t st) {
    const int width = delivery_width(encoding);
    const int cells = (int)(stream_pack_pitch(width, n) / 16);
    const dim3 grid((unsigned)((cells + kDeliveryThreads - 1) / kDeliveryThreads), (unsigned)B);
    uint4 *out = static_cast<uint4 *>(bytes);
    const int nm = norm ? 1 : 0;
    stream_for_encoding(encoding, [&](auto enc) {
        stream_pack_kernel<decltype(enc)::value><<<grid, kDeliveryThreads, 0, st>>>(x, x_pitch, rows, first, n, fmt, nm, out, cells, peak_run);
    });
    return hipGetLastError();
}

}  // namespace vitsmi
