// test_dev.hip.hpp — what the kernel-level test hooks (vitsmi.hip, g2p.hip) share on the host side: an owner of their
// device buffers and one event timer - and one kernel, which applies the device helpers of sx_split.hip.hpp to an array.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "sx_split.hip.hpp"

namespace vitsmi {

// The activation -> operand-plane path of the fused ResBlock-step kernel on an array, helper by helper as that kernel calls them:
// a = lrelu_max(x, slope), then FORM 0: split2h_pair_pk (the engine-wide form), FORM 1: sx_pair_split (conv_sx_pair_kernel's).
// Pair i = elements 2 i, 2 i + 1 (n even).  Out: the two planes' fp16 bits per element, the guard magnitude per pair, and the
// reconstruction of the high plane (unact4h with unslope: what a consumer of activated planes recovers), per element.
template <int FORM>
__global__ void split_forms_kernel(const float *x, int n, float slope, float unslope, uint16_t *h0, uint16_t *h1, float *pk_out, float *rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * i + 1 >= n) return;
    const float a = lrelu_max(x[2 * i], slope), b = lrelu_max(x[2 * i + 1], slope);
    unsigned w0, w1;
    float pk = 0.f;
    if constexpr (FORM == 0) split2h_pair_pk(a, b, w0, w1, pk);
    else sx_pair_split(a, b, w0, w1, pk);
    h0[2 * i] = (uint16_t)(w0 & 0xffffu);
    h0[2 * i + 1] = (uint16_t)(w0 >> 16);
    h1[2 * i] = (uint16_t)(w1 & 0xffffu);
    h1[2 * i + 1] = (uint16_t)(w1 >> 16);
    pk_out[i] = pk;
    float o[4];
    unact4h(u32x2{w0, w0}, unslope, o);
    rec[2 * i] = o[0];
    rec[2 * i + 1] = o[1];
}

// Owner of a hook's device buffers: whatever it handed out is freed when it goes out of scope, whichever way the hook
// returns.  The first failure stays in `err`; every call after it does nothing and returns nullptr, so a hook asks for all
// its buffers and checks once.  Sizes are in elements of T; `pad` bytes are added to the allocation only (the slack some
// kernels' whole-cell loads read behind a tensor's end).
struct DevBufs {
    std::vector<void *> p;
    hipError_t err = hipSuccess;
    DevBufs() = default;
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs() {
        for (void *q : p) hipFree(q);
    }
    bool ok() const { return err == hipSuccess; }
    template <class T>
    T *alloc(size_t n, size_t pad = 0) {  // uninitialised
        if (!ok()) return nullptr;
        void *d = nullptr;
        const size_t bytes = n * sizeof(T) + pad;
        err = hipMalloc(&d, bytes ? bytes : 1);
        if (!ok()) return nullptr;
        p.push_back(d);
        return static_cast<T *>(d);
    }
    template <class T>
    T *fill(size_t n, int byte = 0, size_t pad = 0) {  // the n elements set to `byte`
        T *d = alloc<T>(n, pad);
        if (d && n) err = hipMemset(d, byte, n * sizeof(T));
        return d;
    }
    template <class T>
    T *up(const T *host, size_t n, size_t pad = 0) {  // a copy of host[0..n)
        T *d = alloc<T>(n, pad);
        if (d && n) err = hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
};

template <class T>
inline hipError_t download(T *host, const T *dev, size_t n) {
    return hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
}

// Milliseconds per launch of n back-to-back launches on the null stream, between two events.  `launch` returns a
// hipError_t; the first failure ends the loop and is returned.
template <class F>
hipError_t time_launches(int n, F &&launch, float *ms_per_launch) {
    struct Event {
        hipEvent_t e = nullptr;
        hipError_t err;
        Event() : err(hipEventCreate(&e)) {}
        ~Event() {
            if (e) hipEventDestroy(e);
        }
    } e0, e1;
    hipError_t err = e0.err != hipSuccess ? e0.err : e1.err;
    if (err == hipSuccess) err = hipEventRecord(e0.e, nullptr);
    for (int i = 0; i < n && err == hipSuccess; i++) err = launch();
    if (err == hipSuccess) err = hipEventRecord(e1.e, nullptr);
    if (err == hipSuccess) err = hipEventSynchronize(e1.e);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0.e, e1.e);
    if (err == hipSuccess) *ms_per_launch = ms / (float)n;
    return err;
}

}  // namespace vitsmi
