// test_dev.hip.hpp — what the kernel-level test hooks (vitsmi.hip, g2p.hip) share on the host side: an owner of their
// device buffers and one event timer.  Nothing here runs on the device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace vitsmi {

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
