// slab.hpp — the bump allocator every device workspace is carved with.  Host-side C++17, no HIP types.
//
// A workspace is stated ONCE, as the walk that carves it: a function that calls take() for every buffer, in order.  Run
// over a Carver without a base (a dry walk) it only counts, and `used` afterwards IS the size of the workspace; run with
// the same arguments over the allocated slab it hands out the pointers.  fits() after the real walk, before any launch,
// is the bound check: it cannot fail while both walks are one function, and turns a later mistake into an error return
// instead of a write past the allocation.
#pragma once
#include <cstddef>

namespace vitsmi {

struct Carver {
    char *base = nullptr;  // nullptr: a dry walk
    size_t cap = 0, used = 0;
    Carver() = default;
    Carver(void *b, size_t c) : base(static_cast<char *>(b)), cap(c) {}
    // n elements of T at the next 256-byte boundary (nullptr on a dry walk)
    template <class T>
    T *take(size_t n) {
        const size_t off = (used + 255) & ~size_t(255);
        used = off + n * sizeof(T);
        return base ? reinterpret_cast<T *>(base + off) : nullptr;
    }
    // what is carved behind a mark may be carved again after rewind(mark): the chunked renderer's per-chunk reuse
    size_t mark() const { return used; }
    void rewind(size_t m) { used = m; }
    bool fits() const { return used <= cap; }
};

// the size of the workspace a walk carves: `used` after a dry run of it
template <class Walk>
size_t carved_bytes(Walk &&walk) {
    Carver dry;
    walk(dry);
    return dry.used;
}

}  // namespace vitsmi
