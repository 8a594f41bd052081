// dev_buf.hpp -- the one owner of a device allocation (DevBuf) and the one way to cut it into planes (Carve) in geosrad.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace geosrad {

// Movable, not copyable; frees in its destructor, so the device it was allocated on must be current when it dies (geosrad_destroy and
// ~MultiCtx see to that).  `bytes` is what is allocated; a failed call leaves the buffer empty.  Converts to T * like the raw pointer
// it replaces.  The call site turns the hipError_t into its own message and error code.
template <typename T = char> struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    // exactly n bytes, the old allocation freed first
    hipError_t resize(size_t n)
    {
        release();
        const hipError_t e = hipMalloc((void **)&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    // at least n bytes: grow-only, a smaller request keeps the allocation
    hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : resize(n); }
    operator T *() const { return p; }
};

// Hands out consecutive pieces of one allocation as typed pointers, each starting on a 256-byte boundary of it.  Without a base it only
// measures: every take returns null, and `off` ends as the bytes the same sequence of takes needs (a zero-count take has an address but
// no bytes).  A layout is one function of a Carve, run once on Carve() to size the allocation and once on Carve(buffer) to address it.
struct Carve {
    char *base;
    size_t off = 0;
    explicit Carve(void *b = nullptr) : base((char *)b) {}
    template <typename T> T *take(size_t count)
    {
        const size_t o = off;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return base ? (T *)(base + o) : nullptr;
    }
};

}  // namespace geosrad
