// devbuf.h -- DevBuf: one device allocation that grows on demand and frees itself.  Host code only (the HIP runtime API and
// the standard library), so a host compiler builds it alone (tools/devbuf_check.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace dabgpu_api {

// Move-only; a moved-from buffer is empty.  The destructor frees on whichever device is current: the owner makes the
// allocation's device current first (dabgpu_destroy does, before it deletes the context).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }

    // at least n bytes; the contents are NOT preserved when it grows.  On failure the buffer is empty.
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace dabgpu_api
