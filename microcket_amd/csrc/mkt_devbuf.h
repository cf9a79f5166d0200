// mkt_devbuf.h -- who frees device memory in the matrix analyses: a move-only owner per allocation, and the one early return on a
// HIP error.  A struct of DevBufs is released by `s = S()`; a function that fails half way leaks nothing.  DESIGN.md 7f.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mkt {

#define MKT_TRY(call) do { hipError_t mkt_e_ = (call); if (mkt_e_ != hipSuccess) return mkt_e_; } while (0)

template <typename T>
class DevBuf {
    T* p_ = nullptr;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // n elements and pad_bytes behind them; what was held is freed first
    hipError_t alloc(size_t n, size_t pad_bytes = 0) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T) + pad_bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void adopt(T* p) { reset(); p_ = p; }            // memory that another module hipMalloc'ed for its caller
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};

// the same for the events a call times its phases with
template <int N>
struct DevEvents {
    hipEvent_t ev[N] = {};
    DevEvents() = default;
    DevEvents(const DevEvents&) = delete;
    DevEvents& operator=(const DevEvents&) = delete;
    ~DevEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create() {
        for (hipEvent_t& e : ev) MKT_TRY(hipEventCreate(&e));
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
};

}  // namespace mkt
