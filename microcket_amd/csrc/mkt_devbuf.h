// mkt_devbuf.h -- who frees device memory, pinned host memory, events and streams: a move-only owner per allocation, and the one
// early return on a HIP error.  A struct of owners is released by `s = S()` or with the struct; a function that fails half way
// leaks nothing.  Used by the matrix analyses, the contexts of the C ABI, sam2bam, the sorter and rmdup.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

namespace mkt {

#define MKT_TRY(call) do { hipError_t mkt_e_ = (call); if (mkt_e_ != hipSuccess) return mkt_e_; } while (0)

struct DevMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};

template <typename T, typename M>
class OwnBuf {
    T* p_ = nullptr;

public:
    OwnBuf() = default;
    OwnBuf(const OwnBuf&) = delete;
    OwnBuf& operator=(const OwnBuf&) = delete;
    OwnBuf(OwnBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    OwnBuf& operator=(OwnBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    ~OwnBuf() { reset(); }
    // n elements and pad_bytes behind them; what was held is freed first
    hipError_t alloc(size_t n, size_t pad_bytes = 0) {
        reset();
        const hipError_t e = M::alloc((void**)&p_, n * sizeof(T) + pad_bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void adopt(T* p) { reset(); p_ = p; }            // memory that another module allocated for its caller
    void reset() {
        if (p_) M::free(p_);
        p_ = nullptr;
    }
    T* release() { T* p = p_; p_ = nullptr; return p; }      // the caller frees
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};
template <typename T> using DevBuf = OwnBuf<T, DevMem>;
template <typename T> using PinBuf = OwnBuf<T, PinMem>;

// A buffer that knows how many elements it holds room for.  No policy: the caller says how much to allocate (its slack formula)
// and whether anything has to be idle first.
template <typename T, typename M = DevMem>
class GrowBuf {
    OwnBuf<T, M> b_;
    size_t cap_ = 0;

public:
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : b_(std::move(o.b_)), cap_(o.cap_) { o.cap_ = 0; }
    GrowBuf& operator=(GrowBuf&& o) noexcept {
        if (this != &o) { b_ = std::move(o.b_); cap_ = o.cap_; o.cap_ = 0; }
        return *this;
    }
    bool fits(size_t n) const { return n <= cap_; }
    size_t cap() const { return cap_; }
    // contents dropped: free, then allocate; a failure leaves the buffer empty
    hipError_t regrow(size_t new_cap) {
        cap_ = 0;
        MKT_TRY(b_.alloc(new_cap));
        cap_ = new_cap;
        return hipSuccess;
    }
    // the first `keep` elements carried over (device memory, nothing queued on it): allocate, copy, then free; a failure leaves
    // the buffer as it was
    hipError_t regrow_keep(size_t new_cap, size_t keep) {
        OwnBuf<T, M> nb;
        MKT_TRY(nb.alloc(new_cap));
        if (keep) MKT_TRY(hipMemcpy(nb.get(), b_.get(), keep * sizeof(T), hipMemcpyDeviceToDevice));
        b_ = std::move(nb);
        cap_ = new_cap;
        return hipSuccess;
    }
    void reset() { b_.reset(); cap_ = 0; }
    T* get() const { return b_.get(); }
    operator T*() const { return b_.get(); }
};
template <typename T> using PinGrowBuf = GrowBuf<T, PinMem>;

// Device bytes that one object holds, where that sum decides something (sam2bam spills by it: DESIGN.md 6c).  limit 0: none.
struct DevLedger { size_t now = 0, peak = 0, limit = 0; };
// An owner whose bytes (the caller's formula, pads included) are charged to a ledger on allocation or adoption and credited on release.
template <typename T>
class LedgerBuf {
    DevLedger* l_ = nullptr;
    T* p_ = nullptr;
    size_t bytes_ = 0;
    void take(DevLedger& l, T* p, size_t bytes) { l_ = &l; p_ = p; bytes_ = bytes; l.now += bytes; if (l.now > l.peak) l.peak = l.now; }

public:
    LedgerBuf() = default;
    LedgerBuf(const LedgerBuf&) = delete;
    LedgerBuf& operator=(const LedgerBuf&) = delete;
    LedgerBuf(LedgerBuf&& o) noexcept : l_(o.l_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    LedgerBuf& operator=(LedgerBuf&& o) noexcept {
        if (this != &o) { reset(); l_ = o.l_; p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~LedgerBuf() { reset(); }
    // what was held is released first.  Refused with hipErrorOutOfMemory BEFORE any hipMalloc where the ledger's limit would be
    // exceeded; a hipMalloc that fails leaves no pending error.  Either way the buffer is empty afterwards.
    hipError_t alloc(DevLedger& l, size_t bytes) {
        reset();
        if (l.limit && l.now + bytes > l.limit) return hipErrorOutOfMemory;
        T* p = nullptr;
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        take(l, p, bytes);
        return hipSuccess;
    }
    // a buffer that only grows, contents not kept: nothing when `bytes` fit, else alloc
    hipError_t grow(DevLedger& l, size_t bytes) { return p_ && bytes <= bytes_ ? hipSuccess : alloc(l, bytes); }
    void adopt(DevLedger& l, T* p, size_t bytes) { reset(); take(l, p, bytes); }      // memory that another module allocated for its caller
    void reset() { if (p_) { l_->now -= bytes_; (void)hipFree(p_); } p_ = nullptr; bytes_ = 0; }
    size_t bytes() const { return bytes_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};

// the same for the events a call times its phases with (flags 0: hipEventCreate)
template <int N>
struct DevEvents {
    hipEvent_t ev[N] = {};
    DevEvents() = default;
    DevEvents(const DevEvents&) = delete;
    DevEvents& operator=(const DevEvents&) = delete;
    ~DevEvents() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create(int i, unsigned flags) { return flags ? hipEventCreateWithFlags(&ev[i], flags) : hipEventCreate(&ev[i]); }
    hipError_t create() {
        for (int i = 0; i < N; ++i) MKT_TRY(create(i, 0));
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return ev[i]; }
};

// ... and for a stream
struct DevStream {
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
    operator hipStream_t() const { return s; }
};

}  // namespace mkt
