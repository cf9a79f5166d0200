// devbuf_check.cpp -- the owning buffer types of microcket_amd/csrc/mkt_devbuf.h on a real device: growth with and without the
// contents kept, failed allocations, moves, release(), the pinned counterparts, and the ledger-charged owner.  One line per check; the first failed check ends the
// program with status 1 (nothing further is started on the device).  tests/test_gpu_devbuf.py runs it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include <vector>
#include "../../microcket_amd/csrc/mkt_devbuf.h"

using namespace mkt;

static int g_checks = 0;
static void check(bool ok, const char* what) {
    printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    fflush(stdout);
    if (!ok) exit(1);
    ++g_checks;
}
static void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) { printf("FAIL %s: %s\n", what, hipGetErrorString(e)); fflush(stdout); exit(1); }
}

static const size_t kHuge = ((size_t)1 << 60) / sizeof(uint64_t);       // 2^60 bytes: the runtime says out of memory, no device work
static std::vector<uint64_t> pattern(size_t n) {
    std::vector<uint64_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (uint64_t)i * 0x9E3779B97F4A7C15ull;
    return v;
}
static bool holds(const uint64_t* d, const std::vector<uint64_t>& want) {
    std::vector<uint64_t> got(want.size());
    hip_ok(hipMemcpy(got.data(), d, want.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "read back");
    return got == want;
}
// what a context does before it uses a buffer: nothing when it fits, else a new one
template <typename B>
static hipError_t ensure(B& b, size_t need, size_t new_cap) { return b.fits(need) ? hipSuccess : b.regrow(new_cap); }

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { printf("FAIL no HIP device\n"); return 1; }
    hip_ok(hipSetDevice(0), "hipSetDevice");
    const std::vector<uint64_t> pat = pattern(1000);
    {   // growth, contents kept
        GrowBuf<uint64_t> b;
        check(b.get() == nullptr && b.cap() == 0 && b.fits(0) && !b.fits(1), "a new buffer is empty");
        hip_ok(b.regrow(1000), "regrow(1000)");
        check(b.get() != nullptr && b.cap() == 1000, "regrow(1000): capacity 1000");
        hip_ok(hipMemcpy(b.get(), pat.data(), 1000 * sizeof(uint64_t), hipMemcpyHostToDevice), "upload");
        uint64_t* before = b.get();
        check(b.fits(1) && b.fits(1000) && !b.fits(1001), "fits(n) exactly for n <= capacity");
        hip_ok(ensure(b, 1000, 4000), "ensure of what fits");
        check(b.get() == before && b.cap() == 1000, "an ensure of what fits reallocates nothing");
        hip_ok(b.regrow_keep(2000, 1000), "regrow_keep(2000, 1000)");
        check(b.get() != before && b.cap() == 2000, "regrow_keep(2000, 1000): new pointer, capacity 2000");
        check(holds(b.get(), pat), "regrow_keep(2000, 1000): the first 1000 elements are identical");
        // a failed regrow_keep changes nothing
        before = b.get();
        const hipError_t e = b.regrow_keep(kHuge, 1000);
        (void)hipGetLastError();
        check(e == hipErrorOutOfMemory, "regrow_keep of 2^60 bytes: out of memory");
        check(b.get() == before && b.cap() == 2000 && holds(b.get(), pat), "after it the old pointer, capacity and contents are intact");
        // growth, contents dropped
        hip_ok(b.regrow(3000), "regrow(3000)");
        check(b.get() != nullptr && b.cap() == 3000 && b.fits(3000), "regrow of a larger size updates the capacity");
        const hipError_t e2 = b.regrow(kHuge);
        (void)hipGetLastError();
        check(e2 == hipErrorOutOfMemory, "regrow of 2^60 bytes: out of memory");
        check(b.get() == nullptr && b.cap() == 0 && !b.fits(1), "after it the buffer is empty with capacity 0");
        hip_ok(ensure(b, 10, 16), "ensure after the failure");
        check(b.get() != nullptr && b.cap() == 16, "an ensure of an emptied buffer allocates");
    }
    {   // the edges of regrow_keep
        GrowBuf<uint64_t> b;
        hip_ok(b.regrow_keep(500, 0), "regrow_keep(500, 0)");
        check(b.get() != nullptr && b.cap() == 500, "regrow_keep on an empty buffer with keep = 0 succeeds");
        hip_ok(hipMemcpy(b.get(), pat.data(), 500 * sizeof(uint64_t), hipMemcpyHostToDevice), "upload");
        hip_ok(b.regrow_keep(1000, 500), "regrow_keep(1000, 500)");
        check(b.cap() == 1000 && holds(b.get(), std::vector<uint64_t>(pat.begin(), pat.begin() + 500)), "regrow_keep with keep = the old capacity keeps all of it");
    }
    {   // DevBuf: a failed alloc leaves it empty
        DevBuf<uint64_t> d;
        hip_ok(d.alloc(64), "DevBuf::alloc(64)");
        const hipError_t e = d.alloc(kHuge);
        (void)hipGetLastError();
        check(e == hipErrorOutOfMemory && d.get() == nullptr, "DevBuf::alloc of 2^60 bytes: out of memory, the buffer empty");
    }
    {   // ownership
        GrowBuf<uint64_t> a;
        hip_ok(a.regrow(1000), "regrow(1000)");
        hip_ok(hipMemcpy(a.get(), pat.data(), 1000 * sizeof(uint64_t), hipMemcpyHostToDevice), "upload");
        uint64_t* p = a.get();
        GrowBuf<uint64_t> b(std::move(a));
        check(b.get() == p && b.cap() == 1000 && a.get() == nullptr && a.cap() == 0, "move-construction transfers, the source is empty with capacity 0");
        GrowBuf<uint64_t> c;
        hip_ok(c.regrow(8), "regrow(8)");
        c = std::move(b);
        check(c.get() == p && c.cap() == 1000 && b.get() == nullptr && b.cap() == 0, "move-assignment transfers, the source is empty with capacity 0");
        GrowBuf<uint64_t>& self = c;
        c = std::move(self);
        check(c.get() == p && c.cap() == 1000 && holds(c.get(), pat), "self-move-assignment is harmless");
        DevBuf<uint64_t> d;
        hip_ok(d.alloc(8), "DevBuf::alloc(8)");
        uint64_t* q = d.get();
        DevBuf<uint64_t> e(std::move(d));
        DevBuf<uint64_t>& eself = e;
        e = std::move(eself);
        check(e.get() == q && d.get() == nullptr, "DevBuf: moves transfer, a self-move is harmless");
        // release: the pointer is the caller's from then on
        hip_ok(hipMemcpy(q, pat.data(), 8 * sizeof(uint64_t), hipMemcpyHostToDevice), "upload");
        uint64_t* r = e.release();
        check(r == q && e.get() == nullptr, "DevBuf::release hands the pointer over, the owner is empty");
        e.reset();
        e = DevBuf<uint64_t>();
        check(holds(r, std::vector<uint64_t>(pat.begin(), pat.begin() + 8)), "after release, reset and reassignment of the owner the memory is still valid");
        check(hipFree(r) == hipSuccess, "the caller frees what was released (the owner did not)");
    }
    {   // pinned host memory: allocate, use, grow, move (no failure request: a modest one that succeeds)
        PinGrowBuf<uint64_t> h;
        check(h.get() == nullptr && h.cap() == 0, "a new pinned buffer is empty");
        hip_ok(h.regrow(1000), "pinned regrow(1000)");
        check(h.get() != nullptr && h.cap() == 1000 && h.fits(1000) && !h.fits(1001), "pinned regrow(1000): capacity 1000");
        GrowBuf<uint64_t> d;
        hip_ok(d.regrow(1000), "regrow(1000)");
        hip_ok(hipMemcpy(d.get(), pat.data(), 1000 * sizeof(uint64_t), hipMemcpyHostToDevice), "upload");
        hip_ok(hipMemcpy(h.get(), d.get(), 1000 * sizeof(uint64_t), hipMemcpyDeviceToHost), "copy into pinned memory");
        check(memcmp(h.get(), pat.data(), 1000 * sizeof(uint64_t)) == 0, "pinned memory takes a device copy");
        uint64_t* before = h.get();
        hip_ok(ensure(h, 1000, 4000), "pinned ensure of what fits");
        check(h.get() == before && h.cap() == 1000, "a pinned ensure of what fits reallocates nothing");
        PinGrowBuf<uint64_t> g(std::move(h));
        check(g.get() == before && g.cap() == 1000 && h.get() == nullptr && h.cap() == 0, "pinned move-construction transfers, the source is empty");
        PinGrowBuf<uint64_t> k;
        k = std::move(g);
        PinGrowBuf<uint64_t>& kself = k;
        k = std::move(kself);
        check(k.get() == before && k.cap() == 1000 && g.get() == nullptr && g.cap() == 0, "pinned move-assignment transfers, a self-move is harmless");
        hip_ok(k.regrow(2000), "pinned regrow(2000)");
        check(k.get() != nullptr && k.cap() == 2000, "pinned regrow of a larger size updates the capacity");
        PinBuf<uint64_t> s;
        hip_ok(s.alloc(16), "PinBuf::alloc(16)");
        uint64_t* sp = s.get();
        PinBuf<uint64_t> t(std::move(s));
        check(t.get() == sp && s.get() == nullptr, "PinBuf: move-construction transfers");
    }
    {   // LedgerBuf: every byte charged to the ledger and credited again, the limit refuses before hipMalloc, grow keeps what fits
        DevLedger L;
        {
            LedgerBuf<uint64_t> a, b;
            check(a.get() == nullptr && a.bytes() == 0 && L.now == 0 && L.peak == 0, "a new ledger buffer is empty, the ledger at 0");
            hip_ok(a.alloc(L, 8000 + 64), "LedgerBuf::alloc(8064)");
            check(a.get() != nullptr && a.bytes() == 8064 && L.now == 8064 && L.peak == 8064, "alloc charges its bytes, pad included");
            hip_ok(hipMemcpy(a.get(), pat.data(), 8000, hipMemcpyHostToDevice), "upload");
            uint64_t* before = a.get();
            hip_ok(a.grow(L, 8064), "grow of what fits");
            hip_ok(a.grow(L, 100), "grow of less");
            check(a.get() == before && a.bytes() == 8064 && L.now == 8064 && holds(a.get(), pat), "grow of what fits keeps pointer, size, contents and ledger");
            hip_ok(b.alloc(L, 1000), "second alloc");
            check(L.now == 9064 && L.peak == 9064, "two buffers: the ledger holds their sum");
            hip_ok(a.grow(L, 16000), "grow(16000)");
            check(a.bytes() == 16000 && L.now == 17000 && L.peak == 17000, "grow frees first, then allocates: no moment with both sizes in the ledger");
            b.reset();
            check(b.get() == nullptr && b.bytes() == 0 && L.now == 16000 && L.peak == 17000, "reset credits; the peak stays");
            b.reset();
            check(L.now == 16000, "a second reset credits nothing");
            // the limit: refused before any hipMalloc (a request the runtime could serve), nothing charged, what was held released first
            L.limit = 20000;
            hip_ok(b.alloc(L, 4000), "alloc up to the limit exactly");
            check(L.now == 20000, "an allocation that reaches the limit exactly is allowed");
            const hipError_t e = b.alloc(L, 4001);
            check(e == hipErrorOutOfMemory && b.get() == nullptr && b.bytes() == 0 && L.now == 16000, "one byte past the limit: out of memory, the buffer empty, its old bytes credited");
            check(hipGetLastError() == hipSuccess, "a refusal by the limit is not a HIP error");
            const hipError_t e2 = a.grow(L, 16001 + 4000);
            check(e2 == hipErrorOutOfMemory && a.get() == nullptr && L.now == 0, "grow past the limit: the contents are dropped first, as for any growth");
            L.limit = 0;
            const hipError_t e3 = a.alloc(L, (size_t)1 << 60);
            check(e3 == hipErrorOutOfMemory && a.get() == nullptr && L.now == 0, "hipMalloc of 2^60 bytes: out of memory, nothing charged");
            check(hipGetLastError() == hipSuccess, "after a failed hipMalloc no error is pending");
            // adoption and moves
            uint64_t* raw = nullptr;
            hip_ok(hipMalloc((void**)&raw, 512), "hipMalloc(512)");
            a.adopt(L, raw, 512);
            check(a.get() == raw && a.bytes() == 512 && L.now == 512, "adopt charges the size it is given");
            LedgerBuf<uint64_t> c(std::move(a));
            check(c.get() == raw && c.bytes() == 512 && a.get() == nullptr && a.bytes() == 0 && L.now == 512, "move-construction transfers, the ledger unchanged");
            hip_ok(b.alloc(L, 256), "alloc(256)");
            b = std::move(c);
            check(b.get() == raw && c.get() == nullptr && L.now == 512, "move-assignment releases what the target held and transfers");
            LedgerBuf<uint64_t>& bself = b;
            b = std::move(bself);
            check(b.get() == raw && b.bytes() == 512 && L.now == 512, "self-move-assignment is harmless");
            struct Two { LedgerBuf<uint64_t> x, y; } two;
            hip_ok(two.x.alloc(L, 128), "alloc(128)"); hip_ok(two.y.alloc(L, 64), "alloc(64)");
            check(L.now == 704, "a struct of owners: charged");
            two = Two();
            check(two.x.get() == nullptr && L.now == 512, "s = S() releases a struct of owners");
        }
        check(L.now == 0 && L.peak == 20000, "the destructors credit the rest; the peak is the largest sum ever held");
    }
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    printf("devbuf_check: %d checks passed\n", g_checks);
    return 0;
}
