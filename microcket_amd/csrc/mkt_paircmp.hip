// mkt_paircmp.hip -- pair-level concordance of two .pairs texts (the reference's benchmarking/check.consistency.pl) on the GPU.
// include/mkt.h has the definition, DESIGN.md 6e the join and why neighbours suffice.
//
// Both texts lie behind one another in one buffer (A, then B), so that one newline index numbers the lines "A in file order, then B in
// file order".  Per line a 16-byte SortRec: a hash of the id bytes in its 96 key bits (bit 63 of hi says "comment line", which sends
// those behind every data line), the line in idx.  The stable radix passes keep the line order inside a run of equal keys, so in a run
// that holds ONE id the last A record is the value and the first B record behind it the claimant: every record finds its class from
// its two neighbours.  A record whose predecessor has its key but not its id bytes marks a collision; the runs with such a mark are
// grouped by string on the host (pc_resolve, mkt_paircmp.h) and their classes written back.  Counters come from the class bytes.
// Integers only; the atomics are integer sums and an integer minimum, whose results do not depend on the order.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_blockscan.h"
#include "mkt_launch.h"
#include "mkt_paircmp.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

constexpr uint64_t kPcCommentBit = 1ull << 63;
constexpr uint64_t kPcNoBadLine = ~0ull;
constexpr int kPcCopyLanes = 16;                                   // lanes that copy one line (gather and emit)

// eight bytes from any offset: two aligned loads (the text buffers are 16-byte aligned and readable 64 bytes past their end)
__device__ inline uint64_t pc_load8(const uint8_t* text, uint64_t off) {
    const uint64_t* p = reinterpret_cast<const uint64_t*>(text + (off & ~7ull));
    const uint32_t sh = (uint32_t)(off & 7u) * 8u;
    const uint64_t lo = p[0];
    return sh ? (lo >> sh) | (p[1] << (64u - sh)) : lo;
}
// text[a, a + la) == text[b, b + lb), eight bytes a step
__device__ inline bool pc_bytes_eq(const uint8_t* text, uint64_t a, uint32_t la, uint64_t b, uint32_t lb) {
    if (la != lb) return false;
    uint32_t k = 0;
    for (; k + 8 <= la; k += 8) if (pc_load8(text, a + k) != pc_load8(text, b + k)) return false;
    if (k < la) {
        const uint64_t m = (1ull << ((la - k) * 8u)) - 1ull;
        if ((pc_load8(text, a + k) ^ pc_load8(text, b + k)) & m) return false;
    }
    return true;
}
__device__ inline uint64_t pc_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
    return x;
}
__device__ inline uint32_t pc_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

// ---- parse: field offsets, positions, distribution class, key --------------------------------------------------------------
// ctr: dist[2][4] (cis<1K, cis 1-10K, cis>10K, trans), then the data lines of the two sides.  bad: the smallest refused line.
__global__ __launch_bounds__(SWG) void k_pc_parse(const uint8_t* text, const uint64_t* starts, uint64_t nlines, uint64_t nA, uint32_t hash_bits, PcLine* lines,
                                                  SortRec* rec, unsigned long long* ctr, unsigned long long* bad) {
    __shared__ uint32_t sc[10];
    if (threadIdx.x < 10) sc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (j < nlines) {
        const uint64_t ls = starts[j], le = starts[j + 1] - 1;     // le: the newline
        PcLine L = {0, 0, 0, 0, 0, 0, 0, 0};
        SortRec r;
        r.hi = kPcCommentBit; r.lo = 0; r.idx = (uint32_t)j;
        if (!(le > ls && text[ls] == '#')) {
            const uint32_t side = j >= nA ? 1u : 0u;
            bool ok = le - ls < 0x80000000ull;
            uint32_t tabs[5];
            int nt = 0;
            uint64_t h1 = 0xcbf29ce484222325ull;
            uint32_t h2 = 0x811c9dc5u;
            if (ok) for (uint64_t p = ls; p < le; ++p) {
                const uint8_t c = text[p];
                if (c == '\t') { tabs[nt++] = (uint32_t)(p - ls); if (nt == 5) break; }
                else if (nt == 0) { h1 = (h1 ^ c) * 0x100000001b3ull; h2 = (h2 ^ c) * 16777619u; }
            }
            if (nt < 4) ok = false;
            if (ok) {
                L.t0 = tabs[0]; L.t1 = tabs[1]; L.t2 = tabs[2]; L.t3 = tabs[3];
                L.e5 = nt == 5 ? tabs[4] : (uint32_t)(le - ls);
                auto num = [&](uint32_t a, uint32_t b, uint32_t& out) {            // decimal, at least one digit, below 2^31
                    if (a >= b) return false;
                    uint64_t v = 0;
                    for (uint32_t q = a; q < b; ++q) {
                        const uint32_t d = (uint32_t)text[ls + q] - (uint32_t)'0';
                        if (d > 9u) return false;
                        v = v * 10 + d;
                        if (v > 0x7FFFFFFFull) return false;
                    }
                    out = (uint32_t)v;
                    return true;
                };
                ok = num(L.t1 + 1, L.t2, L.p1) && num(L.t3 + 1, L.e5, L.p2);
            }
            if (!ok) atomicMin(bad, (unsigned long long)j);
            else {
                L.data = 1;
                uint32_t cls = 3;
                if (pc_bytes_eq(text, ls + L.t0 + 1, L.t1 - L.t0 - 1, ls + L.t2 + 1, L.t3 - L.t2 - 1)) {
                    const uint32_t d = pc_absdiff(L.p1, L.p2);
                    cls = d > 10000u ? 2u : d < 1000u ? 0u : 1u;
                }
                atomicAdd(&sc[side * 4 + cls], 1u);
                atomicAdd(&sc[8 + side], 1u);
                const uint64_t g1 = pc_mix64(h1 ^ ((uint64_t)L.t0 << 40));
                const uint32_t g2 = pc_mix32(h2);
                if (hash_bits == 0) { r.hi = g1 >> 1; r.lo = g2; }
                else { r.hi = 0; r.lo = hash_bits >= 32 ? g2 : g2 & ((1u << hash_bits) - 1u); }
            }
        }
        lines[j] = L;
        rec[j] = r;
    }
    __syncthreads();
    if (threadIdx.x < 10 && sc[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

// ---- join: every sorted record from its two neighbours ----------------------------------------------------------------------
struct PcView {
    const uint8_t* text; const uint64_t* starts; const PcLine* lines;
};
__device__ inline bool pc_key_eq(const SortRec& x, const SortRec& y) { return x.hi == y.hi && x.lo == y.lo; }
__device__ inline bool pc_id_eq(const PcView& v, uint32_t a, uint32_t b) {
    return pc_bytes_eq(v.text, v.starts[a], v.lines[a].t0, v.starts[b], v.lines[b].t0);
}
__device__ inline bool pc_consistent_dev(const PcView& v, uint32_t ia, uint32_t ib, uint32_t D) {
    const PcLine a = v.lines[ia], b = v.lines[ib];
    const uint64_t sa = v.starts[ia], sb = v.starts[ib];
    const uint64_t a1 = sa + a.t0 + 1, a2 = sa + a.t2 + 1, b1 = sb + b.t0 + 1, b2 = sb + b.t2 + 1;
    const uint32_t la1 = a.t1 - a.t0 - 1, la2 = a.t3 - a.t2 - 1, lb1 = b.t1 - b.t0 - 1, lb2 = b.t3 - b.t2 - 1;
    if (pc_absdiff(a.p1, b.p1) < D && pc_absdiff(a.p2, b.p2) < D && pc_bytes_eq(v.text, a1, la1, b1, lb1) && pc_bytes_eq(v.text, a2, la2, b2, lb2)) return true;
    return pc_absdiff(a.p1, b.p2) < D && pc_absdiff(a.p2, b.p1) < D && pc_bytes_eq(v.text, a1, la1, b2, lb2) && pc_bytes_eq(v.text, a2, la2, b1, lb1);
}
// rec[0, ndata): the data lines in key order.  cls and partner per LINE, cflag per sorted RECORD (1: its predecessor has its key but
// another id), ncoll: how many of those (only "none" or "some" is used).
__global__ __launch_bounds__(SWG) void k_pc_join(PcView v, const SortRec* rec, uint64_t ndata, uint32_t nA, uint32_t D, uint8_t* cls, uint32_t* partner, uint8_t* cflag,
                                                 unsigned int* ncoll) {
    const uint64_t j = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (j >= ndata) return;
    const SortRec r = rec[j];
    const bool isB = r.idx >= nA;
    bool prev_same = false, next_same = false, coll = false;
    uint32_t pi = 0, ni = 0;
    if (j > 0) {
        const SortRec q = rec[j - 1];
        if (pc_key_eq(q, r)) { pi = q.idx; prev_same = pc_id_eq(v, pi, r.idx); coll = !prev_same; }
    }
    if (j + 1 < ndata) {
        const SortRec q = rec[j + 1];
        if (pc_key_eq(q, r)) { ni = q.idx; next_same = pc_id_eq(v, ni, r.idx); }
    }
    uint8_t c = PC_ONLY;
    uint32_t pa = kPcNoPartner;
    if (!isB) {
        if (next_same && ni < nA) c = PC_SUPERSEDED;                               // a later A line has this id
        else if (next_same) c = pc_consistent_dev(v, r.idx, ni, D) ? PC_CONSISTENT : PC_DISCORDANT;      // the id's first B line claims it
    } else if (prev_same && pi < nA) {                                             // the id's first B line, right behind its value
        c = pc_consistent_dev(v, pi, r.idx, D) ? PC_CONSISTENT : PC_DISCORDANT;
        pa = pi;
    }
    cls[r.idx] = c;
    partner[r.idx] = pa;
    cflag[j] = coll ? 1 : 0;
    if (coll) atomicAdd(ncoll, 1u);
}

// ctr[0..4]: classes 0..4 of side A, ctr[5..9]: of side B
__global__ __launch_bounds__(SWG) void k_pc_count(const uint8_t* cls, uint64_t nlines, uint64_t nA, unsigned long long* ctr) {
    __shared__ uint32_t sc[10];
    if (threadIdx.x < 10) sc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t j = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (j < nlines) { const uint32_t c = cls[j]; if (c < 5u) atomicAdd(&sc[(j >= nA ? 5u : 0u) + c], 1u); }
    __syncthreads();
    if (threadIdx.x < 10 && sc[threadIdx.x]) atomicAdd(&ctr[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

// ---- the lines of flagged runs for the host, and its answer ---------------------------------------------------------------------
__global__ void k_pc_gather_meta(const uint32_t* list, uint64_t m, const PcLine* lines, PcLine* meta, uint64_t* len) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const PcLine L = lines[list[k]];
    meta[k] = L;
    len[k] = L.e5;
}
__global__ __launch_bounds__(SWG) void k_pc_gather_bytes(const uint32_t* list, uint64_t m, const uint8_t* text, const uint64_t* starts, const PcLine* meta, const uint64_t* offs,
                                                         uint8_t* out) {
    const uint64_t k = ((uint64_t)blockIdx.x * SWG + threadIdx.x) / kPcCopyLanes;
    const uint32_t sub = threadIdx.x % kPcCopyLanes;
    if (k >= m) return;
    const uint64_t s = starts[list[k]], o = offs[k];
    const uint32_t n = meta[k].e5;
    for (uint32_t q = sub; q < n; q += kPcCopyLanes) out[o + q] = text[s + q];
}
__global__ void k_pc_scatter(const uint32_t* list, uint64_t m, const uint8_t* c, const uint32_t* pa, uint8_t* cls, uint32_t* partner) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    cls[list[k]] = c[k];
    partner[list[k]] = pa[k];
}

// ---- the text: B's discordant and B-only lines in file order, then the A-only lines in file order --------------------------------
// output slot k: line nA + k for k < nB, line k - nB behind them
__device__ inline uint64_t pc_slot_line(uint64_t k, uint64_t nA, uint64_t nB) { return k < nB ? nA + k : k - nB; }
__global__ void k_pc_lens(const uint8_t* cls, const uint32_t* partner, const PcLine* lines, uint64_t nA, uint64_t nB, uint64_t* len) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nA + nB) return;
    const uint64_t i = pc_slot_line(k, nA, nB);
    const uint32_t c = cls[i];
    uint64_t n = 0;
    if (c == PC_ONLY) n = 2ull + lines[i].e5 + 1ull;                               // "B\t" or "A\t", id .. p2, newline
    else if (c == PC_DISCORDANT && k < nB && partner[i] < nA) {
        const PcLine b = lines[i], a = lines[partner[i]];
        n = 2ull + (b.t0 + 1ull) + (a.e5 - a.t0 - 1ull) + 4ull + (b.e5 - b.t0 - 1ull) + 1ull;      // "I\t" id "\t" A's four "\tvs\t" B's four "\n"
    }
    len[k] = n;
}
__device__ inline void pc_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t sub) {
    for (uint32_t q = sub; q < n; q += kPcCopyLanes) dst[q] = src[q];
}
__global__ __launch_bounds__(SWG) void k_pc_emit(const uint8_t* cls, const uint32_t* partner, const PcLine* lines, const uint8_t* text, const uint64_t* starts, uint64_t nA,
                                                 uint64_t nB, const uint64_t* offs, uint8_t* out) {
    const uint64_t k = ((uint64_t)blockIdx.x * SWG + threadIdx.x) / kPcCopyLanes;
    const uint32_t sub = threadIdx.x % kPcCopyLanes;
    if (k >= nA + nB) return;
    const uint64_t i = pc_slot_line(k, nA, nB);
    const uint32_t c = cls[i];
    uint8_t* d = out + offs[k];
    if (c == PC_ONLY) {
        const PcLine L = lines[i];
        if (sub == 0) { d[0] = k < nB ? 'B' : 'A'; d[1] = '\t'; d[2 + L.e5] = '\n'; }
        pc_copy(d + 2, text + starts[i], L.e5, sub);
    } else if (c == PC_DISCORDANT && k < nB && partner[i] < nA) {
        const uint32_t ia = partner[i];
        const PcLine b = lines[i], a = lines[ia];
        const uint32_t na = a.e5 - a.t0 - 1, nb = b.e5 - b.t0 - 1;
        uint8_t* da = d + 2 + b.t0 + 1;
        uint8_t* dv = da + na;
        if (sub == 0) { d[0] = 'I'; d[1] = '\t'; dv[0] = '\t'; dv[1] = 'v'; dv[2] = 's'; dv[3] = '\t'; dv[4 + nb] = '\n'; }
        pc_copy(d + 2, text + starts[i], b.t0 + 1, sub);                            // the id and its tab
        pc_copy(da, text + starts[ia] + a.t0 + 1, na, sub);
        pc_copy(dv + 4, text + starts[i] + b.t0 + 1, nb, sub);
    }
}

}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------------
struct mkt_paircmp {
    int device = 0;
    DevStream stream;                                   // declared first: destroyed after every buffer
    GrowBuf<uint8_t> side[2]; size_t len[2] = {0, 0};   // the two texts as they were added
    DevBuf<uint8_t> cat; uint64_t cat_len = 0, cat_a = 0;      // A, then B, each ending with a newline; cat_a: bytes of A in it
    bool cat_valid = false;
    DevBuf<uint8_t> cls; uint64_t nlines = 0, nA = 0;   // class bytes of the last run, per line of cat
    DevBuf<uint8_t> out; uint64_t out_len = 0;
    bool ran = false;
    double ms[4] = {0, 0, 0, 0};
    std::string err;
};
static int pfail(mkt_paircmp* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf;
    return code;
}
#define PCHK(p, call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return pfail((p), MKT_E_NOMEM, "%s: the device memory does not suffice (both texts, their line index and 16-byte records are resident)", #call); } \
                           if (e_ != hipSuccess) return pfail((p), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

static int paircmp_reserve(mkt_paircmp* p, int s, size_t need) {
    GrowBuf<uint8_t>& b = p->side[s];
    if (b.fits(need + 64)) return MKT_OK;
    size_t ncap = b.cap() ? b.cap() - 64 : ((size_t)1 << 20);
    while (ncap < need) ncap *= 2;
    PCHK(p, b.regrow_keep(ncap + 64, p->len[s]));
    return MKT_OK;
}
static int paircmp_add(mkt_paircmp* p, int s, const void* bytes, size_t n, hipMemcpyKind kind) {
    if (!p || (n && !bytes) || s < 0 || s > 1) return MKT_E_ARG;
    PCHK(p, hipSetDevice(p->device));
    if (int rc = paircmp_reserve(p, s, p->len[s] + n + 1)) return rc;
    if (n) PCHK(p, hipMemcpyAsync(p->side[s] + p->len[s], bytes, n, kind, p->stream));
    PCHK(p, hipStreamSynchronize(p->stream));           // the caller may reuse `bytes`
    p->len[s] += n;
    p->cat_valid = false; p->ran = false;
    return MKT_OK;
}
// A, then B, whole lines only: a missing final newline is added
static int paircmp_cat(mkt_paircmp* p) {
    if (p->cat_valid) return MKT_OK;
    uint64_t n[2];
    bool nl[2];
    for (int s = 0; s < 2; ++s) {
        char last = '\n';
        if (p->len[s]) PCHK(p, hipMemcpy(&last, p->side[s] + p->len[s] - 1, 1, hipMemcpyDeviceToHost));
        nl[s] = last != '\n';
        n[s] = p->len[s] + (nl[s] ? 1 : 0);
    }
    p->cat.reset();
    PCHK(p, p->cat.alloc(n[0] + n[1], 64));
    uint64_t at = 0;
    for (int s = 0; s < 2; ++s) {
        if (p->len[s]) PCHK(p, hipMemcpyAsync(p->cat + at, p->side[s].get(), p->len[s], hipMemcpyDeviceToDevice, p->stream));
        if (nl[s]) PCHK(p, hipMemsetAsync(p->cat + at + p->len[s], '\n', 1, p->stream));
        at += n[s];
    }
    PCHK(p, hipMemsetAsync(p->cat + at, 0, 64, p->stream));
    PCHK(p, hipStreamSynchronize(p->stream));
    p->cat_len = at; p->cat_a = n[0];
    p->cat_valid = true;
    return MKT_OK;
}

extern "C" {

int mkt_paircmp_create(int device, mkt_paircmp** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_paircmp* p = new mkt_paircmp();
    p->device = device;
    if (hipSetDevice(device) != hipSuccess || p->stream.create(hipStreamNonBlocking) != hipSuccess) { mkt_paircmp_destroy(p); return MKT_E_HIP; }
    *out = p;
    return MKT_OK;
}
void mkt_paircmp_destroy(mkt_paircmp* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;                                           // the buffers, then the stream
}
const char* mkt_paircmp_error(const mkt_paircmp* p) { return p ? p->err.c_str() : ""; }

int mkt_paircmp_add(mkt_paircmp* p, int side, const char* bytes, size_t n) { return paircmp_add(p, side, bytes, n, hipMemcpyHostToDevice); }
int mkt_paircmp_add_device(mkt_paircmp* p, int side, const void* d_bytes, size_t n) { return paircmp_add(p, side, d_bytes, n, hipMemcpyDeviceToDevice); }

void mkt_paircmp_opts_default(mkt_paircmp_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_dist = kPcDefaultDist; o->want_lines = 1; o->hash_bits = 0;
}

int mkt_paircmp_run(mkt_paircmp* p, const mkt_paircmp_opts* opts, mkt_paircmp_info* info) {
    if (!p) return MKT_E_ARG;
    mkt_paircmp_opts o;
    mkt_paircmp_opts_default(&o);
    if (opts) o = *opts;
    if (o.hash_bits > 32) return pfail(p, MKT_E_ARG, "hash_bits %u: 0 (the full width) or 1 .. 32", o.hash_bits);
    for (uint32_t r : o.reserved) if (r) return pfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    const uint32_t D = pc_dist(o.max_dist);
    mkt_paircmp_info I;
    memset(&I, 0, sizeof I);
    if (info) *info = I;
    PCHK(p, hipSetDevice(p->device));
    p->ran = false; p->out_len = 0; p->nlines = 0; p->nA = 0;
    p->out.reset(); p->cls.reset();
    for (double& m : p->ms) m = 0;
    if (int rc = paircmp_cat(p)) return rc;
    const uint64_t n = p->cat_len;
    if (n == 0) { p->ran = true; return MKT_OK; }
    const uint8_t* text = p->cat;
    hipStream_t st = p->stream;
    DevEvents<5> ev;
    PCHK(p, ev.create());
    PCHK(p, hipEventRecord(ev[0], st));
    // line index over both texts; the lines of A are those that start inside it
    uint64_t nA = 0;
    if (p->cat_a) { LineIndex ia; PCHK(p, ia.count(text, p->cat_a, st)); nA = ia.nlines; }
    LineIndex ix;
    PCHK(p, ix.count(text, n, st));
    const uint64_t nl = ix.nlines, nB = nl - nA;
    if (nl >= (1ull << 32)) return pfail(p, MKT_E_CAPACITY, "%llu lines in the two texts together: lines are indexed with 32 bits", (unsigned long long)nl);
    PCHK(p, ix.fill(text, n, st));
    const uint64_t* starts = ix.starts;
    DevBuf<PcLine> lines;
    DevBuf<SortRec> bufA, bufB;
    DevBuf<uint32_t> d_hist, partner;
    DevBuf<unsigned long long> d_ctr;                    // [0..9] parse counters, [10] smallest refused line, [11] collisions (low word), [12..21] class counts
    DevBuf<uint8_t> cflag;
    PCHK(p, lines.alloc(nl));
    PCHK(p, bufA.alloc(nl + 1));
    PCHK(p, bufB.alloc(nl + 1));
    PCHK(p, d_hist.alloc(kSortHistBytes / 4));
    PCHK(p, partner.alloc(nl));
    PCHK(p, d_ctr.alloc(32));
    PCHK(p, p->cls.alloc(nl));
    PCHK(p, hipMemsetAsync(d_ctr, 0, 32 * sizeof(unsigned long long), st));
    PCHK(p, hipMemsetAsync(d_ctr + 10, 0xFF, sizeof(unsigned long long), st));
    PCHK(p, hipMemsetAsync(p->cls, 0, nl, st));
    const unsigned lgrid = (unsigned)((nl + SWG - 1) / SWG);
    SortRec *rA = bufA, *rB = bufB;
    hipLaunchKernelGGL(k_pc_parse, dim3(lgrid), dim3(SWG), 0, st, text, starts, nl, nA, o.hash_bits, lines.get(), rA, d_ctr.get(), d_ctr + 10);
    PCHK(p, hipGetLastError());
    unsigned long long hc[11];
    PCHK(p, hipMemcpyAsync(hc, d_ctr, sizeof hc, hipMemcpyDeviceToHost, st));
    PCHK(p, hipEventRecord(ev[1], st));
    PCHK(p, hipStreamSynchronize(st));
    if (hc[10] != kPcNoBadLine) {
        const bool inB = hc[10] >= nA;
        return pfail(p, MKT_E_ARG, "file %s line %llu: fewer than five fields or a position that is not a decimal integer below 2^31", inB ? "B" : "A",
                     (unsigned long long)(hc[10] - (inB ? nA : 0) + 1));
    }
    I.lines[0] = nA; I.lines[1] = nB;
    I.data_lines[0] = hc[8]; I.data_lines[1] = hc[9];
    for (int s = 0; s < 2; ++s) for (int k = 0; k < 4; ++k) I.dist[s][k] = hc[s * 4 + k];
    const uint64_t ndata = hc[8] + hc[9];
    // stable radix passes over the bits the key uses; the comment bit goes last, so the data lines come first
    if (o.hash_bits) {
        sort_radix_passes(rA, rB, nl, d_hist, 0, 0, (int)((o.hash_bits + 3) / 4 * 4), st);
        sort_radix_passes(rA, rB, nl, d_hist, 1, 60, 4, st);
    } else {
        sort_radix_passes(rA, rB, nl, d_hist, 0, 0, 32, st);
        sort_radix_passes(rA, rB, nl, d_hist, 1, 0, 64, st);
    }
    PCHK(p, hipGetLastError());
    PCHK(p, hipEventRecord(ev[2], st));
    // join
    if (ndata) {
        PCHK(p, cflag.alloc(ndata));
        const PcView v = {text, starts, lines.get()};
        hipLaunchKernelGGL(k_pc_join, dim3((unsigned)((ndata + SWG - 1) / SWG)), dim3(SWG), 0, st, v, (const SortRec*)rA, ndata, (uint32_t)nA, D, p->cls.get(), partner.get(),
                           cflag.get(), (unsigned int*)(d_ctr + 11));
        PCHK(p, hipGetLastError());
        unsigned long long ncoll = 0;
        PCHK(p, hipMemcpyAsync(&ncoll, d_ctr + 11, sizeof ncoll, hipMemcpyDeviceToHost, st));
        PCHK(p, hipStreamSynchronize(st));
        if (ncoll) {                                     // runs that hold more than one id: grouped by string on the host
            std::vector<SortRec> hrec(ndata);
            std::vector<uint8_t> hflag(ndata);
            PCHK(p, hipMemcpy(hrec.data(), rA, ndata * sizeof(SortRec), hipMemcpyDeviceToHost));
            PCHK(p, hipMemcpy(hflag.data(), cflag, ndata, hipMemcpyDeviceToHost));
            std::vector<uint32_t> list;                  // the lines of the flagged runs, run by run in sorted order
            std::vector<uint64_t> run_end;               // ... and where each run ends in the list
            for (uint64_t b = 0; b < ndata;) {
                uint64_t e = b + 1;
                bool flagged = false;
                while (e < ndata && hrec[e].hi == hrec[b].hi && hrec[e].lo == hrec[b].lo) { flagged |= hflag[e] != 0; ++e; }
                if (flagged) { for (uint64_t k = b; k < e; ++k) list.push_back(hrec[k].idx); run_end.push_back(list.size()); }
                b = e;
            }
            hrec = std::vector<SortRec>(); hflag = std::vector<uint8_t>();
            const uint64_t m = list.size();
            DevBuf<uint32_t> d_list, d_pa;
            DevBuf<PcLine> d_meta;
            DevBuf<uint64_t> d_len;
            DevBuf<uint8_t> d_bytes, d_c;
            PCHK(p, d_list.alloc(m));
            PCHK(p, d_meta.alloc(m));
            PCHK(p, d_len.alloc(m + 1));
            PCHK(p, hipMemcpyAsync(d_list, list.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            const unsigned mgrid = (unsigned)((m + 255) / 256);
            hipLaunchKernelGGL(k_pc_gather_meta, dim3(mgrid), dim3(256), 0, st, (const uint32_t*)d_list.get(), m, (const PcLine*)lines.get(), d_meta.get(), d_len.get());
            PCHK(p, launch_exscan(d_len, m, d_len + m, st));
            std::vector<uint64_t> hoff(m + 1);
            PCHK(p, hipMemcpyAsync(hoff.data(), d_len, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
            PCHK(p, hipStreamSynchronize(st));
            const uint64_t nbytes = hoff[m];
            PCHK(p, d_bytes.alloc(nbytes + 1));
            hipLaunchKernelGGL(k_pc_gather_bytes, dim3((unsigned)((m * kPcCopyLanes + SWG - 1) / SWG)), dim3(SWG), 0, st, (const uint32_t*)d_list.get(), m, text, starts,
                               (const PcLine*)d_meta.get(), (const uint64_t*)d_len.get(), d_bytes.get());
            PCHK(p, hipGetLastError());
            std::vector<PcLine> hmeta(m);
            std::vector<char> hbytes(nbytes + 1);
            PCHK(p, hipMemcpyAsync(hmeta.data(), d_meta, m * sizeof(PcLine), hipMemcpyDeviceToHost, st));
            PCHK(p, hipMemcpyAsync(hbytes.data(), d_bytes, nbytes, hipMemcpyDeviceToHost, st));
            PCHK(p, hipStreamSynchronize(st));
            std::vector<uint8_t> hc2(m);
            std::vector<uint32_t> hpa(m);
            std::vector<PcItem> items;
            std::vector<uint8_t> c1;
            std::vector<uint32_t> p1;
            uint64_t b = 0;
            for (uint64_t e : run_end) {
                items.clear();
                for (uint64_t k = b; k < e; ++k) items.push_back(PcItem{list[k], list[k] >= nA ? 1u : 0u, hbytes.data() + hoff[k], hmeta[k]});
                pc_resolve(items, D, c1, p1);
                for (uint64_t k = b; k < e; ++k) { hc2[k] = c1[k - b]; hpa[k] = p1[k - b]; }
                b = e;
            }
            I.host_runs = run_end.size();
            PCHK(p, d_c.alloc(m));
            PCHK(p, d_pa.alloc(m));
            PCHK(p, hipMemcpyAsync(d_c, hc2.data(), m, hipMemcpyHostToDevice, st));
            PCHK(p, hipMemcpyAsync(d_pa, hpa.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_pc_scatter, dim3(mgrid), dim3(256), 0, st, (const uint32_t*)d_list.get(), m, (const uint8_t*)d_c.get(), (const uint32_t*)d_pa.get(), p->cls.get(),
                               partner.get());
            PCHK(p, hipGetLastError());
            PCHK(p, hipStreamSynchronize(st));           // the host vectors and the device buffers of this block end here
        }
    }
    hipLaunchKernelGGL(k_pc_count, dim3(lgrid), dim3(SWG), 0, st, (const uint8_t*)p->cls.get(), nl, nA, d_ctr + 12);
    PCHK(p, hipGetLastError());
    unsigned long long cc[10];
    PCHK(p, hipMemcpyAsync(cc, d_ctr + 12, sizeof cc, hipMemcpyDeviceToHost, st));
    PCHK(p, hipEventRecord(ev[3], st));
    PCHK(p, hipStreamSynchronize(st));
    I.a_only = cc[PC_ONLY]; I.distinct_a = cc[PC_ONLY] + cc[PC_CONSISTENT] + cc[PC_DISCORDANT];
    I.b_only = cc[5 + PC_ONLY]; I.consistent = cc[5 + PC_CONSISTENT]; I.discordant = cc[5 + PC_DISCORDANT];
    if (cc[PC_CONSISTENT] != I.consistent || cc[PC_DISCORDANT] != I.discordant)
        return pfail(p, MKT_E_KERNEL, "the two sides disagree on the claimed pairs (A: %llu + %llu, B: %llu + %llu)", cc[PC_CONSISTENT], cc[PC_DISCORDANT],
                     (unsigned long long)I.consistent, (unsigned long long)I.discordant);
    // the text
    if (o.want_lines) {
        DevBuf<uint64_t> d_len;
        PCHK(p, d_len.alloc(nl + 1));
        hipLaunchKernelGGL(k_pc_lens, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, (const uint8_t*)p->cls.get(), (const uint32_t*)partner.get(), (const PcLine*)lines.get(), nA,
                           nB, d_len.get());
        PCHK(p, launch_exscan(d_len, nl, d_len + nl, st));
        uint64_t total = 0;
        PCHK(p, hipMemcpyAsync(&total, d_len + nl, sizeof total, hipMemcpyDeviceToHost, st));
        PCHK(p, hipStreamSynchronize(st));
        PCHK(p, p->out.alloc(total + 1));
        hipLaunchKernelGGL(k_pc_emit, dim3((unsigned)((nl * kPcCopyLanes + SWG - 1) / SWG)), dim3(SWG), 0, st, (const uint8_t*)p->cls.get(), (const uint32_t*)partner.get(),
                           (const PcLine*)lines.get(), text, starts, nA, nB, (const uint64_t*)d_len.get(), p->out.get());
        PCHK(p, hipGetLastError());
        PCHK(p, hipEventRecord(ev[4], st));
        PCHK(p, hipStreamSynchronize(st));
        p->out_len = total;
        I.lines_bytes = total;
    } else {
        PCHK(p, hipEventRecord(ev[4], st));
        PCHK(p, hipStreamSynchronize(st));
    }
    for (int k = 0; k < 4; ++k) { float f = 0; PCHK(p, hipEventElapsedTime(&f, ev[k], ev[k + 1])); p->ms[k] = f; }
    p->nlines = nl; p->nA = nA;
    p->ran = true;
    if (info) *info = I;
    return MKT_OK;
}

int mkt_paircmp_fetch_classes(mkt_paircmp* p, int side, uint64_t first, uint64_t n, uint8_t* out) {
    if (!p || (n && !out) || side < 0 || side > 1) return MKT_E_ARG;
    if (!p->ran) return pfail(p, MKT_E_STATE, "fetch before run");
    const uint64_t have = side ? p->nlines - p->nA : p->nA;
    if (first > have || n > have - first) return pfail(p, MKT_E_ARG, "lines [%llu, %llu) of a side of %llu", (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)have);
    PCHK(p, hipSetDevice(p->device));
    if (n) PCHK(p, hipMemcpy(out, p->cls + (side ? p->nA : 0) + first, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_paircmp_fetch_lines(mkt_paircmp* p, uint64_t off, char* out, size_t n) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->ran) return pfail(p, MKT_E_STATE, "fetch before run");
    if (off > p->out_len || n > p->out_len - off) return pfail(p, MKT_E_ARG, "range past the end of the text");
    PCHK(p, hipSetDevice(p->device));
    if (n) PCHK(p, hipMemcpy(out, p->out + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
long mkt_paircmp_report(const mkt_paircmp_info* info, uint32_t max_dist, const char* name_a, const char* name_b, char* out, size_t cap) {
    if (!info || !out) return -1;
    const std::string s = pc_report(*info, max_dist, name_a ? name_a : "", name_b ? name_b : "");
    if (s.size() + 1 > cap) return -1;
    memcpy(out, s.c_str(), s.size() + 1);
    return (long)s.size();
}
int mkt_paircmp_timing(const mkt_paircmp* p, double* parse_ms, double* sort_ms, double* join_ms, double* emit_ms) {
    if (!p) return MKT_E_ARG;
    if (parse_ms) *parse_ms = p->ms[0];
    if (sort_ms) *sort_ms = p->ms[1];
    if (join_ms) *join_ms = p->ms[2];
    if (emit_ms) *emit_ms = p->ms[3];
    return MKT_OK;
}

}  // extern "C"
