// mkt_pairstat.hip -- pair statistics of a .pairs text on the GPU: distance by orientation, the counters behind P(s), chromosome pairs.
// include/mkt.h has the definition, DESIGN.md 6k the kernels; what a line adds to which counter is mkt_pairstat.h, shared with the host.
//
// One streaming pass.  A piece of text is indexed by the sorter's newline index; k_ps_text gives every lane kPsIters lines, which it
// parses and classifies with the shared device functions.  The scalar counters are aggregated per wave (a ballot and a popcount per
// counter, one LDS add), the 74 x 4 distance cells are LDS atomics, and the workgroup's LDS table leaves once, as 64-bit atomic adds of
// its non-zero cells.  The dense chromosome-pair table is global: inside the wave the lanes that share the leader's cell are balloted
// away round by round, one 64-bit add of the popcount per distinct cell -- one round for a wave of sorted final.pairs, 64 at the most.
// k_ps_keys does the same from a context's key records.  Integers only: the sums do not depend on the order.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_core.h"
#include "mkt_devbuf.h"
#include "mkt_pairstat.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

constexpr int PSWG = 256;
constexpr int kPsIters = 8;                                    // lines per lane: a workgroup flushes its table once per 2048 lines
constexpr uint32_t kPsLinesPerWg = PSWG * kPsIters;
constexpr uint64_t kPsNoBadLine = ~0ull;

// every lane of the wave calls this (live: the lane holds a line); sh: the workgroup's table, chrom: n x n
__device__ inline void ps_accumulate(const PsClass& c, bool live, uint32_t* sh, unsigned long long* chrom) {
    const int lane = threadIdx.x & 63;
    const uint32_t m = live ? ps_scalar_mask(c) : 0u;
#pragma unroll
    for (int s = 0; s < PS_SCALARS; ++s) {
        const uint64_t b = __ballot((m >> s) & 1u);
        if (lane == 0 && b) atomicAdd(&sh[kPsDistCells + s], (uint32_t)__popcll(b));
    }
    const int d = live ? ps_dist_cell(c) : -1;
    if (d >= 0) atomicAdd(&sh[d], 1u);
    const bool counted = live && (c.kind == PS_K_CIS || c.kind == PS_K_TRANS);
    uint64_t rest = __ballot(counted);                          // uniform in the wave, as is everything derived from ballots
    while (rest) {
        const int leader = __ffsll((unsigned long long)rest) - 1;
        const uint32_t lc = (uint32_t)__shfl((int)c.cell, leader, 64);
        const uint64_t same = __ballot(counted && c.cell == lc);
        if (lane == leader) atomicAdd(&chrom[lc], (unsigned long long)__popcll(same));
        rest &= ~same;                                          // the leader is in `same`: at most 64 rounds
    }
}
__device__ inline void ps_flush(const uint32_t* sh, unsigned long long* ctr) {
    __syncthreads();
    for (int k = threadIdx.x; k < kPsCells; k += PSWG) if (sh[k]) atomicAdd(&ctr[k], (unsigned long long)sh[k]);
}

// line j of this piece is line line0 + j of the whole text; bad: the smallest refused line
__global__ __launch_bounds__(PSWG) void k_ps_text(const uint8_t* text, const uint64_t* starts, uint64_t nlines, uint64_t line0, const MxTab* tab, uint32_t n,
                                                  unsigned long long* ctr, unsigned long long* chrom, unsigned long long* bad) {
    __shared__ uint32_t sh[kPsCells];
    for (int k = threadIdx.x; k < kPsCells; k += PSWG) sh[k] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kPsLinesPerWg;
    for (int it = 0; it < kPsIters; ++it) {
        const uint64_t j = base + (uint64_t)it * PSWG + threadIdx.x;
        const bool live = j < nlines;
        PsClass c;
        c.kind = PS_K_BAD; c.cell = 0; c.dist = 0; c.ori = kPsNoOri; c.ref = 0;
        if (live) {
            c = ps_parse_line(text, starts[j], starts[j + 1] - 1, tab, n);
            if (c.kind == PS_K_BAD) atomicMin(bad, (unsigned long long)(line0 + j));
        }
        ps_accumulate(c, live, sh, chrom);
    }
    ps_flush(sh, ctr);
}

// a context's key records (mkt_core.h KeyRec); lut: the context's chromosome slot -> table index (0xFFFF: not in the table)
__global__ __launch_bounds__(PSWG) void k_ps_keys(const KeyRec* keys, uint64_t nkeys, const uint16_t* lut, const uint8_t* flags, const MxTab* tab, uint32_t n,
                                                  unsigned long long* ctr, unsigned long long* chrom) {
    __shared__ uint32_t sh[kPsCells];
    for (int k = threadIdx.x; k < kPsCells; k += PSWG) sh[k] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kPsLinesPerWg;
    for (int it = 0; it < kPsIters; ++it) {
        const uint64_t j = base + (uint64_t)it * PSWG + threadIdx.x;
        const bool live = j < nkeys && !(flags && flags[j]);
        PsClass c;
        c.kind = PS_K_BAD; c.cell = 0; c.dist = 0; c.ori = kPsNoOri; c.ref = 0;
        if (live) {
            const KeyRec k = keys[j];
            const uint32_t a = lut[(k.k0 >> 45) & (kChrSlots - 1u)], b = lut[(k.k0 >> 32) & (kChrSlots - 1u)];
            const uint32_t ori = (uint32_t)((k.k1 >> 30) & 3ull);                  // sA('-') << 1 | sB('-')
            const uint32_t sa = (uint32_t)(k.k0 >> 45) & (kChrSlots - 1u), sb = (uint32_t)(k.k0 >> 32) & (kChrSlots - 1u);      // one slot per name
            c = ps_classify(a == 0xFFFFu ? MX_SKIP : a, k.k0 & 0xFFFFFFFFull, b == 0xFFFFu ? MX_SKIP : b, k.k1 >> 32, ori, sa == sb, tab, n);
        }
        ps_accumulate(c, live, sh, chrom);
    }
    ps_flush(sh, ctr);
}

}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------------
struct mkt_pairstat {
    int device = 0;
    DevStream stream;                                   // declared first: destroyed after every buffer
    DevEvents<4> ev;
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    std::unordered_map<std::string, uint32_t> index;
    DevBuf<MxTab> d_tab;
    DevBuf<unsigned long long> d_ctr;                   // kPsCells counters, then the smallest refused line
    DevBuf<unsigned long long> d_chrom;                 // n x n
    GrowBuf<uint8_t> text;                              // one piece: whole lines, 64 readable bytes behind them
    std::string carry;                                  // an incomplete last line of the text seen so far
    uint64_t lines_seen = 0;
    bool ran = false;
    std::vector<uint64_t> ctr, chrom;                   // of the last run
    PsResult res;
    double ms[3] = {0, 0, 0};
    std::string err;
};
static thread_local std::string g_ps_create_err;
static int sfail(mkt_pairstat* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf; else g_ps_create_err = buf;
    return code;
}
#define SCHK(p, call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return sfail((p), MKT_E_NOMEM, "%s: the device memory does not suffice (one piece of text and its line index are resident: add smaller pieces)", #call); } \
                           if (e_ != hipSuccess) return sfail((p), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

static int ps_reserve(mkt_pairstat* p, size_t need) {
    if (p->text.fits(need + 64)) return MKT_OK;
    size_t ncap = (size_t)1 << 20;
    while (ncap < need) ncap *= 2;
    SCHK(p, hipStreamSynchronize(p->stream));
    SCHK(p, p->text.regrow(ncap + 64));
    return MKT_OK;
}
// text[0, n) holds whole lines: index them and count
static int ps_process(mkt_pairstat* p, size_t n) {
    if (n == 0) return MKT_OK;
    hipStream_t st = p->stream;
    const uint8_t* text = p->text;
    SCHK(p, hipMemsetAsync(p->text + n, 0, 64, st));
    SCHK(p, hipEventRecord(p->ev[1], st));
    LineIndex ix;
    SCHK(p, ix.count(text, n, st));
    const uint64_t nl = ix.nlines;
    if (nl) SCHK(p, ix.fill(text, n, st));
    SCHK(p, hipEventRecord(p->ev[2], st));
    if (nl) {
        const uint64_t grid = (nl + kPsLinesPerWg - 1) / kPsLinesPerWg;
        if (grid > 0x7FFFFFFFull) return sfail(p, MKT_E_CAPACITY, "%llu lines in one piece: add smaller pieces", (unsigned long long)nl);
        hipLaunchKernelGGL(k_ps_text, dim3((unsigned)grid), dim3(PSWG), 0, st, text, (const uint64_t*)ix.starts.get(), nl, p->lines_seen, (const MxTab*)p->d_tab.get(),
                           (uint32_t)p->names.size(), p->d_ctr.get(), p->d_chrom.get(), p->d_ctr + kPsCells);
        SCHK(p, hipGetLastError());
    }
    SCHK(p, hipEventRecord(p->ev[3], st));
    SCHK(p, hipStreamSynchronize(st));                  // the index goes with this scope, the piece may be overwritten
    float a = 0, b = 0, c = 0;
    SCHK(p, hipEventElapsedTime(&a, p->ev[1], p->ev[2]));
    SCHK(p, hipEventElapsedTime(&b, p->ev[2], p->ev[3]));
    SCHK(p, hipEventElapsedTime(&c, p->ev[0], p->ev[3]));
    p->ms[0] += a; p->ms[1] += b; p->ms[2] += c;
    p->lines_seen += nl;
    p->ran = false;
    return MKT_OK;
}

extern "C" {

int mkt_pairstat_create(int device, const char* chromsizes, size_t len, mkt_pairstat** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sfail(nullptr, MKT_E_NO_DEVICE, "no usable HIP device (there is no CPU path)");
    if (device < 0 || device >= ndev) return sfail(nullptr, MKT_E_ARG, "device %d of %d", device, ndev);
    if (len && !chromsizes) return sfail(nullptr, MKT_E_ARG, "null argument");
    mkt_pairstat* p = new mkt_pairstat();
    p->device = device;
    const std::string bad = mx_parse_table(chromsizes, len, p->names, p->lens);
    if (!bad.empty() && p->names.size() <= kPsMaxChrom) { delete p; return sfail(nullptr, MKT_E_ARG, "%s", bad.c_str()); }
    const size_t nc = p->names.size();
    if (nc > kPsMaxChrom) { delete p; return sfail(nullptr, MKT_E_RANGE, "chromosome table: %zu names, at most %u are taken (the chromosome-pair table is dense: 32 MB at the limit)", nc, kPsMaxChrom); }
    for (uint32_t i = 0; i < nc; ++i)
        if (!p->index.emplace(p->names[i], i).second) { const std::string nm = p->names[i]; delete p; return sfail(nullptr, MKT_E_ARG, "chromosome table: %s is there twice", nm.c_str()); }
    auto dfail = [&](const char* what, hipError_t e) { mkt_pairstat_destroy(p); return sfail(nullptr, e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return dfail("hipSetDevice", e);
    if ((e = p->stream.create(hipStreamNonBlocking)) != hipSuccess) return dfail("hipStreamCreate", e);
    if ((e = p->ev.create()) != hipSuccess) return dfail("hipEventCreate", e);
    std::vector<uint8_t> hostTab(sizeof(MxTab), 0);
    mx_tab_fill(reinterpret_cast<MxTab*>(hostTab.data()), p->names, p->lens);
    if ((e = p->d_tab.alloc(1)) != hipSuccess) return dfail("hipMalloc", e);
    if ((e = hipMemcpy(p->d_tab, hostTab.data(), sizeof(MxTab), hipMemcpyHostToDevice)) != hipSuccess) return dfail("hipMemcpy", e);
    if ((e = p->d_ctr.alloc(kPsCells + 1)) != hipSuccess) return dfail("hipMalloc", e);
    if ((e = hipMemset(p->d_ctr, 0, kPsCells * sizeof(unsigned long long))) != hipSuccess) return dfail("hipMemset", e);
    if ((e = hipMemset(p->d_ctr + kPsCells, 0xFF, sizeof(unsigned long long))) != hipSuccess) return dfail("hipMemset", e);
    if ((e = p->d_chrom.alloc(nc * nc)) != hipSuccess) return dfail("hipMalloc", e);
    if ((e = hipMemset(p->d_chrom, 0, nc * nc * sizeof(unsigned long long))) != hipSuccess) return dfail("hipMemset", e);
    *out = p;
    return MKT_OK;
}
void mkt_pairstat_destroy(mkt_pairstat* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;                                           // the buffers and the events, then the stream
}
const char* mkt_pairstat_error(const mkt_pairstat* p) { return p ? p->err.c_str() : g_ps_create_err.c_str(); }

int mkt_pairstat_add(mkt_pairstat* p, const char* bytes, size_t n) {
    if (!p || (n && !bytes)) return MKT_E_ARG;
    size_t end = n;                                     // bytes[0, end): up to the last newline
    while (end > 0 && bytes[end - 1] != '\n') --end;
    if (end == 0) { p->carry.append(bytes, n); return MKT_OK; }
    SCHK(p, hipSetDevice(p->device));
    const size_t c = p->carry.size();
    if (int rc = ps_reserve(p, c + end)) return rc;
    SCHK(p, hipEventRecord(p->ev[0], p->stream));
    if (c) SCHK(p, hipMemcpyAsync(p->text.get(), p->carry.data(), c, hipMemcpyHostToDevice, p->stream));
    SCHK(p, hipMemcpyAsync(p->text.get() + c, bytes, end, hipMemcpyHostToDevice, p->stream));
    SCHK(p, hipStreamSynchronize(p->stream));           // the caller may reuse `bytes`
    p->carry.assign(bytes + end, n - end);
    return ps_process(p, c + end);
}
int mkt_pairstat_add_device(mkt_pairstat* p, const void* d_bytes, size_t n) {
    if (!p || (n && !d_bytes)) return MKT_E_ARG;
    if (n == 0) return MKT_OK;
    SCHK(p, hipSetDevice(p->device));
    // the last newline of the piece, looked for from its end, a MiB of it on the host at a time
    const uint8_t* src = static_cast<const uint8_t*>(d_bytes);
    std::vector<char> win((size_t)1 << 20);
    size_t end = n;                                     // src[0, end): up to the last newline
    bool found = false;
    while (end > 0 && !found) {
        const size_t w = end < win.size() ? end : win.size();
        SCHK(p, hipMemcpy(win.data(), src + end - w, w, hipMemcpyDeviceToHost));
        size_t t = w;
        while (t > 0 && win[t - 1] != '\n') --t;
        if (t) { end = end - w + t; found = true; } else end -= w;
    }
    std::string tail(n - end, '\0');
    if (n - end) SCHK(p, hipMemcpy(&tail[0], src + end, n - end, hipMemcpyDeviceToHost));
    if (end == 0) { p->carry += tail; return MKT_OK; }
    const size_t c = p->carry.size();
    if (int rc = ps_reserve(p, c + end)) return rc;
    SCHK(p, hipEventRecord(p->ev[0], p->stream));
    if (c) SCHK(p, hipMemcpyAsync(p->text.get(), p->carry.data(), c, hipMemcpyHostToDevice, p->stream));
    SCHK(p, hipMemcpyAsync(p->text.get() + c, src, end, hipMemcpyDeviceToDevice, p->stream));
    SCHK(p, hipStreamSynchronize(p->stream));
    p->carry.swap(tail);
    return ps_process(p, c + end);
}
int mkt_pairstat_add_keys(mkt_pairstat* p, mkt_ctx* ctx, int drop_last, const uint8_t* skip_flags, size_t n_flags) {
    if (!p || !ctx) return MKT_E_ARG;
    const void* d_keys = nullptr;
    uint64_t n = 0;
    int rc = mkt_ext_keys_device(ctx, drop_last, &d_keys, &n);
    if (rc) return sfail(p, rc, "the context's key list: %s", mkt_last_error(ctx));
    if (n == 0) return MKT_OK;
    if (skip_flags && n_flags < n) return sfail(p, MKT_E_ARG, "%zu flags for %llu reported pairs", n_flags, (unsigned long long)n);
    hipPointerAttribute_t at;
    SCHK(p, hipPointerGetAttributes(&at, d_keys));
    if (at.device != p->device) return sfail(p, MKT_E_ARG, "the context lives on device %d, the statistics on device %d", at.device, p->device);
    // the context's chromosome slots -> table indices
    size_t tl = 0;
    if ((rc = mkt_ext_chr_names(ctx, nullptr, 0, &tl))) return sfail(p, rc, "the context's chromosome names: %s", mkt_last_error(ctx));
    std::string txt(tl, '\0');
    if (tl && (rc = mkt_ext_chr_names(ctx, &txt[0], tl, &tl))) return sfail(p, rc, "the context's chromosome names: %s", mkt_last_error(ctx));
    std::vector<uint16_t> lut(kChrSlots, (uint16_t)0xFFFFu);
    for (size_t q0 = 0; q0 < tl;) {
        size_t q = txt.find('\n', q0);
        if (q == std::string::npos) q = tl;
        const size_t t = txt.find('\t', q0);
        if (t != std::string::npos && t < q) {
            const unsigned long slot = strtoul(txt.c_str() + q0, nullptr, 10);
            const auto it = p->index.find(txt.substr(t + 1, q - t - 1));
            if (slot < kChrSlots && it != p->index.end()) lut[slot] = (uint16_t)it->second;
        }
        q0 = q + 1;
    }
    SCHK(p, hipSetDevice(p->device));
    const uint64_t grid = (n + kPsLinesPerWg - 1) / kPsLinesPerWg;
    if (grid > 0x7FFFFFFFull) return sfail(p, MKT_E_CAPACITY, "%llu reported pairs in one context", (unsigned long long)n);
    hipStream_t st = p->stream;
    DevBuf<uint16_t> d_lut;
    DevBuf<uint8_t> d_flags;
    SCHK(p, d_lut.alloc(kChrSlots));
    if (skip_flags) SCHK(p, d_flags.alloc(n));
    SCHK(p, hipEventRecord(p->ev[0], st));
    SCHK(p, hipMemcpyAsync(d_lut, lut.data(), kChrSlots * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    if (skip_flags) SCHK(p, hipMemcpyAsync(d_flags, skip_flags, n, hipMemcpyHostToDevice, st));
    SCHK(p, hipEventRecord(p->ev[2], st));
    hipLaunchKernelGGL(k_ps_keys, dim3((unsigned)grid), dim3(PSWG), 0, st, (const KeyRec*)d_keys, n, (const uint16_t*)d_lut.get(), (const uint8_t*)d_flags.get(),
                       (const MxTab*)p->d_tab.get(), (uint32_t)p->names.size(), p->d_ctr.get(), p->d_chrom.get());
    const hipError_t e = hipGetLastError();
    SCHK(p, hipEventRecord(p->ev[3], st));
    const hipError_t e2 = hipStreamSynchronize(st);     // the context may go on (and the host buffers be reused) when this returns
    if (e != hipSuccess || e2 != hipSuccess) return sfail(p, MKT_E_HIP, "statistics of %llu keys failed: %s", (unsigned long long)n, hipGetErrorString(e != hipSuccess ? e : e2));
    float b = 0, c = 0;
    SCHK(p, hipEventElapsedTime(&b, p->ev[2], p->ev[3]));
    SCHK(p, hipEventElapsedTime(&c, p->ev[0], p->ev[3]));
    p->ms[1] += b; p->ms[2] += c;
    p->ran = false;
    return MKT_OK;
}

void mkt_pairstat_opts_default(mkt_pairstat_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->tol_permille = 50; o->min_count = 1000;
}

int mkt_pairstat_run(mkt_pairstat* p, const mkt_pairstat_opts* opts, mkt_pairstat_info* info) {
    if (!p) return MKT_E_ARG;
    mkt_pairstat_opts o;
    mkt_pairstat_opts_default(&o);
    if (opts) o = *opts;
    if (o.reserved0) return sfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    for (uint32_t r : o.reserved) if (r) return sfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    if (info) memset(info, 0, sizeof *info);
    p->ran = false;
    if (!p->carry.empty()) {                            // a last line without its newline
        std::string last;
        last.swap(p->carry);
        last += '\n';
        if (int rc = mkt_pairstat_add(p, last.data(), last.size())) return rc;
    }
    SCHK(p, hipSetDevice(p->device));
    const size_t nc = p->names.size();
    std::vector<unsigned long long> hc(kPsCells + 1);
    p->chrom.assign(nc * nc, 0);
    SCHK(p, hipMemcpyAsync(hc.data(), p->d_ctr, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    SCHK(p, hipMemcpyAsync(p->chrom.data(), p->d_chrom, nc * nc * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
    SCHK(p, hipStreamSynchronize(p->stream));
    if (hc[kPsCells] != kPsNoBadLine)
        return sfail(p, MKT_E_FORMAT, "line %llu: fewer than five columns or a position that is not a plain decimal integer", (unsigned long long)(hc[kPsCells] + 1));
    p->ctr.assign(hc.begin(), hc.begin() + kPsCells);
    ps_finish(p->ctr.data(), p->chrom.data(), p->names, p->lens, o.tol_permille, o.min_count, p->res);
    p->ran = true;
    if (info) *info = p->res.info;
    return MKT_OK;
}

int mkt_pairstat_fetch_dist(mkt_pairstat* p, uint64_t* out) {
    if (!p || !out) return MKT_E_ARG;
    if (!p->ran) return sfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    memcpy(out, p->ctr.data(), kPsDistCells * sizeof(uint64_t));
    return MKT_OK;
}
int mkt_pairstat_fetch_chrom(mkt_pairstat* p, uint32_t first_row, uint32_t n_rows, uint64_t* out) {
    if (!p || (n_rows && !out)) return MKT_E_ARG;
    if (!p->ran) return sfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    const size_t nc = p->names.size();
    if (first_row > nc || n_rows > nc - first_row) return sfail(p, MKT_E_ARG, "rows [%u, %llu) of %zu", first_row, (unsigned long long)first_row + n_rows, nc);
    if (n_rows) memcpy(out, p->chrom.data() + (size_t)first_row * nc, (size_t)n_rows * nc * sizeof(uint64_t));
    return MKT_OK;
}
int mkt_pairstat_fetch_scaling(mkt_pairstat* p, uint64_t* edges, double* area, double* pp) {
    if (!p) return MKT_E_ARG;
    if (!p->ran) return sfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    if (edges) { for (int k = 0; k < kPsBins; ++k) edges[k] = kPsEdges[k]; edges[kPsBins] = kPsLastHi; }
    if (area) memcpy(area, p->res.area_d, sizeof p->res.area_d);
    if (pp) memcpy(pp, p->res.p, sizeof p->res.p);
    return MKT_OK;
}
long mkt_pairstat_text(mkt_pairstat* p, int which, char* out, size_t cap) {
    if (!p) return MKT_E_ARG;
    if (which != 0 && which != 1) return sfail(p, MKT_E_ARG, "text %d (0 the statistics, 1 the scaling table)", which);
    if (!p->ran) return sfail(p, MKT_E_STATE, "text before a run that succeeded");
    const std::string& s = which ? p->res.scaling : p->res.stat;
    if (out && s.size() <= cap) memcpy(out, s.data(), s.size());
    return (long)s.size();
}
int mkt_pairstat_timing(const mkt_pairstat* p, double* index_ms, double* kernel_ms, double* total_ms) {
    if (!p) return MKT_E_ARG;
    if (index_ms) *index_ms = p->ms[0];
    if (kernel_ms) *kernel_ms = p->ms[1];
    if (total_ms) *total_ms = p->ms[2];
    return MKT_OK;
}

}  // extern "C"
