// mkt_matrix.hip -- the last stage of the driver (microcket:520-554): reported pairs -> a binned contact matrix at several
// resolutions, on the GPU.  The .hic container is written by mkt_hic.hip from the cells made here; .cool is out of scope; what is computed here is what
// they spend their time on, the sparse upper-triangle matrix, handed back as arrays and as the COO text `cooler load -f coo` reads.
//
// Definition (include/mkt.h has it in full): chromosome i of length L_i owns ceil(L_i / r) bins in table order; a pair
// (chrA, posA, chrB, posB) adds 1 to cell (min, max) of its two bin ids; a pair with a chromosome that is not in the table or a
// position of 0 or past the chromosome's end is counted as skipped.  The result depends on the multiset of pairs only.
//
// Data: one 16-byte MxRec per pair stays resident (chromosome index and position of both sides); the .pairs text that produced it
// does not.  Per resolution: records -> u64 key = bin1 << B | bin2 (B = bits of nbins), the stable 7-bit LSD radix passes of the
// duplicate marker over the 2B significant bits (launch_radix64), then run-length reduction: head flags on key[j] != key[j - 1], a
// scan for the output slots, and a cell's count is the DIFFERENCE of two neighbouring head positions -- exact for runs of any length
// across tiles and workgroups, no atomics on the counts, no dependence on the order anything ran in.  Then the COO text: byte length
// per cell, a scan, a write through LDS.
// This file: the kernels, the object's life (create, add, run, destroy) and the fetches of the cells.  The object itself, its records
// and the guards are mkt_matrix_obj.h; every analysis on the cells serves its own entry points from its own mkt_<analysis>.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "mkt_matrix_obj.h"
#include "mkt_rle.h"
#include "mkt_launch.h"
#include "mkt_segred.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

constexpr int MXWG = 256;
enum { ME_FIELDS = 1 };                             // MxCounters::err

__device__ inline uint32_t mx_exscan(uint32_t v, uint32_t* total, uint32_t* sh /* [MXWG / 64] */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= d) inc += y; }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < MXWG / 64; ++w) { if (w < wv) pre += sh[w]; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}
// one add per wave for the two counters
__device__ inline void mx_count(bool skipped, bool none, MxCounters* c) {
    const uint64_t bs = __ballot(skipped), bn = __ballot(none);
    if ((threadIdx.x & 63) == 0) {
        if (bs) atomicAdd(&c->skipped, (unsigned long long)__popcll(bs));
        if (bn) atomicAdd(&c->none, (unsigned long long)__popcll(bn));
    }
}
__device__ inline MxRec mx_make(uint32_t ia, uint64_t pa, uint32_t ib, uint64_t pb, const MxTab* tab, bool* skipped) {
    MxRec r;
    const bool ok = ia < kChrSlots && ib < kChrSlots && pa >= 1 && pb >= 1 && pa <= tab->len[ia < kChrSlots ? ia : 0] && pb <= tab->len[ib < kChrSlots ? ib : 0];
    *skipped = !ok;
    r.ia = ok ? ia : MX_SKIP; r.pa = (uint32_t)pa; r.ib = ib; r.pb = (uint32_t)pb;
    return r;
}

// ---- .pairs text -> records: rid \t chr1 \t pos1 \t chr2 \t pos2 [\t ...] \n, one lane per line (the newline index is the sorter's)
__global__ __launch_bounds__(MXWG) void k_mx_parse(const uint8_t* text, const uint64_t* starts, uint64_t nlines, const MxTab* tab, MxRec* rec, MxCounters* cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool skipped = false, none = false;
    if (j < nlines) {
        const uint64_t ls = starts[j], le = starts[j + 1] - 1;                    // le: the newline
        MxRec r;
        r.ia = MX_NONE; r.pa = 0; r.ib = 0; r.pb = 0;
        if (ls < le && text[ls] == '#') none = true;                              // a 4DN header line
        else {
            uint64_t tabs[5];
            int nt = 0;
            for (uint64_t p = ls; p < le && nt < 5; ++p) if (text[p] == '\t') tabs[nt++] = p;
            if (nt < 4) { atomicOr(&cnt->err, (uint32_t)ME_FIELDS); none = true; }
            else {
                const uint64_t p5 = nt >= 5 ? tabs[4] : le;
                auto num = [&](uint64_t a, uint64_t b) -> uint64_t {              // a plain decimal field; anything past 2^32 only has to stay past it
                    uint64_t v = 0;
                    if (a == b) atomicOr(&cnt->err, (uint32_t)ME_FIELDS);
                    for (uint64_t p = a; p < b; ++p) {
                        const uint32_t d = (uint32_t)text[p] - (uint32_t)'0';
                        if (d > 9u) { atomicOr(&cnt->err, (uint32_t)ME_FIELDS); break; }
                        if (v < (1ull << 40)) v = v * 10 + d;
                    }
                    return v;
                };
                const uint32_t ia = mx_tab_find(tab, text, tabs[0] + 1, tabs[1]), ib = mx_tab_find(tab, text, tabs[2] + 1, tabs[3]);
                r = mx_make(ia, num(tabs[1] + 1, tabs[2]), ib, num(tabs[3] + 1, p5), tab, &skipped);
            }
        }
        rec[j] = r;
    }
    mx_count(skipped, none, cnt);
}

// ---- a context's key records (mkt_core.h KeyRec) -> records; lut: the context's chromosome slot -> table index (0xFFFF: not in the table)
__global__ __launch_bounds__(MXWG) void k_mx_from_keys(const KeyRec* keys, uint64_t n, const uint16_t* lut, const uint8_t* flags, const MxTab* tab, MxRec* rec, MxCounters* cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool skipped = false, none = false;
    if (j < n) {
        const KeyRec k = keys[j];
        MxRec r;
        if (flags && flags[j]) { none = true; r.ia = MX_NONE; r.pa = 0; r.ib = 0; r.pb = 0; }
        else {
            const uint32_t a = lut[(k.k0 >> 45) & (kChrSlots - 1u)], b = lut[(k.k0 >> 32) & (kChrSlots - 1u)];
            r = mx_make(a == 0xFFFFu ? MX_SKIP : a, k.k0 & 0xFFFFFFFFull, b == 0xFFFFu ? MX_SKIP : b, k.k1 >> 32, tab, &skipped);
        }
        rec[j] = r;
    }
    mx_count(skipped, none, cnt);
}

// ---- one resolution: key = bin1 << B | bin2, bin1 <= bin2; what is not binned gets nbins << B | nbins and sorts behind every cell
__global__ __launch_bounds__(MXWG) void k_mx_keys(const MxRec* rec, uint64_t n, const uint32_t* off, uint32_t r, int B, uint64_t nbins, uint64_t* key) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint4 x = reinterpret_cast<const uint4*>(rec)[j];
    uint64_t k = (nbins << B) | nbins;
    if (x.x < MX_NONE) {
        const uint32_t b1 = off[x.x] + (x.y - 1u) / r, b2 = off[x.z] + (x.w - 1u) / r;
        k = ((uint64_t)(b1 < b2 ? b1 : b2) << B) | (uint64_t)(b1 < b2 ? b2 : b1);
    }
    key[j] = k;
}
constexpr uint32_t MX_TILE = 8 * MXWG;                        // sorted keys per workgroup in the two head passes
__device__ inline bool mx_head(const uint64_t* key, uint64_t j) { return j == 0 || key[j] != key[j - 1]; }
__global__ __launch_bounds__(MXWG) void k_mx_head_count(const uint64_t* key, uint64_t nv, uint64_t* sums) {
    __shared__ uint32_t sh[MXWG / 64];
    const uint64_t b = (uint64_t)blockIdx.x * MX_TILE;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < MX_TILE / MXWG; ++k) { const uint64_t j = b + k * MXWG + threadIdx.x; if (j < nv && mx_head(key, j)) ++c; }
    uint32_t tot;
    (void)mx_exscan(c, &tot, sh);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
// sums: exclusive prefixes now.  Cell s = the s-th run: its two bin ids and the position of its head among the sorted keys.
__global__ __launch_bounds__(MXWG) void k_mx_cells(const uint64_t* key, uint64_t nv, const uint64_t* sums, int B, uint32_t* bin1, uint32_t* bin2, uint32_t* pos) {
    __shared__ uint32_t sh[MXWG / 64];
    const uint64_t b = (uint64_t)blockIdx.x * MX_TILE;
    uint64_t at = sums[blockIdx.x];
    const uint64_t lo = (1ull << B) - 1ull;                    // B <= 32
    for (uint32_t k = 0; k < MX_TILE / MXWG; ++k) {            // sub-tiles in order
        const uint64_t j = b + k * MXWG + threadIdx.x;
        const bool h = j < nv && mx_head(key, j);
        uint32_t tot;
        const uint32_t ex = mx_exscan(h ? 1u : 0u, &tot, sh);
        if (h) { const uint64_t x = key[j], s = at + ex; bin1[s] = (uint32_t)(x >> B); bin2[s] = (uint32_t)(x & lo); pos[s] = (uint32_t)j; }
        at += tot;
    }
}
// count = distance to the next head (the last run ends at nv); and the bytes of "bin1 \t bin2 \t count \n" per workgroup of cells
constexpr uint32_t MX_CPW = 4 * MXWG;                         // cells per workgroup in the text passes
constexpr uint32_t MX_LINE_MAX = 33;                          // 3 x 10 digits, 2 tabs, newline
__device__ inline uint32_t mx_line_len(uint32_t a, uint32_t b, uint32_t c) { return dec_digits(a) + dec_digits(b) + dec_digits(c) + 3u; }
__global__ __launch_bounds__(MXWG) void k_mx_counts(const uint32_t* bin1, const uint32_t* bin2, const uint32_t* pos, uint64_t nnz, uint64_t nv, uint32_t* count, uint64_t* tsums) {
    __shared__ uint32_t sh[MXWG / 64];
    const uint64_t b = (uint64_t)blockIdx.x * MX_CPW;
    uint32_t bytes = 0;
#pragma unroll
    for (uint32_t k = 0; k < MX_CPW / MXWG; ++k) {
        const uint64_t s = b + k * MXWG + threadIdx.x;
        if (s < nnz) {
            const uint32_t c = (uint32_t)((s + 1 < nnz ? (uint64_t)pos[s + 1] : nv) - pos[s]);
            count[s] = c;
            bytes += mx_line_len(bin1[s], bin2[s], c);
        }
    }
    uint32_t tot;
    (void)mx_exscan(bytes, &tot, sh);
    if (threadIdx.x == 0) tsums[blockIdx.x] = tot;
}
__device__ inline uint32_t mx_put(uint8_t* p, uint32_t v, uint8_t tail) {        // v in decimal and one byte behind it; returns the bytes written
    uint64_t hi8; uint32_t lo2;
    dec10(v, hi8, lo2);
    const uint32_t nd = dec_digits(v), drop = 10u - nd;
    for (uint32_t k = 0; k < nd; ++k) { const uint32_t q = drop + k; p[k] = (uint8_t)(q < 8u ? (hi8 >> (8u * q)) : ((uint64_t)lo2 >> (8u * (q - 8u)))); }
    p[nd] = tail;
    return nd + 1u;
}
// tsums: exclusive prefixes now.  The workgroup's lines are laid out in LDS and leave as aligned 4-byte stores.
__global__ __launch_bounds__(MXWG) void k_mx_text(const uint32_t* bin1, const uint32_t* bin2, const uint32_t* count, uint64_t nnz, const uint64_t* tsums, uint8_t* out) {
    __shared__ uint32_t sh[MXWG / 64];
    __shared__ uint32_t buf32[(MX_CPW * MX_LINE_MAX + 3) / 4 + 1];
    uint8_t* buf = reinterpret_cast<uint8_t*>(buf32);
    const uint64_t b = (uint64_t)blockIdx.x * MX_CPW;
    uint32_t carry = 0;
    for (uint32_t k = 0; k < MX_CPW / MXWG; ++k) {
        const uint64_t s = b + k * MXWG + threadIdx.x;
        uint32_t a = 0, c = 0, d = 0, len = 0;
        if (s < nnz) { a = bin1[s]; c = bin2[s]; d = count[s]; len = mx_line_len(a, c, d); }
        uint32_t tot;
        const uint32_t ex = mx_exscan(len, &tot, sh);
        if (s < nnz) {
            uint8_t* p = buf + carry + ex;
            p += mx_put(p, a, '\t');
            p += mx_put(p, c, '\t');
            (void)mx_put(p, d, '\n');
        }
        carry += tot;
    }
    __syncthreads();
    const uint32_t T = carry;                                                    // the workgroup's bytes
    uint8_t* dst = out + tsums[blockIdx.x];
    uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    if (head > T) head = T;
    if (threadIdx.x < head) dst[threadIdx.x] = buf[threadIdx.x];
    const uint32_t words = (T - head) / 4u;
    uint32_t* dw = reinterpret_cast<uint32_t*>(dst + head);
    for (uint32_t w = threadIdx.x; w < words; w += MXWG) {
        const uint8_t* q = buf + head + 4u * w;
        dw[w] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    const uint32_t done = head + 4u * words;
    if (threadIdx.x < T - done) dst[done + threadIdx.x] = buf[done + threadIdx.x];
}

}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------
thread_local std::string mkt::g_mx_create_err;     // the one the header declares

// the table's grammar (mx_parse_table), its lookup and how it is filled: mkt_chromtab.h

static void mx_free_results(mkt_matrix* m) {
    for (MxRes& r : m->res) mx_invalidate(r, MX_NEW_CELLS);
    m->vp = VpState();
    m->hic = HicState();
    m->ran = false;
}
static int mx_reserve_rec(mkt_matrix* m, uint64_t need) {
    if (need >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "%llu pairs: a matrix object holds fewer than 2^32 (counts are 32-bit)", (unsigned long long)need);
    if (need <= m->rec_cap) return MKT_OK;
    uint64_t ncap = m->rec_cap ? m->rec_cap : (1ull << 20);
    while (ncap < need) ncap *= 2;
    DevBuf<MxRec> nb;
    { hipError_t e_ = nb.alloc(ncap); if (e_ != hipSuccess) return mfail(m, MKT_E_NOMEM, "hipMalloc of %llu pair records failed: %s", (unsigned long long)ncap, hipGetErrorString(e_)); }
    if (m->d_rec) {
        MCHK(m, hipStreamSynchronize(m->stream));
        if (m->n) MCHK(m, hipMemcpy(nb, m->d_rec, m->n * sizeof(MxRec), hipMemcpyDeviceToDevice));
    }
    m->d_rec = std::move(nb); m->rec_cap = ncap;
    return MKT_OK;
}
static int mx_reserve_text(mkt_matrix* m, size_t need) {
    if (need <= m->text_cap) return MKT_OK;
    size_t ncap = m->text_cap ? m->text_cap : ((size_t)64 << 20);
    while (ncap < need) ncap *= 2;
    if (m->d_text) { MCHK(m, hipStreamSynchronize(m->stream)); m->d_text.reset(); m->text_cap = 0; }
    { hipError_t e_ = m->d_text.alloc(ncap, 64); if (e_ != hipSuccess) return mfail(m, MKT_E_NOMEM, "hipMalloc of %zu text bytes failed: %s", ncap, hipGetErrorString(e_)); }
    m->text_cap = ncap;
    return MKT_OK;
}
// d_text[0, n) holds whole lines: index them, one record per line behind the ones that are there
static int mx_process_text(mkt_matrix* m, size_t n) {
    if (n == 0) return MKT_OK;
    DevBuf<uint64_t> starts;
    uint64_t* d_starts = nullptr;
    uint64_t nl = 0;
    MCHK(m, sort_line_index(m->d_text, n, m->stream, &d_starts, &nl));
    starts.adopt(d_starts);
    int rc = nl ? mx_reserve_rec(m, m->n + nl) : MKT_OK;
    if (rc == MKT_OK && nl) {
        hipLaunchKernelGGL(k_mx_parse, dim3(grid_for(nl, MXWG)), dim3(MXWG), 0, m->stream, (const uint8_t*)m->d_text, (const uint64_t*)d_starts, nl,
                           (const MxTab*)m->d_tab, m->d_rec.get() + m->n, m->d_counters.get());
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) rc = mfail(m, MKT_E_HIP, "parsing %llu .pairs lines failed: %s", (unsigned long long)nl, hipGetErrorString(e));
        else m->n += nl;
    }
    return rc;
}

// the scratch of one mkt_matrix_run: the two key buffers and the counters of the radix passes, the sums of the scans
struct MxScratch {
    DevBuf<uint64_t> a, b, sums;
    DevBuf<uint32_t> radix, pos;                                         // pos: a resolution's head positions, until its time is taken
    hipError_t alloc(uint64_t n, uint64_t nv) {
        MKT_TRY(a.alloc(n, 64));
        MKT_TRY(b.alloc(n, 64));
        MKT_TRY(radix.alloc(0, radix64_count_bytes(n)));
        return sums.alloc(rle_sums_words(nv));
    }
};
namespace mkt {
size_t rle_sums_words(uint64_t nv) { return (size_t)((nv + MX_CPW - 1) / MX_CPW + 2); }        // (at most nv runs: room for the text passes' sums, which are more than the head passes')
hipError_t rle_reduce(const uint64_t* key, uint64_t nv, int B, uint64_t* sums, DevBuf<uint32_t>& hi, DevBuf<uint32_t>& lo, DevBuf<uint32_t>& cnt, DevBuf<uint32_t>& pos,
                      uint64_t* runs, uint64_t* text_bytes, hipStream_t st) {
    const uint64_t hblocks = (nv + MX_TILE - 1) / MX_TILE;
    hipLaunchKernelGGL(k_mx_head_count, dim3((unsigned)hblocks), dim3(MXWG), 0, st, key, nv, sums);
    MKT_TRY(launch_exscan(sums, hblocks, sums + hblocks, st));
    uint64_t nnz = 0, tb = 0;
    MKT_TRY(hipMemcpyAsync(&nnz, sums + hblocks, 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    *runs = nnz; *text_bytes = 0;
    if (nnz == 0 || nnz > nv) return hipSuccess;
    MKT_TRY(hi.alloc(nnz)); MKT_TRY(lo.alloc(nnz)); MKT_TRY(cnt.alloc(nnz));
    MKT_TRY(pos.alloc(nnz));
    hipLaunchKernelGGL(k_mx_cells, dim3((unsigned)hblocks), dim3(MXWG), 0, st, key, nv, (const uint64_t*)sums, B, hi.get(), lo.get(), pos.get());
    const uint64_t tblocks = (nnz + MX_CPW - 1) / MX_CPW;
    hipLaunchKernelGGL(k_mx_counts, dim3((unsigned)tblocks), dim3(MXWG), 0, st, (const uint32_t*)hi, (const uint32_t*)lo, (const uint32_t*)pos, nnz, nv, cnt.get(), sums);
    MKT_TRY(launch_exscan(sums, tblocks, sums + tblocks, st));
    MKT_TRY(hipMemcpyAsync(&tb, sums + tblocks, 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    *text_bytes = tb;
    return hipGetLastError();
}
}  // namespace mkt
// one resolution's cells and COO text from the n records (nv of them binned).  A cell count that cannot be (0, or above nv) is left
// in r.nnz for the caller and nothing more is done.
static hipError_t mx_bin(mkt_matrix* m, MxRes& r, MxScratch& sc, uint64_t n, uint64_t nv) {
    hipStream_t st = m->stream;
    uint64_t *kA = sc.a, *kB = sc.b, *sums = sc.sums;                    // the passes swap the two as needed
    hipLaunchKernelGGL(k_mx_keys, dim3(grid_for(n, MXWG)), dim3(MXWG), 0, st, (const MxRec*)m->d_rec, n, (const uint32_t*)r.d_off, r.r, r.B, r.nbins, kA);
    MKT_TRY(launch_radix64(kA, kB, n, 0, 2 * r.B, sc.radix, st));
    uint64_t nnz = 0, tb = 0;
    MKT_TRY(rle_reduce(kA, nv, r.B, sums, r.d_b1, r.d_b2, r.d_cnt, sc.pos, &nnz, &tb, st));
    r.nnz = nnz;
    if (nnz == 0 || nnz > nv) return hipSuccess;
    const uint64_t tblocks = (nnz + MX_CPW - 1) / MX_CPW;
    MKT_TRY(r.d_text.alloc(tb, 64));
    hipLaunchKernelGGL(k_mx_text, dim3((unsigned)tblocks), dim3(MXWG), 0, st, (const uint32_t*)r.d_b1, (const uint32_t*)r.d_b2, (const uint32_t*)r.d_cnt, nnz, (const uint64_t*)sums, r.d_text.get());
    MKT_TRY(hipGetLastError());
    r.text_bytes = tb;
    return hipSuccess;
}

extern "C" {

int mkt_matrix_create(int device, const char* chromsizes, size_t len, const uint32_t* resolutions, uint32_t n_res, mkt_matrix** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return mfail(nullptr, MKT_E_NO_DEVICE, "no usable HIP device (there is no CPU path)");
    if (device < 0 || device >= ndev) return mfail(nullptr, MKT_E_ARG, "device %d of %d", device, ndev);
    if ((len && !chromsizes) || !resolutions) return mfail(nullptr, MKT_E_ARG, "null argument");
    if (n_res == 0 || n_res > 16) return mfail(nullptr, MKT_E_ARG, "%u resolutions: 1 .. 16 per matrix object", n_res);
    mkt_matrix* m = new mkt_matrix();
    m->device = device;
    const std::string bad = mx_parse_table(chromsizes, len, m->names, m->lens);
    if (!bad.empty()) { delete m; return mfail(nullptr, MKT_E_ARG, "%s", bad.c_str()); }
    const uint32_t nc = (uint32_t)m->names.size();
    for (uint32_t i = 0; i < nc; ++i)
        if (!m->index.emplace(m->names[i], i).second) { const std::string nm = m->names[i]; delete m; return mfail(nullptr, MKT_E_ARG, "chromosome table: %s is there twice", nm.c_str()); }
    m->res.resize(n_res);
    for (uint32_t k = 0; k < n_res; ++k) {
        MxRes& r = m->res[k];
        r.r = resolutions[k];
        if (r.r == 0) { delete m; return mfail(nullptr, MKT_E_ARG, "resolution %u of the list is 0", k); }
        r.off.resize(nc);
        uint64_t nb = 0;
        for (uint32_t i = 0; i < nc; ++i) { r.off[i] = (uint32_t)nb; nb += ((uint64_t)m->lens[i] + r.r - 1) / r.r; if (nb >= (1ull << 32)) break; }
        if (nb >= (1ull << 32)) { const uint32_t rr = r.r; delete m; return mfail(nullptr, MKT_E_CAPACITY, "resolution %u: 2^32 bins or more (bin ids are 32-bit)", rr); }
        r.nbins = nb;
        r.B = 0;
        while (r.B < 32 && (1ull << r.B) <= nb) ++r.B;              // nbins itself (the key of what is not binned) fits B bits
    }
    // the device side
    auto dfail = [&](const char* what, hipError_t e) { mkt_matrix_destroy(m); return mfail(nullptr, MKT_E_HIP, "%s failed: %s", what, hipGetErrorString(e)); };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return dfail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking)) != hipSuccess) return dfail("hipStreamCreate", e);
    if ((e = hipEventCreate(&m->ev0)) != hipSuccess || (e = hipEventCreate(&m->ev1)) != hipSuccess) return dfail("hipEventCreate", e);
    std::vector<uint8_t> hostTab(sizeof(MxTab), 0);
    MxTab* ht = reinterpret_cast<MxTab*>(hostTab.data());
    mx_tab_fill(ht, m->names, m->lens);
    if ((e = m->d_tab.alloc(1)) != hipSuccess) return dfail("hipMalloc", e);
    if ((e = hipMemcpy(m->d_tab, ht, sizeof(MxTab), hipMemcpyHostToDevice)) != hipSuccess) return dfail("hipMemcpy", e);
    if ((e = m->d_counters.alloc(1)) != hipSuccess) return dfail("hipMalloc", e);
    if ((e = hipMemset(m->d_counters, 0, sizeof(MxCounters))) != hipSuccess) return dfail("hipMemset", e);
    for (MxRes& r : m->res) {
        if ((e = r.d_off.alloc(nc)) != hipSuccess) return dfail("hipMalloc", e);
        if ((e = hipMemcpy(r.d_off, r.off.data(), (size_t)nc * 4, hipMemcpyHostToDevice)) != hipSuccess) return dfail("hipMemcpy", e);
    }
    *out = m;
    return MKT_OK;
}

void mkt_matrix_destroy(mkt_matrix* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    m->res.clear();                                                     // every device buffer goes with its owner, before the stream
    m->hic = HicState();
    m->d_tab.reset(); m->d_counters.reset(); m->d_rec.reset(); m->d_text.reset();
    if (m->ev0) (void)hipEventDestroy(m->ev0);
    if (m->ev1) (void)hipEventDestroy(m->ev1);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}
const char* mkt_matrix_error(const mkt_matrix* m) { return m ? m->err.c_str() : g_mx_create_err.c_str(); }

int mkt_matrix_add(mkt_matrix* m, const char* bytes, size_t n) {
    if (!m || (n && !bytes)) return MKT_E_ARG;
    MCHK(m, hipSetDevice(m->device));
    size_t end = n;                                                    // bytes[0, end): up to the last newline
    while (end > 0 && bytes[end - 1] != '\n') --end;
    if (end == 0) { m->carry.append(bytes, n); return MKT_OK; }
    if (m->ran) mx_free_results(m);
    const size_t c = m->carry.size();
    int rc = mx_reserve_text(m, c + end);
    if (rc) return rc;
    if (c) MCHK(m, hipMemcpyAsync(m->d_text, m->carry.data(), c, hipMemcpyHostToDevice, m->stream));
    MCHK(m, hipMemcpyAsync(m->d_text.get() + c, bytes, end, hipMemcpyHostToDevice, m->stream));
    MCHK(m, hipStreamSynchronize(m->stream));                          // the caller may reuse `bytes`
    m->carry.assign(bytes + end, n - end);
    return mx_process_text(m, c + end);
}
int mkt_matrix_add_device(mkt_matrix* m, const void* d_bytes, size_t n) {
    if (!m || (n && !d_bytes)) return MKT_E_ARG;
    MCHK(m, hipSetDevice(m->device));
    if (n == 0) return MKT_OK;
    if (!m->carry.empty()) return mfail(m, MKT_E_STATE, "device text behind an incomplete host line");
    if (m->ran) mx_free_results(m);
    int rc = mx_reserve_text(m, n + 1);
    if (rc) return rc;
    MCHK(m, hipMemcpyAsync(m->d_text, d_bytes, n, hipMemcpyDeviceToDevice, m->stream));
    char last = 0;
    MCHK(m, hipMemcpyAsync(&last, m->d_text.get() + n - 1, 1, hipMemcpyDeviceToHost, m->stream));
    MCHK(m, hipStreamSynchronize(m->stream));
    if (last != '\n') { const char nl = '\n'; MCHK(m, hipMemcpy(m->d_text.get() + n, &nl, 1, hipMemcpyHostToDevice)); ++n; }
    return mx_process_text(m, n);
}
int mkt_matrix_add_keys(mkt_matrix* m, mkt_ctx* ctx, int drop_last, const uint8_t* skip_flags, size_t n_flags) {
    if (!m || !ctx) return MKT_E_ARG;
    const void* d_keys = nullptr;
    uint64_t n = 0;
    int rc = mkt_ext_keys_device(ctx, drop_last, &d_keys, &n);
    if (rc) return mfail(m, rc, "the context's key list: %s", mkt_last_error(ctx));
    if (n == 0) return MKT_OK;
    if (skip_flags && n_flags < n) return mfail(m, MKT_E_ARG, "%zu flags for %llu reported pairs", n_flags, (unsigned long long)n);
    hipPointerAttribute_t at;
    MCHK(m, hipPointerGetAttributes(&at, d_keys));
    if (at.device != m->device) return mfail(m, MKT_E_ARG, "the context lives on device %d, the matrix on device %d", at.device, m->device);
    // the context's chromosome slots -> table indices
    size_t tl = 0;
    if ((rc = mkt_ext_chr_names(ctx, nullptr, 0, &tl))) return mfail(m, rc, "the context's chromosome names: %s", mkt_last_error(ctx));
    std::string txt(tl, '\0');
    if (tl && (rc = mkt_ext_chr_names(ctx, &txt[0], tl, &tl))) return mfail(m, rc, "the context's chromosome names: %s", mkt_last_error(ctx));
    std::vector<uint16_t> lut(kChrSlots, (uint16_t)0xFFFFu);
    for (size_t p = 0; p < tl;) {
        size_t q = txt.find('\n', p);
        if (q == std::string::npos) q = tl;
        const size_t t = txt.find('\t', p);
        if (t != std::string::npos && t < q) {
            const unsigned long slot = strtoul(txt.c_str() + p, nullptr, 10);
            const auto it = m->index.find(txt.substr(t + 1, q - t - 1));
            if (slot < kChrSlots && it != m->index.end()) lut[slot] = (uint16_t)it->second;
        }
        p = q + 1;
    }
    MCHK(m, hipSetDevice(m->device));
    if (m->ran) mx_free_results(m);
    if ((rc = mx_reserve_rec(m, m->n + n))) return rc;
    DevBuf<uint16_t> d_lut;
    DevBuf<uint8_t> d_flags;
    MCHK(m, d_lut.alloc(kChrSlots));
    hipError_t e = hipMemcpyAsync(d_lut, lut.data(), kChrSlots * sizeof(uint16_t), hipMemcpyHostToDevice, m->stream);
    if (e == hipSuccess && skip_flags) {
        e = d_flags.alloc(n);
        if (e == hipSuccess) e = hipMemcpyAsync(d_flags, skip_flags, n, hipMemcpyHostToDevice, m->stream);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_mx_from_keys, dim3(grid_for(n, MXWG)), dim3(MXWG), 0, m->stream, (const KeyRec*)d_keys, n, (const uint16_t*)d_lut,
                           (const uint8_t*)d_flags, (const MxTab*)m->d_tab, m->d_rec.get() + m->n, m->d_counters.get());
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(m->stream);             // the context may go on (and the host buffers be reused) when this returns
    if (e != hipSuccess || e2 != hipSuccess) return mfail(m, MKT_E_HIP, "records from %llu keys failed: %s", (unsigned long long)n, hipGetErrorString(e != hipSuccess ? e : e2));
    m->n += n;
    return MKT_OK;
}

int mkt_matrix_run(mkt_matrix* m, uint64_t* pairs, uint64_t* skipped) {
    if (!m) return MKT_E_ARG;
    if (pairs) *pairs = 0;
    if (skipped) *skipped = 0;
    MCHK(m, hipSetDevice(m->device));
    if (!m->carry.empty()) {                                            // a last line without its newline
        std::string last;
        last.swap(m->carry);
        last += '\n';
        const int rc = mkt_matrix_add(m, last.data(), last.size());
        if (rc) return rc;
    }
    mx_free_results(m);
    hipStream_t st = m->stream;
    MxCounters hc;
    MCHK(m, hipMemcpyAsync(&hc, m->d_counters, sizeof hc, hipMemcpyDeviceToHost, st));
    MCHK(m, hipStreamSynchronize(st));
    if (hc.err) return mfail(m, MKT_E_ARG, "not .pairs text (error bits 0x%x: 1 = fewer than five fields / non-decimal position)", hc.err);
    const uint64_t n = m->n, nv = n - hc.skipped - hc.none;
    m->pairs = n - hc.none; m->skipped = hc.skipped;
    MxScratch sc;
    const hipError_t ea = nv ? sc.alloc(n, nv) : hipSuccess;
    if (ea != hipSuccess) return mfail(m, MKT_E_NOMEM, "hipMalloc of the sort scratch of %llu pairs failed: %s", (unsigned long long)n, hipGetErrorString(ea));
    for (MxRes& r : m->res) {
        if (nv == 0) continue;
        const hipError_t e = mx_timed(m, &r.ms, [&] { return mx_bin(m, r, sc, n, nv); });
        sc.pos.reset();
        if (e == hipSuccess && r.nnz != 0 && r.nnz <= nv) continue;
        const uint64_t nnz = r.nnz;
        mx_free_results(m);                                              // a failure leaves no half-made result behind
        if (e != hipSuccess) return mx_hip(m, "run: ", e, true);
        return mfail(m, MKT_E_KERNEL, "%llu cells from %llu binned pairs", (unsigned long long)nnz, (unsigned long long)nv);
    }
    m->ran = true;
    if (pairs) *pairs = m->pairs;
    if (skipped) *skipped = m->skipped;
    return MKT_OK;
}

int mkt_matrix_info(const mkt_matrix* m, uint32_t res_index, uint64_t* nbins, uint64_t* nnz, uint64_t* text_bytes) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const MxRes& r = m->res[res_index];
    if (nbins) *nbins = r.nbins;
    if (nnz) *nnz = m->ran ? r.nnz : 0;
    if (text_bytes) *text_bytes = m->ran ? r.text_bytes : 0;
    return MKT_OK;
}
int mkt_matrix_timing(const mkt_matrix* m, uint32_t res_index, double* ms) {
    if (!m || !ms || res_index >= m->res.size()) return MKT_E_ARG;
    *ms = m->ran ? m->res[res_index].ms : 0.0;
    return MKT_OK;
}
int mkt_matrix_fetch(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint32_t* bin1, uint32_t* bin2, uint32_t* count) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_RAN, "fetch");
    const MxRes& r = *rp;
    if (first > r.nnz || n > r.nnz - first) return mfail(m, MKT_E_ARG, "cells [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)r.nnz);
    MCHK(m, hipSetDevice(m->device));
    if (n == 0) return MKT_OK;
    if (bin1) MCHK(m, hipMemcpy(bin1, r.d_b1.get() + first, n * 4, hipMemcpyDeviceToHost));
    if (bin2) MCHK(m, hipMemcpy(bin2, r.d_b2.get() + first, n * 4, hipMemcpyDeviceToHost));
    if (count) MCHK(m, hipMemcpy(count, r.d_cnt.get() + first, n * 4, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_matrix_fetch_text(mkt_matrix* m, uint32_t res_index, uint64_t off, char* out, size_t n) {
    if (n && !out) return MKT_E_ARG;
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_RAN, "fetch");
    const MxRes& r = *rp;
    if (off > r.text_bytes || n > r.text_bytes - off) return mfail(m, MKT_E_ARG, "range past the end of the COO text");
    MCHK(m, hipSetDevice(m->device));
    if (n) MCHK(m, hipMemcpy(out, r.d_text.get() + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

}  // extern "C"
