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
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_balance.h"
#include "mkt_expected.h"
#include "mkt_loops.h"
#include "mkt_eigs.h"
#include "mkt_insulation.h"
#include "mkt_pileup.h"
#include "mkt_saddle.h"
#include "mkt_scc.h"
#include "mkt_viewpoint.h"
#include "mkt_hic.h"
#include "mkt_rle.h"
#include "mkt_launch.h"
#include "mkt_layout.h"
#include "mkt_segred.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

constexpr int MXWG = 256;
constexpr uint32_t MX_SKIP = 0xFFFFFFFFu;          // MxRec::ia of a skipped pair
constexpr uint32_t MX_NONE = 0xFFFFFFFEu;          // ... of something that is not a pair (a '#' line, a pair left out by its flag)
struct MxRec { uint32_t ia, pa, ib, pb; };         // table index and 1-based position of the two sides
static_assert(sizeof(MxRec) == 16, "one 16-byte vector per pair");

// the given table, read-only on the device: open addressing over FNV-1a of the name (nothing is ever inserted by a kernel)
constexpr uint32_t kMxSlots = 2 * kChrSlots;
struct MxTab {
    unsigned long long hash[kMxSlots];             // 0 = empty
    uint16_t idx[kMxSlots];                        // table index of the slot's name
    uint8_t name[kChrSlots][64];                   // by table index; [63] = length (<= 63)
    uint32_t len[kChrSlots];                       // L_i
};
enum { ME_FIELDS = 1 };
struct MxCounters { unsigned long long skipped, none; uint32_t err, pad; };

__host__ __device__ inline uint64_t mx_fnv(const uint8_t* p, uint64_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h ? h : 1ull;
}
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
                auto find = [&](uint64_t a, uint64_t b) -> uint32_t {
                    const uint64_t L = b - a;
                    if (L == 0 || L > 63) return MX_SKIP;
                    const uint64_t h = mx_fnv(text + a, L);
                    uint32_t s = (uint32_t)(h >> 17) & (kMxSlots - 1u);
                    for (uint32_t probe = 0; probe < kMxSlots; ++probe) {
                        const unsigned long long cur = tab->hash[s];
                        if (cur == 0ull) return MX_SKIP;
                        if (cur == h) {
                            const uint32_t i = tab->idx[s];
                            const uint8_t* nm = tab->name[i];
                            bool same = nm[63] == (uint8_t)L;
                            for (uint64_t k = 0; same && k < L; ++k) same = nm[k] == text[a + k];
                            if (same) return i;
                        }
                        s = (s + 1u) & (kMxSlots - 1u);
                    }
                    return MX_SKIP;
                };
                const uint32_t ia = find(tabs[0] + 1, tabs[1]), ib = find(tabs[2] + 1, tabs[3]);
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
namespace {
struct MxRes {
    uint32_t r = 0;
    uint64_t nbins = 0;
    int B = 0;
    std::vector<uint32_t> off;
    DevBuf<uint32_t> d_off;
    uint64_t nnz = 0, text_bytes = 0;
    DevBuf<uint32_t> d_b1, d_b2, d_cnt;
    DevBuf<uint8_t> d_text;
    double ms = 0;
    MxLayout lay;                                   // built on demand by whoever needs it first; lives as long as the cells
    // balancing (mkt_matrix_balance): the weights live until the next balance or run
    DevBuf<double> d_w;
    bool balanced = false;
    double bal_setup_ms = 0, bal_iter_ms = 0;
    // expected tables (mkt_matrix_expected): the grouping lives as long as the cells, the tables until the next balance or run
    ExpSetup exs;
    ExpTables ext;
    double exp_setup_ms = 0, exp_sums_ms = 0;
    // loop calling (mkt_matrix_loops): the results live until the next expected, balance or run
    LoopsState lps;
    // compartment eigenvectors (mkt_matrix_eigs): the results live until the next expected, balance or run
    EigsState egs;
    // insulation scores and boundaries (mkt_matrix_insulation): the results live until the next balance or run
    InsState ins;
    // pileup (mkt_matrix_pileup): the results live until the next expected, balance or run
    PileState pile;
    // saddle tables (mkt_matrix_saddle): the results live until the next expected, balance or run
    SaddleState sad;
    // replicate comparison (mkt_matrix_scc): the results live until the next balance or run
    SccState scc;
};
thread_local std::string g_mx_create_err;
}  // namespace

struct mkt_matrix {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    std::unordered_map<std::string, uint32_t> index;
    DevBuf<MxTab> d_tab;
    DevBuf<MxCounters> d_counters;
    DevBuf<MxRec> d_rec; uint64_t rec_cap = 0, n = 0;
    DevBuf<uint8_t> d_text; size_t text_cap = 0;
    std::string carry;                              // an incomplete last line of the text seen so far
    bool ran = false;
    uint64_t pairs = 0, skipped = 0;
    std::vector<MxRes> res;
    VpState vp;                                     // viewpoint profiles (mkt_matrix_viewpoint): the results live until the next add or run
    HicState hic;                                   // the .hic file (mkt_matrix_hic): the image lives until the next add or run
    std::string err;
};

static int mfail(mkt_matrix* m, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m) m->err = buf; else g_mx_create_err = buf;
    return code;
}
// a HIP error of section `sec` ("balance: ", ...); oom_own: out of memory has its own code there (the analyses and the run)
static int mx_hip(mkt_matrix* m, const char* sec, hipError_t e, bool oom_own) {
    return mfail(m, oom_own && e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "%sHIP call failed: %s", sec, hipGetErrorString(e));
}
#define MX(m, sec, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return mx_hip((m), (sec), e_, true); } while (0)
#define MCHK(m, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return mx_hip((m), "", e_, false); } while (0)

// lines name \t length [\t ...]; empty lines and '#' lines are ignored.  Returns an empty string or what is wrong.
static std::string mx_parse_table(const char* txt, size_t len, std::vector<std::string>& names, std::vector<uint32_t>& lens) {
    size_t p = 0, line = 0;
    char msg[160];
    while (p < len) {
        const char* nlp = (const char*)memchr(txt + p, '\n', len - p);
        size_t q = nlp ? (size_t)(nlp - txt) : len, e = q;
        ++line;
        if (e > p && txt[e - 1] == '\r') --e;
        if (e > p && txt[p] != '#') {
            size_t t = p;
            while (t < e && txt[t] != '\t') ++t;
            if (t == p || t - p > 63) { snprintf(msg, sizeof msg, "chromosome table line %zu: a name of 1 .. 63 bytes is needed", line); return msg; }
            size_t d = t + 1;
            uint64_t v = 0;
            size_t nd = 0;
            while (d < e && txt[d] >= '0' && txt[d] <= '9' && nd < 11) { v = v * 10 + (uint64_t)(txt[d] - '0'); ++d; ++nd; }
            if (t >= e || nd == 0 || (d < e && txt[d] != '\t') || v > 0xFFFFFFFFull) { snprintf(msg, sizeof msg, "chromosome table line %zu: no length (name<TAB>length, length < 2^32)", line); return msg; }
            names.emplace_back(txt + p, t - p);
            lens.push_back((uint32_t)v);
        }
        p = q + 1;
    }
    if (names.empty()) return "chromosome table: no chromosome";
    if (names.size() > kChrSlots) return "chromosome table: more than 8192 chromosomes";
    return "";
}

static void mx_free_results(mkt_matrix* m) {
    for (MxRes& r : m->res) {
        r.d_b1.reset(); r.d_b2.reset(); r.d_cnt.reset(); r.d_text.reset();
        r.nnz = 0; r.text_bytes = 0; r.ms = 0;
        r.lay = MxLayout();
        r.d_w.reset(); r.balanced = false; r.bal_setup_ms = r.bal_iter_ms = 0;
        r.exs = ExpSetup(); r.ext = ExpTables();
        r.exp_setup_ms = r.exp_sums_ms = 0;
        r.lps = LoopsState(); r.egs = EigsState();
        r.ins = InsState();
        r.pile = PileState();
        r.sad = SaddleState();
        r.scc = SccState();
    }
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

// what an entry point needs of a resolution before it may go on; each has its message
enum { MX_RAN = 1, MX_WEIGHTS = 2, MX_TABLES = 4, MX_LOOPS = 8, MX_EIGS = 16, MX_INS = 32, MX_PILE = 64, MX_SADDLE = 128, MX_SCC = 256 };
static int mx_need(mkt_matrix* m, uint32_t res_index, const MxRes& r, int need, const char* what = nullptr) {
    if ((need & MX_RAN) && !m->ran) return mfail(m, MKT_E_STATE, "%s before run", what);
    if ((need & MX_WEIGHTS) && !(m->ran && r.balanced)) return mfail(m, MKT_E_STATE, "no weights for resolution index %u: balance first", res_index);
    if ((need & MX_TABLES) && !(m->ran && r.ext.built)) return mfail(m, MKT_E_STATE, "no expected tables for resolution index %u: expected first", res_index);
    if ((need & MX_LOOPS) && !(m->ran && r.lps.built)) return mfail(m, MKT_E_STATE, "no loops for resolution index %u: loops first", res_index);
    if ((need & MX_EIGS) && !(m->ran && r.egs.built)) return mfail(m, MKT_E_STATE, "no eigenvectors for resolution index %u: eigs first", res_index);
    if ((need & MX_INS) && !(m->ran && r.ins.built)) return mfail(m, MKT_E_STATE, "no insulation scores for resolution index %u: insulation first", res_index);
    if ((need & MX_PILE) && !(m->ran && r.pile.built)) return mfail(m, MKT_E_STATE, "no pileup for resolution index %u: pileup first", res_index);
    if ((need & MX_SADDLE) && !(m->ran && r.sad.built)) return mfail(m, MKT_E_STATE, "no saddle tables for resolution index %u: saddle first", res_index);
    if ((need & MX_SCC) && !(m->ran && r.scc.built)) return mfail(m, MKT_E_STATE, "no comparison for resolution index %u: scc first", res_index);
    return MKT_OK;
}
// the resolution of an entry point, or the error: the object, the index, then what it needs
static int mx_res(mkt_matrix* m, uint32_t res_index, MxRes** r, int need = 0, const char* what = nullptr) {
    if (!m) return MKT_E_ARG;
    if (res_index >= m->res.size()) return mfail(m, MKT_E_ARG, "resolution index %u of %zu", res_index, m->res.size());
    *r = &m->res[res_index];
    return mx_need(m, res_index, **r, need, what);
}
#define MX_RES(...) do { const int rc_ = mx_res(__VA_ARGS__); if (rc_) return rc_; } while (0)
// the resident cells of a resolution, as the layout and the analyses take them
static MxCells mx_cells(const MxRes& r) {
    MxCells c;
    c.b1 = r.d_b1; c.b2 = r.d_b2; c.cnt = r.d_cnt; c.off = r.d_off;
    c.nnz = r.nnz; c.nbins = r.nbins; c.nchr = (uint32_t)r.off.size(); c.B = r.B;
    return c;
}
// device time of work() between the object's two events; the stream is idle when it returns
template <typename F>
static hipError_t mx_timed(mkt_matrix* m, double* ms_out, F&& work) {
    MKT_TRY(hipEventRecord(m->ev0, m->stream));
    MKT_TRY(work());
    MKT_TRY(hipEventRecord(m->ev1, m->stream));
    MKT_TRY(hipStreamSynchronize(m->stream));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
    *ms_out = ms;
    return hipSuccess;
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
    for (uint32_t i = 0; i < nc; ++i) {
        const std::string& nm = m->names[i];
        memcpy(ht->name[i], nm.data(), nm.size());
        ht->name[i][63] = (uint8_t)nm.size();
        ht->len[i] = m->lens[i];
        const uint64_t h = mx_fnv((const uint8_t*)nm.data(), nm.size());
        uint32_t s = (uint32_t)(h >> 17) & (kMxSlots - 1u);
        while (ht->hash[s]) s = (s + 1u) & (kMxSlots - 1u);            // at most 8192 names in 16384 slots
        ht->hash[s] = h; ht->idx[s] = (uint16_t)i;
    }
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

// ---- balancing: the entry points; the kernels are mkt_balance.hip, the definition is in include/mkt.h ------------------------
void mkt_balance_opts_default(mkt_balance_opts* o) {
    if (!o) return;
    o->ignore_diags = 2; o->min_nnz = 10; o->min_count = 0.0; o->mad_max = 5.0; o->tol = 1e-5; o->max_iters = 200; o->reserved = 0;
}

int mkt_matrix_balance(mkt_matrix* m, uint32_t res_index, const mkt_balance_opts* opts, mkt_balance_stats* stats) {
    if (m && stats) memset(stats, 0, sizeof *stats);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_balance_opts o;
    mkt_balance_opts_default(&o);
    if (opts) o = *opts;
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "balance: ignore_diags %d is negative", o.ignore_diags);
    if (o.min_nnz < 0) return mfail(m, MKT_E_ARG, "balance: min_nnz %d is negative", o.min_nnz);
    if (!(o.min_count >= 0.0)) return mfail(m, MKT_E_ARG, "balance: min_count %g is negative or NaN", o.min_count);
    if (!(o.mad_max >= 0.0)) return mfail(m, MKT_E_ARG, "balance: mad_max %g is negative or NaN", o.mad_max);
    if (!(o.tol >= 0.0)) return mfail(m, MKT_E_ARG, "balance: tol %g is negative or NaN", o.tol);
    if (o.max_iters <= 0) return mfail(m, MKT_E_ARG, "balance: max_iters %d (at least 1 is needed)", o.max_iters);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "balance: the reserved field is not 0");
    if (const int rc = mx_need(m, res_index, *rp, MX_RAN, "balance")) return rc;
    if (m->res[res_index].nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "balance: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)m->res[res_index].nnz);
    MCHK(m, hipSetDevice(m->device));
    MxRes& r = *rp;
    hipStream_t st = m->stream;
    const uint64_t nb = r.nbins;
    r.d_w.reset();
    r.balanced = false; r.bal_iter_ms = 0;
    r.ext = ExpTables();                                                // tables of other weights
    r.lps = LoopsState(); r.egs = EigsState();
    r.ins = InsState();                                                 // scores of other weights
    r.pile = PileState();
    r.sad = SaddleState();
    r.scc = SccState();                                                 // a comparison under other weights
    DevBuf<double> d_bias, d_m, d_part, d_w;                            // d_w becomes r.d_w at the end: a failure leaves no weights
    DevBuf<BalState> d_state;
#define BRUN(call) MX(m, "balance: ", call)
    r.bal_setup_ms = 0;
    if (!r.lay.has_full) BRUN(mx_timed(m, &r.bal_setup_ms, [&] { return layout_full(r.lay, mx_cells(r), st); }));
    BRUN(d_bias.alloc(nb, 64));
    BRUN(d_m.alloc(nb, 64));
    BRUN(d_w.alloc(nb, 64));
    BRUN(d_part.alloc(0, bal_partial_bytes(nb)));
    BRUN(d_state.alloc(1));
    BRUN(hipMemsetAsync(d_state, 0, sizeof(BalState), st));

    // steps 2 and 3 on the host, from one nbins-sized copy of the exact (integer-valued) marginals
    std::vector<double> bias(nb, 1.0), hm(nb);
    const uint32_t ig = (uint32_t)o.ignore_diags;
    if (o.min_nnz > 0) {
        BRUN(bal_marginal(r.lay, r.d_b2, r.d_cnt, nb, ig, true, nullptr, d_m, st));
        BRUN(hipMemcpyAsync(hm.data(), d_m, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        BRUN(hipStreamSynchronize(st));
        for (uint64_t k = 0; k < nb; ++k) if (hm[k] < (double)o.min_nnz) bias[k] = 0.0;
    }
    BRUN(hipMemcpyAsync(d_bias, bias.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
    BRUN(bal_marginal(r.lay, r.d_b2, r.d_cnt, nb, ig, false, d_bias, d_m, st));
    BRUN(hipMemcpyAsync(hm.data(), d_m, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
    BRUN(hipStreamSynchronize(st));
    if (o.min_count > 0.0)
        for (uint64_t k = 0; k < nb; ++k) if (hm[k] < o.min_count) bias[k] = 0.0;
    if (o.mad_max > 0.0) {
        auto median = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); const size_t n = v.size(); return n & 1 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0; };
        std::vector<double> tmp;
        const size_t nc = r.off.size();
        for (size_t i = 0; i < nc; ++i) {
            const uint64_t lo = r.off[i], hi = i + 1 < nc ? r.off[i + 1] : nb;
            tmp.clear();
            for (uint64_t k = lo; k < hi; ++k) if (hm[k] > 0.0) tmp.push_back(hm[k]);
            if (tmp.empty()) continue;
            const double med = median(tmp);
            for (uint64_t k = lo; k < hi; ++k) hm[k] /= med;
        }
        tmp.clear();
        for (uint64_t k = 0; k < nb; ++k) if (hm[k] > 0.0) tmp.push_back(std::log(hm[k]));
        if (!tmp.empty()) {
            const double med = median(tmp);
            for (double& x : tmp) x = std::fabs(x - med);
            const double dev = median(tmp), cut = std::exp(med - o.mad_max * dev);
            for (uint64_t k = 0; k < nb; ++k) if (hm[k] < cut) bias[k] = 0.0;
        }
    }
    uint64_t masked = 0;
    for (uint64_t k = 0; k < nb; ++k) masked += bias[k] == 0.0;
    BRUN(hipMemcpyAsync(d_bias, bias.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));

    // step 4 on the device: a few iterations per look at the state (an iteration behind `done` is a no-op: five empty launches).
    // $MKT_BALANCE_BATCH (1 .. 64) is there to measure other batch sizes (tools/balance_bench.py); the result does not depend on it.
    BalState hs;
    memset(&hs, 0, sizeof hs);
    uint32_t per_look = 4;
    if (const char* e = getenv("MKT_BALANCE_BATCH")) { const int v = atoi(e); if (v >= 1 && v <= 64) per_look = (uint32_t)v; }
    BRUN(mx_timed(m, &r.bal_iter_ms, [&]() -> hipError_t {
        for (uint32_t left = (uint32_t)o.max_iters; left && !hs.done;) {
            const uint32_t batch = left < per_look ? left : per_look;
            MKT_TRY(bal_iterate(r.lay, r.d_b2, r.d_cnt, nb, ig, o.tol, batch, d_bias, d_m, d_part, d_state, st));
            MKT_TRY(hipMemcpyAsync(&hs, d_state, sizeof hs, hipMemcpyDeviceToHost, st));
            MKT_TRY(hipStreamSynchronize(st));
            left -= batch;
        }
        return hipSuccess;
    }));
    BRUN(bal_weights(d_bias, nb, d_state, d_w, st));
    BRUN(hipStreamSynchronize(st));
#undef BRUN
    r.d_w = std::move(d_w);
    r.balanced = true;
    if (stats) {
        stats->iterations = hs.iters; stats->converged = hs.converged ? 1 : 0; stats->var = hs.var; stats->scale = hs.mean;
        stats->masked = hs.empty ? nb : masked;
    }
    return MKT_OK;
}

int mkt_matrix_fetch_weights(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, double* out) {
    if (n && !out) return MKT_E_ARG;
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_WEIGHTS);
    const MxRes& r = *rp;
    if (first > r.nbins || n > r.nbins - first) return mfail(m, MKT_E_ARG, "weights [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)r.nbins);
    MCHK(m, hipSetDevice(m->device));
    if (n) MCHK(m, hipMemcpy(out, r.d_w.get() + first, n * 8, hipMemcpyDeviceToHost));
    return MKT_OK;
}

int mkt_matrix_balance_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* iter_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const MxRes& r = m->res[res_index];
    if (setup_ms) *setup_ms = m->ran && r.balanced ? r.bal_setup_ms : 0.0;
    if (iter_ms) *iter_ms = m->ran && r.balanced ? r.bal_iter_ms : 0.0;
    return MKT_OK;
}

// ---- expected tables and observed / expected values: the entry points; the kernels are mkt_expected.hip, the definition is in include/mkt.h
void mkt_expected_opts_default(mkt_expected_opts* o) {
    if (!o) return;
    o->use_weights = 1; o->reserved = 0;
}

int mkt_matrix_expected(mkt_matrix* m, uint32_t res_index, const mkt_expected_opts* opts, mkt_expected_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_expected_opts o;
    mkt_expected_opts_default(&o);
    if (opts) o = *opts;
    if (o.use_weights != 0 && o.use_weights != 1) return mfail(m, MKT_E_ARG, "expected: use_weights %d (0 or 1)", o.use_weights);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "expected: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | (o.use_weights ? MX_WEIGHTS : 0), "expected")) return rc;
    if (r.nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "expected: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)r.nnz);
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    r.ext = ExpTables();
    r.lps = LoopsState(); r.egs = EigsState();                          // loops and eigenvectors of other tables
    r.pile = PileState();                                               // ... and a pileup of other divisors
    r.sad = SaddleState();                                              // ... and saddle tables of them
    r.exp_sums_ms = r.exp_setup_ms = 0;
#define ERUN(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { r.ext = ExpTables(); return mx_hip(m, "expected: ", e_, true); } } while (0)
    if (!r.exs.built) {                                                 // with the chromosome of a bin when nothing has built it yet
        const hipError_t e = mx_timed(m, &r.exp_setup_ms, [&]() -> hipError_t {
            MKT_TRY(layout_chr(r.lay, mx_cells(r), st));
            return exp_setup(r.exs, r.lay.chr, r.d_b1, r.d_b2, r.d_cnt, r.nnz, r.nbins, r.d_off, r.off, st);
        });
        if (e == hipErrorInvalidValue) return mfail(m, MKT_E_CAPACITY, "expected: segment ids and cell indices of resolution index %u do not fit 64 bits together", res_index);
        ERUN(e);
    }
    ERUN(mx_timed(m, &r.exp_sums_ms, [&] { return exp_sums(r.exs, r.ext, r.lay.chr, r.nbins, r.d_off, o.use_weights ? r.d_w.get() : nullptr, st); }));
    ERUN(exp_finish(r.exs, r.ext, r.nbins, r.off, st));
#undef ERUN
    r.ext.use_weights = o.use_weights;
    if (info) {
        info->cis_rows = r.nbins; info->trans_rows = r.exs.trans_rows; info->genome_rows = r.exs.genome_rows;
        info->n_chrom = (uint32_t)r.off.size(); info->smooth_groups = r.ext.smooth_groups;
    }
    return MKT_OK;
}

}  // extern "C"

// the tables of res_index for a fetch of rows [first, first + n) of table `which` (0 cis, 1 trans, 2 genome), or the error
static int mx_expected_tables(mkt_matrix* m, uint32_t res_index, const char* what, uint64_t first, uint64_t n, int which, const ExpTables** out) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_TABLES);
    const MxRes& r = *rp;
    const uint64_t rows = which == 0 ? r.nbins : which == 1 ? r.exs.trans_rows : r.exs.genome_rows;
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "%s rows [%llu, +%llu) of %llu", what, (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    *out = &r.ext;
    return MKT_OK;
}
template <typename T>
static void mx_copy_rows(T* out, const std::vector<T>& v, uint64_t first, uint64_t n) { if (out && n) memcpy(out, v.data() + first, (size_t)n * sizeof(T)); }

extern "C" {

int mkt_matrix_fetch_expected_cis(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum) {
    const ExpTables* t = nullptr;
    const int rc = mx_expected_tables(m, res_index, "cis", first, n, 0, &t);
    if (rc) return rc;
    mx_copy_rows(n_valid, t->cis_n, first, n); mx_copy_rows(count_sum, t->cis_c, first, n); mx_copy_rows(balanced_sum, t->cis_s, first, n);
    return MKT_OK;
}
int mkt_matrix_fetch_expected_trans(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum, double* expected) {
    const ExpTables* t = nullptr;
    const int rc = mx_expected_tables(m, res_index, "trans", first, n, 1, &t);
    if (rc) return rc;
    mx_copy_rows(n_valid, t->tr_n, first, n); mx_copy_rows(count_sum, t->tr_c, first, n); mx_copy_rows(balanced_sum, t->tr_s, first, n); mx_copy_rows(expected, t->tr_e, first, n);
    return MKT_OK;
}
int mkt_matrix_fetch_expected_genome(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* count_sum, double* balanced_sum, double* expected,
                                     double* expected_smooth) {
    const ExpTables* t = nullptr;
    const int rc = mx_expected_tables(m, res_index, "genome", first, n, 2, &t);
    if (rc) return rc;
    mx_copy_rows(n_valid, t->g_n, first, n); mx_copy_rows(count_sum, t->g_c, first, n); mx_copy_rows(balanced_sum, t->g_s, first, n);
    mx_copy_rows(expected, t->g_e, first, n); mx_copy_rows(expected_smooth, t->g_sm, first, n);
    return MKT_OK;
}

int mkt_matrix_fetch_values(mkt_matrix* m, uint32_t res_index, int kind, uint64_t first, uint64_t n, double* out) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    if (kind != MKT_VALUE_BALANCED && kind != MKT_VALUE_OE && kind != MKT_VALUE_OE_SMOOTH) return mfail(m, MKT_E_ARG, "values: kind %d (0 balanced, 1 oe, 2 oe_smooth)", kind);
    const MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | (kind != MKT_VALUE_BALANCED ? MX_TABLES : 0), "values")) return rc;
    if (!r.ext.built) { if (const int rc = mx_need(m, res_index, r, MX_WEIGHTS)) return rc; }
    if (first > r.nnz || n > r.nnz - first) return mfail(m, MKT_E_ARG, "values of cells [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)r.nnz);
    if (!out || n == 0) return MKT_OK;
    MCHK(m, hipSetDevice(m->device));
    const double* w = r.ext.built && !r.ext.use_weights ? nullptr : r.d_w.get();       // the tables' own option; without tables, the weights
    const uint64_t piece = n < (1ull << 24) ? n : (1ull << 24);
    DevBuf<double> d_out;
    { hipError_t e_ = d_out.alloc(piece); if (e_ != hipSuccess) return mfail(m, MKT_E_NOMEM, "values: hipMalloc of %llu doubles failed: %s", (unsigned long long)piece, hipGetErrorString(e_)); }
    for (uint64_t at = 0; at < n; at += piece) {
        const uint64_t k = n - at < piece ? n - at : piece;
        hipError_t e = exp_values(r.ext.built ? &r.ext : nullptr, r.ext.built ? r.lay.chr.get() : nullptr, r.d_b1, r.d_b2, r.d_cnt, first + at, k, r.d_off, (uint32_t)r.off.size(), w, kind, d_out, m->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out + at, d_out, (size_t)k * 8, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) return mfail(m, MKT_E_HIP, "values: cells [%llu, +%llu) failed: %s", (unsigned long long)(first + at), (unsigned long long)k, hipGetErrorString(e));
    }
    return MKT_OK;
}

int mkt_matrix_expected_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sums_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const MxRes& r = m->res[res_index];
    if (setup_ms) *setup_ms = m->ran && r.ext.built ? r.exp_setup_ms : 0.0;
    if (sums_ms) *sums_ms = m->ran && r.ext.built ? r.exp_sums_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- loop calling: the entry points; the kernels, thresholds and clustering are mkt_loops.hip, the definition is in include/mkt.h
extern "C" {

void mkt_loops_opts_default(mkt_loops_opts* o) {
    if (!o) return;
    o->peak = 2; o->window = 5; o->window_max = 20; o->min_ll_count = 16; o->min_dist = 8; o->max_dist = 0; o->fdr = 0.1; o->cluster_radius = 2; o->reserved = 0;
}

int mkt_matrix_loops(mkt_matrix* m, uint32_t res_index, const mkt_loops_opts* opts, mkt_loops_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_loops_opts o;
    mkt_loops_opts_default(&o);
    if (opts) o = *opts;
    if (o.peak < 0) return mfail(m, MKT_E_ARG, "loops: peak %d is negative", o.peak);
    if (o.window <= o.peak) return mfail(m, MKT_E_ARG, "loops: window %d is not larger than peak %d", o.window, o.peak);
    if (o.window_max < o.window || o.window_max > kLpWmax) return mfail(m, MKT_E_ARG, "loops: window_max %d (window %d .. %d)", o.window_max, o.window, kLpWmax);
    if (o.min_ll_count < 0) return mfail(m, MKT_E_ARG, "loops: min_ll_count %d is negative", o.min_ll_count);
    if (o.min_dist < 0 || o.max_dist < 0) return mfail(m, MKT_E_ARG, "loops: min_dist %d / max_dist %d is negative", o.min_dist, o.max_dist);
    if (!(o.fdr > 0.0 && o.fdr < 1.0)) return mfail(m, MKT_E_ARG, "loops: fdr %g is not inside (0, 1)", o.fdr);
    if (o.cluster_radius < 0) return mfail(m, MKT_E_ARG, "loops: cluster_radius %d is negative", o.cluster_radius);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "loops: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | MX_TABLES, "loops")) return rc;
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    r.lps = LoopsState();
#define LRUN(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { r.lps = LoopsState(); return mx_hip(m, "loops: ", e_, true); } } while (0)
    LRUN(layout_rows(r.lay, mx_cells(r), st));                          // the row pointers are all the pass needs
    LoopsIn in;
    in.b1 = r.d_b1; in.b2 = r.d_b2; in.cnt = r.d_cnt; in.rowptr = r.lay.rowptr; in.off = r.d_off; in.chr = r.lay.chr;
    in.w = r.ext.use_weights ? r.d_w.get() : nullptr; in.E = r.ext.d_cis_sm;
    in.nnz = r.nnz; in.nbins = r.nbins; in.genome_rows = r.exs.genome_rows; in.nchr = (uint32_t)r.off.size();
    LRUN(loops_run(r.lps, in, r.off, o, st));
#undef LRUN
    if (info) *info = r.lps.info;
    return MKT_OK;
}

int mkt_matrix_fetch_loop_cells(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* status, uint8_t* window, uint8_t* chunk, double* r,
                                uint8_t* enriched, uint64_t* csum_ll, uint16_t* kept, double* bsum, double* esum, double* e) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_LOOPS);
    const LoopsState* s = &rp->lps;
    const uint64_t nnz = m->res[res_index].nnz;
    if (first > nnz || n > nnz - first) return mfail(m, MKT_E_ARG, "loop cells [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)nnz);
    MCHK(m, hipSetDevice(m->device));
    if (n == 0) return MKT_OK;
    if (status) MCHK(m, hipMemcpy(status, s->status.get() + first, n, hipMemcpyDeviceToHost));
    if (window) MCHK(m, hipMemcpy(window, s->window.get() + first, n, hipMemcpyDeviceToHost));
    if (chunk) MCHK(m, hipMemcpy(chunk, s->chunk.get() + 4 * first, 4 * n, hipMemcpyDeviceToHost));
    if (r) MCHK(m, hipMemcpy(r, s->r.get() + 4 * first, 32 * n, hipMemcpyDeviceToHost));
    if (enriched) MCHK(m, hipMemcpy(enriched, s->enriched.get() + first, n, hipMemcpyDeviceToHost));
    if (csum_ll) MCHK(m, hipMemcpy(csum_ll, s->csum.get() + first, 8 * n, hipMemcpyDeviceToHost));
    if (kept) MCHK(m, hipMemcpy(kept, s->kept.get() + 4 * first, 8 * n, hipMemcpyDeviceToHost));
    if (bsum) MCHK(m, hipMemcpy(bsum, s->bsum.get() + 4 * first, 32 * n, hipMemcpyDeviceToHost));
    if (esum) MCHK(m, hipMemcpy(esum, s->esum.get() + 4 * first, 32 * n, hipMemcpyDeviceToHost));
    if (e) MCHK(m, hipMemcpy(e, s->e.get() + 4 * first, 32 * n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_matrix_fetch_loop_hist(mkt_matrix* m, uint32_t res_index, uint64_t* hist) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_LOOPS);
    const LoopsState* s = &rp->lps;
    if (hist) memcpy(hist, s->hist.data(), s->hist.size() * 8);
    return MKT_OK;
}
int mkt_matrix_fetch_loop_thresholds(mkt_matrix* m, uint32_t res_index, uint32_t* thresholds) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_LOOPS);
    const LoopsState* s = &rp->lps;
    if (thresholds) memcpy(thresholds, s->thr.data(), s->thr.size() * 4);
    return MKT_OK;
}
int mkt_matrix_fetch_loops(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, mkt_loop* out) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_LOOPS);
    const LoopsState* s = &rp->lps;
    const uint64_t rows = s->loops.size();
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "loops [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    if (out && n) memcpy(out, s->loops.data() + first, (size_t)n * sizeof(mkt_loop));
    return MKT_OK;
}
int mkt_matrix_loops_timing(const mkt_matrix* m, uint32_t res_index, double* pass_ms, double* hist_ms, double* flag_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const LoopsState& s = m->res[res_index].lps;
    const bool have = m->ran && s.built;
    if (pass_ms) *pass_ms = have ? s.pass_ms : 0.0;
    if (hist_ms) *hist_ms = have ? s.hist_ms : 0.0;
    if (flag_ms) *flag_ms = have ? s.flag_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- compartment eigenvectors: the entry points; the kernels and the iteration are mkt_eigs.hip, the definition is in include/mkt.h
extern "C" {

void mkt_eigs_opts_default(mkt_eigs_opts* o) {
    if (!o) return;
    o->n_eigs = 3; o->ignore_diags = 2; o->min_good = 9; o->max_iters = 300; o->tol = 1e-8; o->clip = 0.0; o->reserved = 0;
}

}  // extern "C"

// the options checked, the tables there and the full layout built: what eigs and apply share
static int mx_eigs_ready(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, mkt_eigs_opts& o, EigsIn& in, double* setup_ms) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_eigs_opts_default(&o);
    if (opts) o = *opts;
    if (o.n_eigs < 1 || o.n_eigs > 4) return mfail(m, MKT_E_ARG, "eigs: n_eigs %d (1 .. 4)", o.n_eigs);
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "eigs: ignore_diags %d is negative", o.ignore_diags);
    if (o.min_good < 0) return mfail(m, MKT_E_ARG, "eigs: min_good %d is negative", o.min_good);
    if (o.max_iters < 0) return mfail(m, MKT_E_ARG, "eigs: max_iters %d is negative", o.max_iters);
    if (!(o.tol > 0.0 && o.tol < 1.0)) return mfail(m, MKT_E_ARG, "eigs: tol %g is not inside (0, 1)", o.tol);
    if (!(o.clip >= 0.0)) return mfail(m, MKT_E_ARG, "eigs: clip %g is negative or NaN", o.clip);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "eigs: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | MX_TABLES, "eigs")) return rc;
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    if (setup_ms) *setup_ms = 0;
    if (!r.lay.has_full) {                                              // raw counts: the transposed half without a balance
        MX(m, "eigs: ", mx_timed(m, &r.bal_setup_ms, [&] { return layout_full(r.lay, mx_cells(r), st); }));
        if (setup_ms) *setup_ms = r.bal_setup_ms;
    }
    in.lay = &r.lay; in.b2 = r.d_b2; in.cnt = r.d_cnt; in.off = r.d_off;
    in.w = r.ext.use_weights ? r.d_w.get() : nullptr; in.E = r.ext.d_cis_sm;
    in.nbins = r.nbins; in.nchr = (uint32_t)r.off.size();
    return MKT_OK;
}

extern "C" {

int mkt_matrix_eigs(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, const double* phasing, mkt_eigs_info* info) {
    if (!m) return MKT_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    mkt_eigs_opts o;
    EigsIn in;
    double setup_ms = 0;
    const int rc = mx_eigs_ready(m, res_index, opts, o, in, &setup_ms);
    if (rc) return rc;
    MxRes& r = m->res[res_index];
    const hipError_t e = eigs_run(r.egs, in, r.off, o, phasing, m->stream);
    if (e != hipSuccess) { r.egs = EigsState(); return mfail(m, e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "eigs: %s", hipGetErrorString(e)); }
    r.egs.setup_ms += setup_ms;
    if (info) *info = r.egs.info;
    return MKT_OK;
}

int mkt_matrix_eigs_apply(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, const double* x, uint32_t ncols, double* y) {
    if (!m) return MKT_E_ARG;
    mkt_eigs_opts o;
    EigsIn in;
    const int rc = mx_eigs_ready(m, res_index, opts, o, in, nullptr);
    if (rc) return rc;
    if (ncols < 1 || ncols > (uint32_t)kEgCols) return mfail(m, MKT_E_ARG, "eigs apply: ncols %u (1 .. 8)", ncols);
    if (!x || !y) return mfail(m, MKT_E_ARG, "eigs apply: x and y are needed");
    const hipError_t e = eigs_apply(in, m->res[res_index].off, o, x, ncols, y, m->stream);
    if (e != hipSuccess) return mfail(m, e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "eigs apply: %s", hipGetErrorString(e));
    return MKT_OK;
}

int mkt_matrix_fetch_eigvecs(mkt_matrix* m, uint32_t res_index, uint32_t k, uint64_t first, uint64_t n, double* out) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_EIGS);
    const EigsState* s = &rp->egs;
    const uint64_t nb = m->res[res_index].nbins;
    if (k >= (uint32_t)s->n_eigs) return mfail(m, MKT_E_ARG, "eigenvector %u of %d", k, s->n_eigs);
    if (first > nb || n > nb - first) return mfail(m, MKT_E_ARG, "eigenvector bins [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)nb);
    if (out && n) memcpy(out, s->vec.data() + (size_t)k * nb + first, (size_t)n * 8);
    return MKT_OK;
}

int mkt_matrix_fetch_eigvals(mkt_matrix* m, uint32_t res_index, uint32_t first_chrom, uint32_t n, double* lambda, double* resid, uint32_t* n_good,
                             uint32_t* iterations, uint8_t* converged) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_EIGS);
    const EigsState* s = &rp->egs;
    const uint32_t nchr = (uint32_t)s->n_good.size();
    if (first_chrom > nchr || n > nchr - first_chrom) return mfail(m, MKT_E_ARG, "eigenvalues of chromosomes [%u, +%u) of %u", first_chrom, n, nchr);
    if (n == 0) return MKT_OK;
    const size_t ne = (size_t)s->n_eigs;
    if (lambda) memcpy(lambda, s->lambda.data() + first_chrom * ne, n * ne * 8);
    if (resid) memcpy(resid, s->resid.data() + first_chrom * ne, n * ne * 8);
    if (n_good) memcpy(n_good, s->n_good.data() + first_chrom, (size_t)n * 4);
    if (iterations) memcpy(iterations, s->iterations.data() + first_chrom, (size_t)n * 4);
    if (converged) memcpy(converged, s->converged.data() + first_chrom, n);
    return MKT_OK;
}

int mkt_matrix_eigs_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms, double* small_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const EigsState& s = m->res[res_index].egs;
    const bool have = m->ran && s.built;
    if (setup_ms) *setup_ms = have ? s.setup_ms : 0.0;
    if (sweep_ms) *sweep_ms = have ? s.sweep_ms : 0.0;
    if (small_ms) *small_ms = have ? s.small_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- insulation scores and boundaries: the entry points; the sweep and the calling are mkt_insulation.hip, the definition is in include/mkt.h
extern "C" {

void mkt_insulation_opts_default(mkt_insulation_opts* o) {
    if (!o) return;
    o->n_windows = 3; o->window[0] = 5; o->window[1] = 10; o->window[2] = 25; o->window[3] = 0;
    o->ignore_diags = 2; o->use_weights = 1; o->reserved = 0; o->min_frac_valid = 0.66; o->min_strength = 0.2;
}

int mkt_matrix_insulation(mkt_matrix* m, uint32_t res_index, const mkt_insulation_opts* opts, mkt_insulation_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_insulation_opts o;
    mkt_insulation_opts_default(&o);
    if (opts) o = *opts;
    if (o.n_windows < 1 || o.n_windows > kInsWindows) return mfail(m, MKT_E_ARG, "insulation: n_windows %d (1 .. 4)", o.n_windows);
    for (int k = 0; k < o.n_windows; ++k) {
        if (o.window[k] < 1 || o.window[k] > kInsWmax) return mfail(m, MKT_E_ARG, "insulation: window %d is outside 1 .. %d bins", o.window[k], kInsWmax);
        if (k && o.window[k] <= o.window[k - 1]) return mfail(m, MKT_E_ARG, "insulation: windows %d, %d are not strictly ascending", o.window[k - 1], o.window[k]);
    }
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "insulation: ignore_diags %d is negative", o.ignore_diags);
    if (o.use_weights != 0 && o.use_weights != 1) return mfail(m, MKT_E_ARG, "insulation: use_weights %d (0 or 1)", o.use_weights);
    if (!(o.min_frac_valid >= 0.0 && o.min_frac_valid <= 1.0)) return mfail(m, MKT_E_ARG, "insulation: min_frac_valid %g is not inside [0, 1]", o.min_frac_valid);
    if (!(o.min_strength >= 0.0)) return mfail(m, MKT_E_ARG, "insulation: min_strength %g is negative or NaN", o.min_strength);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "insulation: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | (o.use_weights ? MX_WEIGHTS : 0), "insulation")) return rc;
    if (r.nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "insulation: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)r.nnz);
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    r.ins = InsState();
#define IRUN(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { r.ins = InsState(); return mx_hip(m, "insulation: ", e_, true); } } while (0)
    IRUN(layout_rows(r.lay, mx_cells(r), st));                          // the row pointers and the chromosome of a bin are all the sweep needs
    InsIn in;
    in.b2 = r.d_b2; in.cnt = r.d_cnt; in.rowptr = r.lay.rowptr; in.off = r.d_off; in.chr = r.lay.chr;
    in.w = o.use_weights ? r.d_w.get() : nullptr;
    in.nnz = r.nnz; in.nbins = r.nbins; in.nchr = (uint32_t)r.off.size();
    IRUN(insulation_run(r.ins, in, r.off, o, st));
#undef IRUN
    if (info) *info = r.ins.info;
    return MKT_OK;
}

int mkt_matrix_fetch_insulation(mkt_matrix* m, uint32_t res_index, uint32_t k, uint64_t first, uint64_t n, uint64_t* n_valid, uint64_t* csum, double* bsum,
                                double* score, double* log2_score, double* strength, uint8_t* boundary) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_INS);
    const InsState* s = &rp->ins;
    const uint64_t nb = rp->nbins;
    if (k >= (uint32_t)s->n_windows) return mfail(m, MKT_E_ARG, "insulation window %u of %d", k, s->n_windows);
    if (first > nb || n > nb - first) return mfail(m, MKT_E_ARG, "insulation bins [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)nb);
    const uint64_t at = (uint64_t)k * nb + first;
    mx_copy_rows(n_valid, s->n_valid, at, n); mx_copy_rows(csum, s->csum, at, n); mx_copy_rows(bsum, s->bsum, at, n); mx_copy_rows(score, s->score, at, n);
    mx_copy_rows(log2_score, s->log2_score, at, n); mx_copy_rows(strength, s->strength, at, n); mx_copy_rows(boundary, s->boundary, at, n);
    return MKT_OK;
}

int mkt_matrix_insulation_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const InsState& s = m->res[res_index].ins;
    const bool have = m->ran && s.built;
    if (setup_ms) *setup_ms = have ? s.setup_ms : 0.0;
    if (sweep_ms) *sweep_ms = have ? s.sweep_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- pileups: the entry points; the sweep, the statuses and the scores are mkt_pileup.hip, the definition is in include/mkt.h
extern "C" {

void mkt_pileup_opts_default(mkt_pileup_opts* o) {
    if (!o) return;
    o->flank = 10; o->corner = 6; o->kind = MKT_VALUE_OE_SMOOTH; o->ignore_diags = 2; o->edges = 0; o->min_dist = 0; o->max_dist = 0; o->reserved = 0;
}

int mkt_matrix_pileup(mkt_matrix* m, uint32_t res_index, const uint32_t* bin1, const uint32_t* bin2, uint64_t n, const mkt_pileup_opts* opts, mkt_pileup_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_pileup_opts o;
    mkt_pileup_opts_default(&o);
    if (opts) o = *opts;
    if (o.flank < 1 || o.flank > kPileFlankMax) return mfail(m, MKT_E_ARG, "pileup: flank %d is outside 1 .. %d", o.flank, kPileFlankMax);
    if (o.corner < 1 || o.corner > o.flank) return mfail(m, MKT_E_ARG, "pileup: corner %d is outside 1 .. flank %d", o.corner, o.flank);
    if (o.kind != MKT_VALUE_BALANCED && o.kind != MKT_VALUE_OE && o.kind != MKT_VALUE_OE_SMOOTH) return mfail(m, MKT_E_ARG, "pileup: kind %d (0 balanced, 1 oe, 2 oe_smooth)", o.kind);
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "pileup: ignore_diags %d is negative", o.ignore_diags);
    if (o.edges != 0 && o.edges != 1) return mfail(m, MKT_E_ARG, "pileup: edges %d (0 or 1)", o.edges);
    if (o.min_dist < 0 || o.max_dist < 0) return mfail(m, MKT_E_ARG, "pileup: min_dist %d / max_dist %d is negative", o.min_dist, o.max_dist);
    if (o.max_dist && o.max_dist < o.min_dist) return mfail(m, MKT_E_ARG, "pileup: max_dist %d is below min_dist %d", o.max_dist, o.min_dist);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "pileup: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | MX_TABLES, "pileup")) return rc;
    if (n && (!bin1 || !bin2)) return mfail(m, MKT_E_ARG, "pileup: %llu features without their bins (bin1 or bin2 is NULL)", (unsigned long long)n);
    if (n >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "pileup: %llu features: fewer than 2^32 are needed", (unsigned long long)n);
    if (r.nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "pileup: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)r.nnz);
    PileState ps;                                                       // a refused or failed call leaves the previous results alone
    std::string why;
    if (!pileup_status(bin1, bin2, n, r.off, r.nbins, o, ps.status, why)) return mfail(m, MKT_E_ARG, "%s", why.c_str());
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    MX(m, "pileup: ", layout_rows(r.lay, mx_cells(r), st));             // the row pointers and the chromosome of a bin are all the sweep needs
    PileIn in;
    in.b2 = r.d_b2; in.cnt = r.d_cnt; in.rowptr = r.lay.rowptr; in.off = r.d_off; in.chr = r.lay.chr;
    in.w = r.ext.use_weights ? r.d_w.get() : nullptr;
    in.E = o.kind == MKT_VALUE_OE ? r.ext.d_cis_e.get() : o.kind == MKT_VALUE_OE_SMOOTH ? r.ext.d_cis_sm.get() : nullptr;
    in.nnz = r.nnz; in.nbins = r.nbins; in.nchr = (uint32_t)r.off.size();
    MX(m, "pileup: ", pileup_run(ps, in, bin1, bin2, n, o, st));
    r.pile = std::move(ps);
    if (info) *info = r.pile.info;
    return MKT_OK;
}

int mkt_matrix_fetch_pileup(mkt_matrix* m, uint32_t res_index, uint64_t* n, uint64_t* csum, double* vsum, double* mean) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_PILE);
    const PileState* s = &rp->pile;
    const uint64_t rows = s->n.size();
    mx_copy_rows(n, s->n, 0, rows); mx_copy_rows(csum, s->csum, 0, rows); mx_copy_rows(vsum, s->vsum, 0, rows); mx_copy_rows(mean, s->mean, 0, rows);
    return MKT_OK;
}

int mkt_matrix_fetch_pileup_status(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* status) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_PILE);
    const PileState* s = &rp->pile;
    const uint64_t rows = s->status.size();
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "pileup features [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    mx_copy_rows(status, s->status, first, n);
    return MKT_OK;
}

int mkt_matrix_pileup_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const PileState& s = m->res[res_index].pile;
    const bool have = m->ran && s.built;
    if (setup_ms) *setup_ms = have ? s.setup_ms : 0.0;
    if (sweep_ms) *sweep_ms = have ? s.sweep_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- saddle tables: the entry points; the sweep, the groups, the positions and the scores are mkt_saddle.hip, the definition is in
// include/mkt.h
extern "C" {

void mkt_saddle_opts_default(mkt_saddle_opts* o) {
    if (!o) return;
    o->n_groups = 50; o->trim_lo = 250; o->trim_hi = 250; o->contact = 0; o->kind = MKT_VALUE_OE; o->min_diag = 2; o->max_diag = 0; o->corner = 0; o->reserved = 0;
}

int mkt_matrix_saddle(mkt_matrix* m, uint32_t res_index, const mkt_saddle_opts* opts, const double* track, mkt_saddle_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    mkt_saddle_opts o;
    mkt_saddle_opts_default(&o);
    if (opts) o = *opts;
    if (o.n_groups < 2 || o.n_groups > kSaddleGroupsMax) return mfail(m, MKT_E_ARG, "saddle: n_groups %d is outside 2 .. %d", o.n_groups, kSaddleGroupsMax);
    if (o.trim_lo < 0 || o.trim_hi < 0) return mfail(m, MKT_E_ARG, "saddle: trim_lo %d / trim_hi %d is negative", o.trim_lo, o.trim_hi);
    if ((int64_t)o.trim_lo + o.trim_hi >= 10000) return mfail(m, MKT_E_ARG, "saddle: trim_lo %d + trim_hi %d leaves nothing (basis points: below 10000 together)", o.trim_lo, o.trim_hi);
    if (o.contact != 0 && o.contact != 1) return mfail(m, MKT_E_ARG, "saddle: contact %d (0 cis, 1 trans)", o.contact);
    if (o.kind != MKT_VALUE_OE && o.kind != MKT_VALUE_OE_SMOOTH) return mfail(m, MKT_E_ARG, "saddle: kind %d (1 oe, 2 oe_smooth)", o.kind);
    if (o.min_diag < 0 || o.max_diag < 0) return mfail(m, MKT_E_ARG, "saddle: min_diag %d / max_diag %d is negative", o.min_diag, o.max_diag);
    if (o.max_diag && o.max_diag < o.min_diag) return mfail(m, MKT_E_ARG, "saddle: max_diag %d is below min_diag %d", o.max_diag, o.min_diag);
    if (o.corner < 0 || o.corner > o.n_groups / 2) return mfail(m, MKT_E_ARG, "saddle: corner %d is outside 1 .. n_groups / 2 = %d (0: the default)", o.corner, o.n_groups / 2);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "saddle: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | MX_TABLES, "saddle")) return rc;
    if (!track) return mfail(m, MKT_E_ARG, "saddle: no track (track is NULL)");
    if (r.nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "saddle: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)r.nnz);
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    MX(m, "saddle: ", layout_chr(r.lay, mx_cells(r), st));              // the chromosome of a bin is all the sweep needs of the layout
    SaddleIn in;
    in.b1 = r.d_b1; in.b2 = r.d_b2; in.cnt = r.d_cnt; in.chr = r.lay.chr;
    in.w = r.ext.use_weights ? r.d_w.get() : nullptr;
    in.cis_div = o.kind == MKT_VALUE_OE ? r.ext.d_cis_e.get() : r.ext.d_cis_sm.get(); in.tr_div = r.ext.d_tr_e;
    in.nnz = r.nnz; in.nbins = r.nbins; in.nchr = (uint32_t)r.off.size();
    SaddleState ss;                                                     // a refused or failed call leaves the previous results alone
    MX(m, "saddle: ", saddle_run(ss, in, r.off, track, o, st));
    r.sad = std::move(ss);
    if (info) *info = r.sad.info;
    return MKT_OK;
}

int mkt_matrix_fetch_saddle(mkt_matrix* m, uint32_t res_index, uint64_t* n, uint64_t* nnz, uint64_t* csum, double* vsum, double* mean) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SADDLE);
    const SaddleState* s = &rp->sad;
    const uint64_t rows = s->n.size();
    mx_copy_rows(n, s->n, 0, rows); mx_copy_rows(nnz, s->nnz, 0, rows); mx_copy_rows(csum, s->csum, 0, rows); mx_copy_rows(vsum, s->vsum, 0, rows);
    mx_copy_rows(mean, s->mean, 0, rows);
    return MKT_OK;
}

int mkt_matrix_fetch_saddle_groups(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint8_t* group) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SADDLE);
    const SaddleState* s = &rp->sad;
    const uint64_t rows = s->group.size();
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "saddle groups of bins [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    mx_copy_rows(group, s->group, first, n);
    return MKT_OK;
}

int mkt_matrix_fetch_saddle_edges(mkt_matrix* m, uint32_t res_index, uint64_t* bins, double* lo, double* hi) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SADDLE);
    const SaddleState* s = &rp->sad;
    const uint64_t rows = s->g_bins.size();
    mx_copy_rows(bins, s->g_bins, 0, rows); mx_copy_rows(lo, s->g_lo, 0, rows); mx_copy_rows(hi, s->g_hi, 0, rows);
    return MKT_OK;
}

int mkt_matrix_fetch_saddle_profile(mkt_matrix* m, uint32_t res_index, double* strength, double* aa_ab, double* bb_ab) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SADDLE);
    const SaddleState* s = &rp->sad;
    const uint64_t rows = s->strength.size();
    mx_copy_rows(strength, s->strength, 0, rows); mx_copy_rows(aa_ab, s->aa_ab, 0, rows); mx_copy_rows(bb_ab, s->bb_ab, 0, rows);
    return MKT_OK;
}

int mkt_matrix_saddle_timing(const mkt_matrix* m, uint32_t res_index, double* setup_ms, double* sweep_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const SaddleState& s = m->res[res_index].sad;
    const bool have = m->ran && s.built;
    if (setup_ms) *setup_ms = have ? s.setup_ms : 0.0;
    if (sweep_ms) *sweep_ms = have ? s.sweep_ms : 0.0;
    return MKT_OK;
}

}  // extern "C"

// ---- replicate comparison (SCC): the entry points; the bands, the sweep and the scores are mkt_scc.hip, the definition is in
// include/mkt.h
extern "C" {

void mkt_scc_opts_default(mkt_scc_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->h = 5; o->weighting = MKT_SCC_WEIGHT_N; o->min_n = 3;
}

int mkt_matrix_scc(mkt_matrix* a, uint32_t res_a, mkt_matrix* b, uint32_t res_b, const mkt_scc_opts* opts, mkt_scc_info* info) {
    mkt_matrix* m = a;
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_a, &rp);
    if (!b) return mfail(m, MKT_E_ARG, "scc: no second matrix (b is NULL)");
    if (res_b >= b->res.size()) return mfail(m, MKT_E_ARG, "scc: resolution index %u of %zu in the second matrix", res_b, b->res.size());
    MxRes& ra = *rp;
    MxRes& rb = b->res[res_b];
    if (ra.r != rb.r) return mfail(m, MKT_E_ARG, "scc: resolution %u against resolution %u", ra.r, rb.r);
    if (a->names != b->names || a->lens != b->lens) return mfail(m, MKT_E_ARG, "scc: the chromosome tables of the two matrices differ");
    if (a->device != b->device) return mfail(m, MKT_E_ARG, "scc: the matrices live on devices %d and %d", a->device, b->device);
    mkt_scc_opts o;
    mkt_scc_opts_default(&o);
    if (opts) o = *opts;
    if (o.h < 0 || o.h > kSccHMax) return mfail(m, MKT_E_ARG, "scc: h %d is outside 0 .. %d", o.h, kSccHMax);
    if (o.min_diag < 0 || o.max_diag < 0) return mfail(m, MKT_E_ARG, "scc: min_diag %d / max_diag %d is negative", o.min_diag, o.max_diag);
    if (o.use_weights != 0 && o.use_weights != 1) return mfail(m, MKT_E_ARG, "scc: use_weights %d (0 or 1)", o.use_weights);
    if (o.weighting != MKT_SCC_WEIGHT_N && o.weighting != MKT_SCC_WEIGHT_VAR) return mfail(m, MKT_E_ARG, "scc: weighting %d (0 n, 1 var)", o.weighting);
    if (o.min_n < 2) return mfail(m, MKT_E_ARG, "scc: min_n %d is below 2", o.min_n);
    if (o.slab_rows < 0 || o.slab_rows % (int32_t)kSccChunk != 0) return mfail(m, MKT_E_ARG, "scc: slab_rows %d is not 0 or a positive multiple of %u", o.slab_rows, kSccChunk);
    if (o.reserved[0] != 0 || o.reserved[1] != 0 || o.reserved[2] != 0) return mfail(m, MKT_E_ARG, "scc: a reserved word is not 0");
    if (o.max_diag == 0) {                                              // every diagonal of the longest chromosome
        uint64_t longest = 1;
        for (size_t c = 0; c < ra.off.size(); ++c) longest = std::max<uint64_t>(longest, (c + 1 < ra.off.size() ? ra.off[c + 1] : ra.nbins) - ra.off[c]);
        o.max_diag = (int32_t)std::min<uint64_t>(longest - 1, 0x7FFFFF00u);
    }
    if (o.max_diag < o.min_diag) return mfail(m, MKT_E_ARG, "scc: max_diag %d is below min_diag %d", o.max_diag, o.min_diag);
    if (!a->ran || !b->ran) return mfail(m, MKT_E_STATE, "scc before run%s", a->ran ? " of the second matrix" : "");
    if (o.use_weights && !ra.balanced) return mfail(m, MKT_E_STATE, "no weights for resolution index %u: balance first", res_a);
    if (o.use_weights && !rb.balanced) return mfail(m, MKT_E_STATE, "no weights for resolution index %u of the second matrix: balance first", res_b);
    if (ra.nnz >= (1ull << 32) || rb.nnz >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "scc: %llu and %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)ra.nnz, (unsigned long long)rb.nnz);
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    MX(m, "scc: ", layout_rows(ra.lay, mx_cells(ra), st));              // the row pointers find a slab's cells
    if (b != a || res_b != res_a) {
        MX(m, "scc: ", layout_rows(rb.lay, mx_cells(rb), b->stream));
        MX(m, "scc: ", hipStreamSynchronize(b->stream));                // b's buffers are read on a's stream from here on
    }
    SccSide sa, sb;
    sa.b1 = ra.d_b1; sa.b2 = ra.d_b2; sa.cnt = ra.d_cnt; sa.rowptr = ra.lay.rowptr; sa.w = o.use_weights ? ra.d_w.get() : nullptr; sa.nnz = ra.nnz;
    sb.b1 = rb.d_b1; sb.b2 = rb.d_b2; sb.cnt = rb.d_cnt; sb.rowptr = rb.lay.rowptr; sb.w = o.use_weights ? rb.d_w.get() : nullptr; sb.nnz = rb.nnz;
    SccState ss;                                                        // a refused or failed call leaves the previous results alone
    std::string why;
    const hipError_t e = scc_run(ss, sa, sb, ra.off, ra.nbins, o, st, &why);
    if (e == hipErrorOutOfMemory && !why.empty()) return mfail(m, MKT_E_NOMEM, "scc: %s", why.c_str());
    if (e != hipSuccess) return mx_hip(m, "scc: ", e, true);
    ra.scc = std::move(ss);
    if (info) *info = ra.scc.info;
    return MKT_OK;
}

int mkt_matrix_fetch_scc_strata(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, uint64_t* n_cand, uint64_t* n_used, double* sx, double* sy, double* sxx,
                                double* syy, double* sxy, double* rho, double* w) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SCC);
    const SccState* s = &rp->scc;
    const uint64_t rows = s->n.size();
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "scc strata [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    mx_copy_rows(n_cand, s->n_cand, first, n); mx_copy_rows(n_used, s->n, first, n); mx_copy_rows(sx, s->sx, first, n); mx_copy_rows(sy, s->sy, first, n);
    mx_copy_rows(sxx, s->sxx, first, n); mx_copy_rows(syy, s->syy, first, n); mx_copy_rows(sxy, s->sxy, first, n); mx_copy_rows(rho, s->rho, first, n); mx_copy_rows(w, s->w, first, n);
    return MKT_OK;
}

int mkt_matrix_fetch_scc_chrom(mkt_matrix* m, uint32_t res_index, uint64_t first, uint64_t n, double* scc, double* num, double* den, uint64_t* n_scored) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_SCC);
    const SccState* s = &rp->scc;
    const uint64_t rows = s->c_scc.size();
    if (first > rows || n > rows - first) return mfail(m, MKT_E_ARG, "scc chromosomes [%llu, +%llu) of %llu", (unsigned long long)first, (unsigned long long)n, (unsigned long long)rows);
    mx_copy_rows(scc, s->c_scc, first, n); mx_copy_rows(num, s->c_num, first, n); mx_copy_rows(den, s->c_den, first, n); mx_copy_rows(n_scored, s->c_scored, first, n);
    return MKT_OK;
}

int mkt_matrix_scc_timing(const mkt_matrix* m, uint32_t res_index, double* fill_ms, double* sweep_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const SccState& s = m->res[res_index].scc;
    const bool have = m->ran && s.built;
    if (fill_ms) *fill_ms = have ? s.fill_ms : 0.0;
    if (sweep_ms) *sweep_ms = have ? s.sweep_ms : 0.0;
    return MKT_OK;
}

// ---- viewpoint contact profiles: the entry points; the scans are mkt_viewpoint.hip, the host half mkt_viewpoint.h, the definition is
// in include/mkt.h -------------------------------------------------------------------------------------------------------------------
void mkt_viewpoint_opts_default(mkt_viewpoint_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->vbin = 200; o->pbin = 1000000; o->min_count = 1; o->hotspot_ratio = 0.01;
}

int mkt_matrix_viewpoint(mkt_matrix* m, const mkt_viewpoint_opts* opts, mkt_viewpoint_info* info) {
    if (!m) return MKT_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    mkt_viewpoint_opts o;
    mkt_viewpoint_opts_default(&o);
    if (opts) o = *opts;
    const uint32_t nc = (uint32_t)m->names.size();
    if (o.viewpoint >= nc) return mfail(m, MKT_E_ARG, "viewpoint: chromosome index %u of %u", o.viewpoint, nc);
    if (o.partner_mask && o.partner_mask[o.viewpoint]) return mfail(m, MKT_E_ARG, "viewpoint: %s is in its own partner mask", m->names[o.viewpoint].c_str());
    if (o.vbin == 0 || o.pbin == 0) return mfail(m, MKT_E_ARG, "viewpoint: a bin size of 0 (vbin %u, pbin %u)", o.vbin, o.pbin);
    if (o.origin != 0 && o.origin != 1) return mfail(m, MKT_E_ARG, "viewpoint: origin %d (0 or 1)", o.origin);
    if (o.second_side_only != 0 && o.second_side_only != 1) return mfail(m, MKT_E_ARG, "viewpoint: second_side_only %d (0 or 1)", o.second_side_only);
    if (o.min_count == 0) return mfail(m, MKT_E_ARG, "viewpoint: min_count 0 (at least 1 is needed)");
    if (!(o.hotspot_ratio >= 0.0 && o.hotspot_ratio < 1.0)) return mfail(m, MKT_E_ARG, "viewpoint: hotspot_ratio %g is outside [0, 1)", o.hotspot_ratio);
    if (o.reserved[0] != 0 || o.reserved[1] != 0) return mfail(m, MKT_E_ARG, "viewpoint: a reserved word is not 0");
    if (!m->ran) return mfail(m, MKT_E_STATE, "viewpoint before run");
    std::vector<uint8_t> role(nc, 0);
    for (uint32_t c = 0; c < nc; ++c) role[c] = c == o.viewpoint ? 1 : (!o.partner_mask || o.partner_mask[c]) ? 2 : 0;
    MCHK(m, hipSetDevice(m->device));
    VpState vs;                                                         // a refused or failed call leaves the previous results alone
    std::string why;
    const int rc = vp_run(vs, reinterpret_cast<const uint4*>(m->d_rec.get()), m->n, m->names, m->lens, role, o, m->stream, &why);
    if (rc != MKT_OK) return mfail(m, rc, "viewpoint: %s", why.c_str());
    m->vp = std::move(vs);
    if (info) *info = m->vp.info;
    return MKT_OK;
}

static int vp_have(mkt_matrix* m) {
    if (!m) return MKT_E_ARG;
    if (!(m->ran && m->vp.built)) return mfail(m, MKT_E_STATE, "no viewpoint profile: viewpoint first");
    return MKT_OK;
}
int mkt_matrix_fetch_viewpoint_links(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* vbin, uint32_t* chrom, uint32_t* pbin, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<VpLink>& v = m->vp.links;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint links [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    for (uint64_t k = 0; k < n; ++k) {
        const VpLink& l = v[first + k];
        if (vbin) vbin[k] = l.vbin;
        if (chrom) chrom[k] = l.chrom;
        if (pbin) pbin[k] = l.pbin;
        if (count) count[k] = l.count;
    }
    return MKT_OK;
}
int mkt_matrix_fetch_viewpoint_track(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<uint32_t>& v = m->vp.track;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint track bins [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    if (count && n) memcpy(count, v.data() + first, n * 4);
    return MKT_OK;
}
int mkt_matrix_fetch_viewpoint_partners(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* chrom, uint32_t* pbin, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<VpCell>& v = m->vp.partners;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint partner cells [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    for (uint64_t k = 0; k < n; ++k) {
        const VpCell& c = v[first + k];
        if (chrom) chrom[k] = c.chrom;
        if (pbin) pbin[k] = c.pbin;
        if (count) count[k] = c.count;
    }
    return MKT_OK;
}
int mkt_matrix_viewpoint_timing(const mkt_matrix* m, double* scan_ms, double* sort_ms) {
    if (!m) return MKT_E_ARG;
    const bool have = m->ran && m->vp.built;
    if (scan_ms) *scan_ms = have ? m->vp.scan_ms : 0.0;
    if (sort_ms) *sort_ms = have ? m->vp.sort_ms : 0.0;
    return MKT_OK;
}

// ---- the .hic container: the entry points; the device side and the file layout are mkt_hic.hip, the definition is in include/mkt.h --------
void mkt_hic_opts_default(mkt_hic_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->block_bins = 1000; o->level = 2; o->norm = 1;
}

int mkt_matrix_hic(mkt_matrix* m, const mkt_hic_opts* opts, mkt_hic_info* info) {
    if (!m) return MKT_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    mkt_hic_opts o;
    mkt_hic_opts_default(&o);
    if (opts) o = *opts;
    if (o.block_bins < 1 || o.block_bins > kHicBlockBinsMax) return mfail(m, MKT_E_ARG, "hic: block_bins %u (1 .. %u: block coordinates are int16)", o.block_bins, kHicBlockBinsMax);
    if (o.level < 0 || o.level > 2) return mfail(m, MKT_E_ARG, "hic: level %d (0 stored, 1 fixed codes, 2 dynamic codes)", o.level);
    if (o.norm != 0 && o.norm != 1) return mfail(m, MKT_E_ARG, "hic: norm %d (0 or 1)", o.norm);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "hic: the reserved field is not 0");
    if (o.norm_label && !*o.norm_label) return mfail(m, MKT_E_ARG, "hic: an empty norm_label");
    if (!m->ran) return mfail(m, MKT_E_STATE, "hic before run");
    MCHK(m, hipSetDevice(m->device));
    std::vector<HicResIn> in(m->res.size());
    for (size_t k = 0; k < m->res.size(); ++k) {
        MxRes& r = m->res[k];
        if (r.nnz) MX(m, "hic: ", layout_chr(r.lay, mx_cells(r), m->stream));
        in[k].cells = mx_cells(r);
        in[k].chr = r.nnz ? r.lay.chr.get() : nullptr;
        in[k].off = &r.off;
        in[k].bin_size = r.r;
        in[k].d_w = r.balanced ? r.d_w.get() : nullptr;
    }
    HicState hs;                                                        // a refused or failed call leaves the previous file alone
    std::string why;
    const int rc = hic_build(hs, in, m->names, m->lens, o, m->stream, &why);
    if (rc != MKT_OK) return mfail(m, rc, "%s", why.c_str());
    m->hic = std::move(hs);
    if (info) *info = m->hic.info;
    return MKT_OK;
}

int mkt_matrix_fetch_hic(mkt_matrix* m, uint64_t off, char* out, size_t n) {
    if (!m || (n && !out)) return MKT_E_ARG;
    if (!(m->ran && m->hic.built)) return mfail(m, MKT_E_STATE, "no .hic file: hic first");
    const uint64_t fb = m->hic.info.file_bytes;
    if (off > fb || n > fb - off) return mfail(m, MKT_E_ARG, "range past the end of the .hic file");
    MCHK(m, hipSetDevice(m->device));
    if (n) MCHK(m, hipMemcpy(out, m->hic.image.get() + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

int mkt_matrix_hic_timing(const mkt_matrix* m, uint32_t res_index, double* sort_ms, double* serialise_ms, double* deflate_ms, double* pack_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const bool have = m->ran && m->hic.built && res_index < m->hic.timing.size();
    const HicTiming t = have ? m->hic.timing[res_index] : HicTiming();
    if (sort_ms) *sort_ms = t.sort_ms;
    if (serialise_ms) *serialise_ms = t.serialise_ms;
    if (deflate_ms) *deflate_ms = t.deflate_ms;
    if (pack_ms) *pack_ms = t.pack_ms;
    return MKT_OK;
}

}  // extern "C"
