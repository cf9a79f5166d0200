// mkt_expected.hip -- expected-contact tables and observed / expected values of one resolution's binned contact matrix on the GPU;
// include/mkt.h has the definition; the entry points (mkt_matrix_expected, mkt_matrix_fetch_*) are at the end (mkt_matrix_obj.h).
//
// A cell belongs to one SEGMENT: a cis cell of chromosome c on diagonal d to segment off_c + d (the row of the cis table), a trans
// cell to segment nbins + its row of the trans table.  Once per resolution the cells are grouped by segment (KeyGroup, mkt_layout.h,
// over segment << Bc | cell index, Bc = bits of the cell count) into a copy of (bin1, bin2, count).  The sums then read 12 bytes per
// cell in order and gather w[] (nbins doubles, meant to stay in cache).
//
// Nothing depends on the order anything ran in: a segment's sum is formed by ExpSetup::width lanes walking it with a
// fixed stride, and the lane tree.  A segment of more than kExpLong cells is cut into chunks of kExpChunk cells: one workgroup and
// the workgroup tree per chunk, then one workgroup per segment over its chunks' partial sums in chunk order.  count_sum rides along
// as a uint64 (exact in any order).
// n_valid of (chromosome, diagonal) is a popcount over the chromosome's validity bits: M & (M >> d), word by word.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

namespace mkt {

constexpr int EXWG = 256;
typedef unsigned long long ex_u64;

__device__ inline uint64_t ex_trans_row(uint32_t a, uint32_t b, uint32_t nchr) { return (uint64_t)a * (2ull * nchr - a - 1ull) / 2ull + (b - a - 1u); }
__device__ inline uint64_t ex_seg(uint32_t b1, uint32_t b2, const uint16_t* chr, const uint32_t* off, uint32_t nchr, uint64_t nbins) {
    const uint32_t a = chr[b1], b = chr[b2];                             // bin1 <= bin2, so a <= b
    return a == b ? (uint64_t)off[a] + (b2 - b1) : nbins + ex_trans_row(a, b, nchr);
}
__global__ __launch_bounds__(EXWG) void k_ex_keys(const uint32_t* b1, const uint32_t* b2, uint32_t nnz, const uint16_t* chr, const uint32_t* off, uint32_t nchr, uint64_t nbins,
                                                  int Bc, uint64_t* key) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nnz) key[s] = (ex_seg(b1[s], b2[s], chr, off, nchr, nbins) << Bc) | s;
}
__global__ __launch_bounds__(EXWG) void k_ex_gather(const uint64_t* key, int Bc, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint32_t nnz,
                                                    uint32_t* sb1, uint32_t* sb2, uint32_t* scnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nnz) return;
    const uint32_t s = (uint32_t)(key[j] & ((1ull << Bc) - 1ull));
    sb1[j] = b1[s]; sb2[j] = b2[s]; scnt[j] = cnt[s];
}

// ---- validity bits, word-aligned per chromosome, and n_valid of every (chromosome, diagonal) --------------------------------
__global__ __launch_bounds__(EXWG) void k_ex_mask(const double* w, uint64_t nbins, const uint16_t* chr, const uint32_t* off, const uint64_t* moff, ex_u64* mask) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nbins) return;
    if (w) { const double x = w[k]; if (x != x) return; }
    const uint32_t c = chr[k], i = (uint32_t)k - off[c];
    atomicOr(&mask[moff[c] + (i >> 6)], 1ull << (i & 63u));            // an integer OR: the same word in any order
}
__global__ __launch_bounds__(EXWG) void k_ex_nvalid(const ex_u64* mask, uint64_t nbins, const uint16_t* chr, const uint32_t* off, const uint64_t* moff, ex_u64* nvalid) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nbins) return;
    const uint32_t c = chr[k], d = (uint32_t)k - off[c];
    const ex_u64* M = mask + moff[c];
    const uint32_t words = (uint32_t)(moff[c + 1] - moff[c]), q = d >> 6, r = d & 63u;
    ex_u64 acc = 0, lo = M[q];                                           // d < n_c, so q < words; bits past n_c are 0: i < n_c - d needs no test
    for (uint32_t j = 0; j + q < words; ++j) {
        const ex_u64 hi = j + q + 1u < words ? M[j + q + 1u] : 0ull;
        const ex_u64 sh = r ? (lo >> r) | (hi << (64u - r)) : lo;      // bits [64 j + d, 64 j + d + 64) of M
        acc += (ex_u64)__popcll(M[j] & sh);
        lo = hi;
    }
    nvalid[k] = acc;
}

// ---- the sums ---------------------------------------------------------------------------------------------------------------
// lane `l` of `W` walks elements p0 + l, p0 + l + W, ... of the grouped copy
template <bool UNIT>
__device__ inline void ex_walk(uint32_t l, uint32_t W, uint32_t p0, uint32_t p1, const uint32_t* sb1, const uint32_t* sb2, const uint32_t* scnt, const double* w, double& s, ex_u64& c) {
    for (uint32_t j = p0 + l; j < p1; j += W) {
        const uint32_t n = scnt[j];
        if (UNIT) { s = __dadd_rn(s, (double)n); c += n; }
        else {
            const double wa = w[sb1[j]], wb = w[sb2[j]];
            if (wa == wa && wb == wb) { s = __dadd_rn(s, __dmul_rn(__dmul_rn((double)n, wa), wb)); c += n; }    // v is rounded before it is added: no fused multiply-add
        }
    }
}
// W lanes per segment (W = 8 .. 64, a power of two)
template <bool UNIT, int W>
__global__ __launch_bounds__(EXWG) void k_ex_sums(const uint32_t* segptr, const uint32_t* sb1, const uint32_t* sb2, const uint32_t* scnt, uint64_t nseg, const double* w, double* S, ex_u64* C) {
    const uint64_t g = ((uint64_t)blockIdx.x * EXWG + threadIdx.x) / W;
    const uint32_t l = threadIdx.x & (W - 1);
    double s = 0.0;
    ex_u64 c = 0;
    bool mine = false;
    if (g < nseg) {
        const uint32_t p0 = segptr[g], p1 = segptr[g + 1];
        mine = p1 - p0 <= kExpLong;
        if (mine) ex_walk<UNIT>(l, W, p0, p1, sb1, sb2, scnt, w, s, c);
    }
    lane_tree_v<W>(AddRn(), s, c);
    if (mine && l == 0) { S[g] = s; C[g] = c; }
}
// one workgroup per chunk of a long segment: the same walk with 256 lanes
template <bool UNIT>
__global__ __launch_bounds__(EXWG) void k_ex_chunk(const uint2* ltask, const uint32_t* sb1, const uint32_t* sb2, const uint32_t* scnt, const double* w, double* ps, ex_u64* pc) {
    __shared__ double shs[EXWG / 64];
    __shared__ ex_u64 shc[EXWG / 64];
    const uint2 t = ltask[blockIdx.x];
    double s = 0.0;
    ex_u64 c = 0;
    ex_walk<UNIT>(threadIdx.x, EXWG, t.x, t.y, sb1, sb2, scnt, w, s, c);
    wg_tree2(AddRn(), s, shs, c, shc);
    if (threadIdx.x == 0) { ps[blockIdx.x] = s; pc[blockIdx.x] = c; }
}
// one workgroup per long segment: its chunks' partial sums, lane l taking chunks l, l + 256, ..., the same tree
__global__ __launch_bounds__(EXWG) void k_ex_long(const uint64_t* lseg, const double* ps, const ex_u64* pc, double* S, ex_u64* C) {
    __shared__ double shs[EXWG / 64];
    __shared__ ex_u64 shc[EXWG / 64];
    const uint64_t g = lseg[3 * (uint64_t)blockIdx.x], t0 = lseg[3 * (uint64_t)blockIdx.x + 1], nt = lseg[3 * (uint64_t)blockIdx.x + 2];
    double s = 0.0;
    ex_u64 c = 0;
    for (uint64_t t = threadIdx.x; t < nt; t += EXWG) { s = __dadd_rn(s, ps[t0 + t]); c += pc[t0 + t]; }
    wg_tree2(AddRn(), s, shs, c, shc);
    if (threadIdx.x == 0) { S[g] = s; C[g] = c; }
}

// ---- per-cell values, in cell order -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EXWG) void k_ex_values(const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t first, uint64_t n, const double* w, int kind,
                                                    const uint16_t* chr, const uint32_t* off, uint32_t nchr, const double* cis_div, const double* tr_div, double* out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = b1[first + i], y = b2[first + i];
    const double wa = w ? w[x] : 1.0, wb = w ? w[y] : 1.0;
    double v = dev_nan();                                                // a cell with a masked bin
    if (wa == wa && wb == wb) {
        v = __dmul_rn(__dmul_rn((double)cnt[first + i], wa), wb);
        if (kind != 0) {
            const uint32_t a = chr[x], b = chr[y];
            v = v / (a == b ? cis_div[y - x] : tr_div[ex_trans_row(a, b, nchr)]);
        }
    }
    out[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------
static hipError_t ex_setup(ExpSetup& s, const uint16_t* chr, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t nnz, uint64_t nbins, const uint32_t* d_off,
                     const std::vector<uint32_t>& off, hipStream_t st) {
    s = ExpSetup();
    const uint32_t nchr = (uint32_t)off.size();
    if (nnz >= (1ull << 32) || nbins >= (1ull << 32) || nchr == 0 || nchr > 8192u) return hipErrorInvalidValue;
    s.trans_rows = (uint64_t)nchr * (nchr - 1ull) / 2ull;
    s.nseg = nbins + s.trans_rows;
    int Bc = 0, Bs = 0;
    while ((1ull << Bc) < nnz) ++Bc;                                     // a cell index fits Bc bits, a segment id Bs
    while ((1ull << Bs) < s.nseg) ++Bs;
    if (Bc + Bs > 64) return hipErrorInvalidValue;
    std::vector<uint64_t> moff(nchr + 1, 0);
    for (uint32_t c = 0; c < nchr; ++c) {
        const uint64_t n_c = (c + 1 < nchr ? off[c + 1] : nbins) - off[c];
        moff[c + 1] = moff[c] + (n_c + 63) / 64;
        if (n_c > s.genome_rows) s.genome_rows = n_c;
    }
    s.mwords = moff[nchr];
    KeyGroup kg;                                                         // its scratch goes behind the synchronise below
    const size_t pbytes = (size_t)(s.nseg + 1) * 4;
    MKT_TRY(s.moff.alloc(nchr + 1));
    MKT_TRY(s.sb1.alloc(nnz, 64));
    MKT_TRY(s.sb2.alloc(nnz, 64));
    MKT_TRY(s.scnt.alloc(nnz, 64));
    MKT_TRY(s.segptr.alloc(s.nseg + 1));
    MKT_TRY(hipMemcpyAsync(s.moff, moff.data(), (size_t)(nchr + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz == 0) MKT_TRY(hipMemsetAsync(s.segptr, 0, pbytes, st));
    else {
        MKT_TRY(kg.alloc(nnz));
        hipLaunchKernelGGL(k_ex_keys, dim3(grid_for(nnz, EXWG)), dim3(EXWG), 0, st, b1, b2, (uint32_t)nnz, chr, d_off, nchr, nbins, Bc, kg.keys());
        MKT_TRY(kg.group(nnz, Bc, Bs, Bc, s.nseg + 1, s.segptr, st));         // stable: (segment, cell index) order
        hipLaunchKernelGGL(k_ex_gather, dim3(grid_for(nnz, EXWG)), dim3(EXWG), 0, st, (const uint64_t*)kg.keys(), Bc, b1, b2, cnt, (uint32_t)nnz, s.sb1.get(), s.sb2.get(), s.scnt.get());
    }
    MKT_TRY(hipGetLastError());
    // the long segments and their chunks, from the pointers (once per resolution)
    std::vector<uint32_t> sp(s.nseg + 1);
    MKT_TRY(hipMemcpyAsync(sp.data(), s.segptr, pbytes, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    std::vector<uint2> tasks;
    std::vector<uint64_t> ls;
    for (uint64_t g = 0; g < s.nseg; ++g) {
        const uint32_t p0 = sp[g], p1 = sp[g + 1];
        if (p1 - p0 <= kExpLong) continue;
        ls.push_back(g); ls.push_back(tasks.size()); ls.push_back(((uint64_t)(p1 - p0) + kExpChunk - 1) / kExpChunk);
        for (uint64_t p = p0; p < p1; p += kExpChunk) tasks.push_back(make_uint2((uint32_t)p, (uint32_t)(p + kExpChunk < p1 ? p + kExpChunk : p1)));
    }
    s.nlong = (uint32_t)(ls.size() / 3);
    s.ntask = (uint32_t)tasks.size();
    if (s.nlong) {
        MKT_TRY(s.ltask.alloc(tasks.size()));
        MKT_TRY(s.lseg.alloc(ls.size()));
        MKT_TRY(hipMemcpy(s.ltask, tasks.data(), tasks.size() * sizeof(uint2), hipMemcpyHostToDevice));
        MKT_TRY(hipMemcpy(s.lseg, ls.data(), ls.size() * 8, hipMemcpyHostToDevice));
    }
    s.width = seg_width(s.nseg ? nnz / s.nseg : 0);                      // cells a segment holds on average
    s.built = true;
    return hipSuccess;
}

hipError_t exp_setup(ExpSetup& s, const uint16_t* chr, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t nnz, uint64_t nbins, const uint32_t* d_off,
                     const std::vector<uint32_t>& off, hipStream_t st) {
    const hipError_t e = ex_setup(s, chr, b1, b2, cnt, nnz, nbins, d_off, off, st);
    if (e != hipSuccess) s = ExpSetup();                                 // nothing half built stays behind
    return e;
}

template <bool UNIT>
static hipError_t ex_launch_sums(const ExpSetup& s, ExpTables& t, const double* w, hipStream_t st) {
    if (s.nseg == 0) return hipSuccess;
    ex_u64* C = (ex_u64*)t.d_c.get();
    dispatch_width(s.width, [&](auto W) {
        hipLaunchKernelGGL((k_ex_sums<UNIT, decltype(W)::value>), dim3(grid_for(s.nseg * (uint64_t)s.width, EXWG)), dim3(EXWG), 0, st, (const uint32_t*)s.segptr,
                           (const uint32_t*)s.sb1, (const uint32_t*)s.sb2, (const uint32_t*)s.scnt, s.nseg, w, t.d_s.get(), C);
    });
    if (s.nlong) {
        ex_u64* pc = (ex_u64*)(t.d_part.get() + s.ntask);
        hipLaunchKernelGGL((k_ex_chunk<UNIT>), dim3(s.ntask), dim3(EXWG), 0, st, (const uint2*)s.ltask, (const uint32_t*)s.sb1, (const uint32_t*)s.sb2, (const uint32_t*)s.scnt, w, t.d_part.get(), pc);
        hipLaunchKernelGGL(k_ex_long, dim3(s.nlong), dim3(EXWG), 0, st, (const uint64_t*)s.lseg, (const double*)t.d_part, (const ex_u64*)pc, t.d_s.get(), C);
    }
    return hipGetLastError();
}

hipError_t exp_sums(const ExpSetup& s, ExpTables& t, const uint16_t* chr, uint64_t nbins, const uint32_t* d_off, const double* w, hipStream_t st) {
    t = ExpTables();
    MKT_TRY(t.d_n.alloc(nbins, 64));
    MKT_TRY(t.d_c.alloc(s.nseg, 64));
    MKT_TRY(t.d_s.alloc(s.nseg, 64));
    MKT_TRY(t.d_mask.alloc(s.mwords, 64));
    MKT_TRY(t.d_part.alloc(2 * (size_t)s.ntask, 64));
    MKT_TRY(hipMemsetAsync(t.d_mask, 0, (size_t)s.mwords * 8 + 64, st));
    if (nbins) {
        const unsigned bgrid = grid_for(nbins, EXWG);
        hipLaunchKernelGGL(k_ex_mask, dim3(bgrid), dim3(EXWG), 0, st, w, nbins, chr, d_off, (const uint64_t*)s.moff, (ex_u64*)t.d_mask.get());
        hipLaunchKernelGGL(k_ex_nvalid, dim3(bgrid), dim3(EXWG), 0, st, (const ex_u64*)t.d_mask.get(), nbins, chr, d_off, (const uint64_t*)s.moff, (ex_u64*)t.d_n.get());
    }
    return w ? ex_launch_sums<false>(s, t, w, st) : ex_launch_sums<true>(s, t, w, st);
}

hipError_t exp_finish(const ExpSetup& s, ExpTables& t, uint64_t nbins, const std::vector<uint32_t>& off, hipStream_t st) {
    const uint32_t nchr = (uint32_t)off.size();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<uint64_t> c(s.nseg);
    std::vector<double> sm(s.nseg);
    t.cis_n.assign(nbins, 0);
    if (nbins) MKT_TRY(hipMemcpyAsync(t.cis_n.data(), t.d_n, (size_t)nbins * 8, hipMemcpyDeviceToHost, st));
    if (s.nseg) MKT_TRY(hipMemcpyAsync(c.data(), t.d_c, (size_t)s.nseg * 8, hipMemcpyDeviceToHost, st));
    if (s.nseg) MKT_TRY(hipMemcpyAsync(sm.data(), t.d_s, (size_t)s.nseg * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    t.cis_c.assign(c.begin(), c.begin() + nbins);
    t.cis_s.assign(sm.begin(), sm.begin() + nbins);
    t.tr_c.assign(c.begin() + nbins, c.end());
    t.tr_s.assign(sm.begin() + nbins, sm.end());
    auto n_of = [&](uint32_t k) { return (uint64_t)(k + 1 < nchr ? off[k + 1] : nbins) - off[k]; };
    // trans: n_valid = valid bins of a x valid bins of b (diagonal 0 of the cis table), rows in (a, b) order
    t.tr_n.assign(s.trans_rows, 0);
    t.tr_e.assign(s.trans_rows, nan);
    uint64_t row = 0;
    for (uint32_t a = 0; a < nchr; ++a) {
        const uint64_t va = n_of(a) ? t.cis_n[off[a]] : 0;
        for (uint32_t b = a + 1; b < nchr; ++b, ++row) {
            const uint64_t n = va * (n_of(b) ? t.cis_n[off[b]] : 0);
            t.tr_n[row] = n;
            if (n) t.tr_e[row] = t.tr_s[row] / (double)n;
        }
    }
    // genome-wide: the cis rows added over the chromosomes in file order
    const uint64_t G = s.genome_rows;
    t.g_n.assign(G, 0); t.g_c.assign(G, 0); t.g_s.assign(G, 0.0); t.g_e.assign(G, nan); t.g_sm.assign(G, nan);
    for (uint32_t k = 0; k < nchr; ++k)
        for (uint64_t d = 0, n = n_of(k); d < n; ++d) { t.g_n[d] += t.cis_n[off[k] + d]; t.g_c[d] += t.cis_c[off[k] + d]; t.g_s[d] += t.cis_s[off[k] + d]; }
    for (uint64_t d = 0; d < G; ++d) if (t.g_n[d]) t.g_e[d] = t.g_s[d] / (double)t.g_n[d];
    // smoothed: diagonal 0 alone, then groups [e, e + max(1, e >> 3)), both sums in ascending d
    t.smooth_groups = 0;
    for (uint64_t a = 0, b = 1; a < G;) {
        const uint64_t end = b < G ? b : G;
        double ss = 0.0;
        uint64_t nn = 0;
        for (uint64_t d = a; d < end; ++d) { ss += t.g_s[d]; nn += t.g_n[d]; }
        if (nn) for (uint64_t d = a; d < end; ++d) t.g_sm[d] = ss / (double)nn;
        ++t.smooth_groups;
        a = b;
        b = a + ((a >> 3) > 1 ? (a >> 3) : 1);
    }
    MKT_TRY(t.d_cis_e.alloc(G, 64));
    MKT_TRY(t.d_cis_sm.alloc(G, 64));
    MKT_TRY(t.d_tr_e.alloc(s.trans_rows, 64));
    if (G) MKT_TRY(hipMemcpy(t.d_cis_e, t.g_e.data(), (size_t)G * 8, hipMemcpyHostToDevice));
    if (G) MKT_TRY(hipMemcpy(t.d_cis_sm, t.g_sm.data(), (size_t)G * 8, hipMemcpyHostToDevice));
    if (s.trans_rows) MKT_TRY(hipMemcpy(t.d_tr_e, t.tr_e.data(), (size_t)s.trans_rows * 8, hipMemcpyHostToDevice));
    t.built = true;
    return hipSuccess;
}

hipError_t exp_values(const ExpTables* t, const uint16_t* chr, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t first, uint64_t n,
                      const uint32_t* d_off, uint32_t nchr, const double* w, int kind, double* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (kind != 0 && (!chr || !t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ex_values, dim3(grid_for(n, EXWG)), dim3(EXWG), 0, st, b1, b2, cnt, first, n, w, kind, chr, d_off, nchr,
                       t ? (const double*)(kind == 2 ? t->d_cis_sm : t->d_cis_e) : nullptr, t ? (const double*)t->d_tr_e : nullptr, out);
    return hipGetLastError();
}

}  // namespace mkt

// ---- the entry points -----------------------------------------------------------------------------------------------------------
using namespace mkt;

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

extern "C" {

void mkt_expected_opts_default(mkt_expected_opts* o) {
    if (!o) return;
    o->use_weights = 1; o->reserved = 0;
}

int mkt_matrix_expected(mkt_matrix* m, uint32_t res_index, const mkt_expected_opts* opts, mkt_expected_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    const mkt_expected_opts o = mx_opts(opts, mkt_expected_opts_default);
    if (o.use_weights != 0 && o.use_weights != 1) return mfail(m, MKT_E_ARG, "expected: use_weights %d (0 or 1)", o.use_weights);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "expected: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | (o.use_weights ? MX_WEIGHTS : 0), "expected")) return rc;
    if (const int rc = mx_cells32(m, "expected", r.nnz)) return rc;
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    mx_invalidate(r, MX_NEW_TABLES);
    r.exp_sums_ms = r.exp_setup_ms = 0;
    if (!r.exs.built) {                                                 // with the chromosome of a bin when nothing has built it yet
        const hipError_t e = mx_timed(m, &r.exp_setup_ms, [&]() -> hipError_t {
            MKT_TRY(layout_chr(r.lay, mx_cells(r), st));
            return exp_setup(r.exs, r.lay.chr, r.d_b1, r.d_b2, r.d_cnt, r.nnz, r.nbins, r.d_off, r.off, st);
        });
        if (e == hipErrorInvalidValue) return mfail(m, MKT_E_CAPACITY, "expected: segment ids and cell indices of resolution index %u do not fit 64 bits together", res_index);
        MX_OR_RESET(m, "expected: ", r.ext, e);
    }
    MX_OR_RESET(m, "expected: ", r.ext, mx_timed(m, &r.exp_sums_ms, [&] { return exp_sums(r.exs, r.ext, r.lay.chr, r.nbins, r.d_off, o.use_weights ? r.d_w.get() : nullptr, st); }));
    MX_OR_RESET(m, "expected: ", r.ext, exp_finish(r.exs, r.ext, r.nbins, r.off, st));
    r.ext.use_weights = o.use_weights;
    if (info) {
        info->cis_rows = r.nbins; info->trans_rows = r.exs.trans_rows; info->genome_rows = r.exs.genome_rows;
        info->n_chrom = (uint32_t)r.off.size(); info->smooth_groups = r.ext.smooth_groups;
    }
    return MKT_OK;
}

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
    if (const int rc = mx_kind(m, "values", kind)) return rc;
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
    const bool have = m->ran && r.ext.built;
    mx_ms(setup_ms, have, r.exp_setup_ms); mx_ms(sums_ms, have, r.exp_sums_ms);
    return MKT_OK;
}

}  // extern "C"
