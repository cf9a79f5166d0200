// mkt_scc.hip -- the stratum-adjusted correlation of two binned contact matrices of one resolution on the GPU: both maps smoothed with
// a (2h + 1)^2 box filter, then the five sums of every diagonal (stratum) of every chromosome; the correlations and their weighted
// mean are formed on the host.  include/mkt.h has the definition; the entry points (mkt_matrix_scc, mkt_matrix_fetch_scc_*) are at
// the end, on the object of mkt_matrix_obj.h.
//
// Work goes chromosome by chromosome, in SLABS of whole chunks of 256 rows.
//  * The fill.  A slab's part of both matrices is laid out densely in BAND coordinates (row i, e = j - i): the rows of the slab and h
//    more on either side, e in [min_diag - 2h, max_diag + 2h] (rounded up to whole tiles of strata), the part below the diagonal
//    mirrored.  The band is zeroed, then one thread per stored cell of the rows that can reach it writes the cell and its mirror:
//    different cells have different addresses, so these are plain stores.
//  * The sweep.  A workgroup owns one chunk of 256 rows by a TILE of 8 strata and walks the chunk in four sub-blocks of 64 rows.  Per
//    sub-block it does the row pass of both matrices from the band (global memory, 2h + 1 neighbours along e, left to right) into LDS:
//    (64 + 2h) rows by (8 + 2h) values of R per matrix; the column pass then reads R along the anti-diagonal (row i + t, e = d - t:
//    the same column j), in ascending row.  Wave g holds strata 2g and 2g + 1 of the tile, lane l the row l of the sub-block; a lane
//    keeps the sub-blocks 0 + 2 and 1 + 3 apart and adds the two at the end, then the lanes go down the shuffle tree: this is the
//    tree of the definition over the 256 slots of the chunk (halves 128 and 64 across the sub-blocks, 32 .. 1 across the lanes).
//    One partial per (chunk, stratum) leaves; n and n_cand are integers.
//  * The fold adds a stratum's partials in ascending chunk order, one thread per stratum.
// Why the tile of the sweep is R and not the haloed band itself: at h = 16 the haloed band tile of both matrices does not fit the
// 64 KiB of LDS a workgroup may have (288 x 72 doubles per matrix); R of a sub-block does at every h (62976 bytes at h = 16).
//
// Steps 6 .. 8 are host code in this file, which is compiled without floating-point contraction (compared bit for bit with
// tests/sccdef.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

#pragma clang fp contract(off)

namespace mkt {

constexpr int SCC_WG = 256, SCC_SUB = 64, SCC_TILE = 8, SCC_SPT = SCC_TILE / (SCC_WG / 64);
typedef unsigned long long scc_u64;
static_assert(kSccChunk == 4 * SCC_SUB && SCC_WG == 4 * 64 && SCC_SPT * 4 == SCC_TILE, "four sub-blocks of one wave of rows; four waves share a tile of strata");

// one slab of one chromosome in band coordinates
struct SccGeo {
    int h, min_d, D;                              // D strata: min_d .. min_d + D - 1
    int64_t E, e_lo;                              // band columns: e in [e_lo, e_lo + E)
    int64_t rb0, rb1;                             // band rows (chromosome-relative; may lie outside the chromosome, where the band is zero)
    int64_t s0, s1;                               // the slab's own rows
    uint32_t off, nc, ntiles;                     // the chromosome's first bin and bins; tiles of strata
};

// V: [nbins + 1] jointly valid bins below k, or nullptr when every bin is valid
__device__ inline bool scc_valid(const uint32_t* V, uint64_t bin) { return !V || V[bin + 1] != V[bin]; }
// the jointly valid bins with relative index in [max(a, 0), min(b, nc - 1)] of the chromosome at `off`
__device__ inline uint32_t scc_nv(const uint32_t* V, uint32_t off, int64_t nc, int64_t a, int64_t b) {
    const int64_t lo = a > 0 ? a : 0, hi = b < nc - 1 ? b : nc - 1;
    return V ? V[off + hi + 1] - V[off + lo] : (uint32_t)(hi - lo + 1);
}

// cells [k0, k1) (rows of the chromosome) into the zeroed band; csum: the counts of the cells of the slab's own rows inside the strata
__global__ __launch_bounds__(SCC_WG) void k_scc_fill(SccSide m, const uint32_t* V, SccGeo g, uint64_t k0, uint64_t k1, double* band, scc_u64* csum) {
    const uint64_t k = k0 + (uint64_t)blockIdx.x * SCC_WG + threadIdx.x;
    scc_u64 c = 0;
    if (k < k1) {
        const uint32_t a = m.b1[k], b = m.b2[k];
        if (b < g.off + g.nc && scc_valid(V, a) && scc_valid(V, b)) {             // cis, both bins jointly valid
            const uint32_t cnt = m.cnt[k];
            const double v = m.w ? __dmul_rn(__dmul_rn((double)cnt, m.w[a]), m.w[b]) : (double)cnt;
            const int64_t i = (int64_t)a - g.off, j = (int64_t)b - g.off, e = j - i;
            if (i >= g.rb0 && i < g.rb1 && e >= g.e_lo && e < g.e_lo + g.E) band[(size_t)(i - g.rb0) * (size_t)g.E + (size_t)(e - g.e_lo)] = v;
            if (e > 0 && j >= g.rb0 && j < g.rb1 && -e >= g.e_lo && -e < g.e_lo + g.E) band[(size_t)(j - g.rb0) * (size_t)g.E + (size_t)(-e - g.e_lo)] = v;
            if (i >= g.s0 && i < g.s1 && e >= g.min_d && e < (int64_t)g.min_d + g.D) c = cnt;
        }
    }
    c = lane_tree<64>(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(csum, c);
}

// part: [chunk of the chromosome][5][D] the sums of a chunk, ipart: [chunk][2][D] n_cand and n.  One workgroup per (chunk of the
// slab, tile).  Dynamic LDS: 2 * (64 + 2h) * (8 + 2h + 1) doubles; the row stride is odd, so the lanes of the column pass (one row
// each) meet different banks.
__global__ __launch_bounds__(SCC_WG) void k_scc_sweep(const double* bandA, const double* bandB, const uint32_t* V, SccGeo g, double* part, scc_u64* ipart) {
    extern __shared__ double scc_lds[];
    const int h = g.h, RW = SCC_TILE + 2 * h, stride = RW + 1, rows = SCC_SUB + 2 * h;
    double* RA = scc_lds;
    double* RB = scc_lds + rows * stride;
    const uint32_t tile = blockIdx.x % g.ntiles, cq = blockIdx.x / g.ntiles;
    const int64_t i0 = g.s0 + (int64_t)cq * kSccChunk, nc = g.nc;
    const int64_t d0 = (int64_t)g.min_d + (int64_t)tile * SCC_TILE, d_end = (int64_t)g.min_d + g.D;
    const size_t chunk = (size_t)(i0 / kSccChunk), D = (size_t)g.D;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    if (i0 + d0 >= nc) {                                                          // no position of this chunk in any stratum of the tile
        if (threadIdx.x < SCC_TILE && d0 + threadIdx.x < d_end) {
            const size_t dd = (size_t)(d0 - g.min_d) + threadIdx.x;
#pragma unroll
            for (int k = 0; k < 5; ++k) part[(chunk * 5 + k) * D + dd] = 0.0;
            ipart[(chunk * 2 + 0) * D + dd] = 0; ipart[(chunk * 2 + 1) * D + dd] = 0;
        }
        return;
    }
    double acc[2][SCC_SPT][5];
    scc_u64 ncand[SCC_SPT], nused[SCC_SPT];
#pragma unroll
    for (int s = 0; s < SCC_SPT; ++s) { ncand[s] = 0; nused[s] = 0; }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t ib = i0 + (int64_t)b * SCC_SUB;
        const bool live = ib + d0 < nc;                                           // the same for every thread
        if (live) {
            __syncthreads();                                                      // the previous sub-block's R is read no more
            const int per = rows * RW;
            for (int idx = threadIdx.x; idx < 2 * per; idx += SCC_WG) {           // the row pass: R[row][e] = F[e - h] + .. + F[e + h]
                const int mat = idx >= per, rem = idx - mat * per, rr = rem / RW, ee = rem - rr * RW;
                const double* p = (mat ? bandB : bandA) + (size_t)(ib - h + rr - g.rb0) * (size_t)g.E + (size_t)tile * SCC_TILE + (size_t)ee;
                double sum = p[0];
                for (int t = 1; t <= 2 * h; ++t) sum = __dadd_rn(sum, p[t]);
                (mat ? RB : RA)[rr * stride + ee] = sum;
            }
            __syncthreads();
        }
        const int64_t i = ib + lane;
#pragma unroll
        for (int s = 0; s < SCC_SPT; ++s) {
            const int ds = grp * SCC_SPT + s;
            const int64_t d = d0 + ds, j = i + d;
            double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            if (live && d < d_end && j < nc && scc_valid(V, g.off + i) && scc_valid(V, g.off + j)) {      // a candidate
                ++ncand[s];
                // the column pass: rows i - h .. i + h of column j, that is e = d - t in row i + t
                double wa = RA[lane * stride + ds + 2 * h], wb = RB[lane * stride + ds + 2 * h];
                for (int t = 1; t <= 2 * h; ++t) {
                    wa = __dadd_rn(wa, RA[(lane + t) * stride + ds + 2 * h - t]);
                    wb = __dadd_rn(wb, RB[(lane + t) * stride + ds + 2 * h - t]);
                }
                const double nn = (double)((scc_u64)scc_nv(V, g.off, nc, i - h, i + h) * (scc_u64)scc_nv(V, g.off, nc, j - h, j + h));
                const double x = __ddiv_rn(wa, nn), y = __ddiv_rn(wb, nn);
                if (x != 0.0 || y != 0.0) {
                    ++nused[s];
                    v[0] = x; v[1] = y; v[2] = __dmul_rn(x, x); v[3] = __dmul_rn(y, y); v[4] = __dmul_rn(x, y);
                }
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[b & 1][s][k] = b < 2 ? v[k] : __dadd_rn(acc[b & 1][s][k], v[k]);      // slots k and k + 128
        }
    }
#pragma unroll
    for (int s = 0; s < SCC_SPT; ++s) {
        double t[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] = __dadd_rn(acc[0][s][k], acc[1][s][k]);                                  // slots k and k + 64
        lane_tree_v<64>(AddRn(), t[0], t[1], t[2], t[3], t[4], ncand[s], nused[s]);
        const int64_t d = d0 + grp * SCC_SPT + s;
        if (lane == 0 && d < d_end) {
            const size_t dd = (size_t)(d - g.min_d);
#pragma unroll
            for (int k = 0; k < 5; ++k) part[(chunk * 5 + k) * D + dd] = t[k];
            ipart[(chunk * 2 + 0) * D + dd] = ncand[s]; ipart[(chunk * 2 + 1) * D + dd] = nused[s];
        }
    }
}

// a stratum's partials in ascending chunk order into row `row0 + dd` of the table: tab [5][rows], itab [2][rows]
__global__ __launch_bounds__(256) void k_scc_fold(const double* part, const scc_u64* ipart, uint32_t chunks, uint32_t D, size_t row0, size_t rows, double* tab, scc_u64* itab) {
    const uint32_t dd = blockIdx.x * blockDim.x + threadIdx.x;
    if (dd >= D) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    scc_u64 n[2] = {0, 0};
    for (uint32_t c = 0; c < chunks; ++c) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = c ? __dadd_rn(s[k], part[((size_t)c * 5 + k) * D + dd]) : part[(size_t)k * D + dd];
        n[0] += ipart[((size_t)c * 2 + 0) * D + dd]; n[1] += ipart[((size_t)c * 2 + 1) * D + dd];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) tab[(size_t)k * rows + row0 + dd] = s[k];
    itab[row0 + dd] = n[0]; itab[rows + row0 + dd] = n[1];
}

// ---------------------------------------------------------------------------------------------------------------
// every NaN is the one quiet NaN (the scores are compared as bytes)
static double scc_q(double x) { return x != x ? std::numeric_limits<double>::quiet_NaN() : x; }

void scc_scores(SccState& s, uint32_t nchr, uint32_t strata, int weighting, uint64_t min_n) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t rows = (size_t)nchr * strata;
    s.rho.assign(rows, nan); s.w.assign(rows, 0.0);
    s.c_scc.assign(nchr, nan); s.c_num.assign(nchr, 0.0); s.c_den.assign(nchr, 0.0); s.c_scored.assign(nchr, 0);
    double num = 0.0, den = 0.0;
    uint64_t scored = 0;
    for (uint32_t c = 0; c < nchr; ++c) {
        double num_c = 0.0, den_c = 0.0;
        for (uint32_t k = 0; k < strata; ++k) {
            const size_t at = (size_t)c * strata + k;
            const uint64_t n = s.n[at];
            if (n < min_n) continue;
            const double nd = (double)n;
            const double mx = s.sx[at] / nd, my = s.sy[at] / nd;
            const double exx = s.sxx[at] / nd, eyy = s.syy[at] / nd;
            const double vx = exx - mx * mx, vy = eyy - my * my;
            const double cv = s.sxy[at] / nd - mx * my;
            if (!(vx > 0x1p-40 * exx) || !(vy > 0x1p-40 * eyy)) continue;
            const double sd = std::sqrt(vx * vy);
            s.rho[at] = scc_q(cv / sd);
            s.w[at] = weighting == MKT_SCC_WEIGHT_VAR ? nd * sd : nd;
            num_c += s.w[at] * s.rho[at]; den_c += s.w[at];
            ++s.c_scored[c];
        }
        s.c_num[c] = num_c; s.c_den[c] = den_c;
        if (s.c_scored[c]) s.c_scc[c] = scc_q(num_c / den_c);
        num += num_c; den += den_c;
        scored += s.c_scored[c];
    }
    s.info.scored = scored;
    s.info.scc = scored ? scc_q(num / den) : nan;
}

hipError_t scc_run(SccState& s, const SccSide& a, const SccSide& b, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_scc_opts& o, hipStream_t st, std::string* why) {
    if (nbins >= (1ull << 32) || a.nnz >= (1ull << 32) || b.nnz >= (1ull << 32)) return hipErrorInvalidValue;
    const uint32_t nchr = (uint32_t)off.size();
    const int h = o.h;
    const uint32_t D = (uint32_t)(o.max_diag - o.min_diag + 1), ntiles = (D + SCC_TILE - 1) / SCC_TILE;
    const int64_t E = (int64_t)ntiles * SCC_TILE + 4 * h, e_lo = (int64_t)o.min_diag - 2 * h;
    const size_t rows = (size_t)nchr * D;
    uint64_t nc_max = 0;
    for (uint32_t c = 0; c < nchr; ++c) nc_max = std::max<uint64_t>(nc_max, (c + 1 < nchr ? off[c + 1] : nbins) - off[c]);
    const uint64_t rows_max = (nc_max + kSccChunk - 1) / kSccChunk * kSccChunk, chunks_max = rows_max / kSccChunk;
    // the slab: as many whole chunks as half of the free memory holds for the two bands, or what the caller fixed
    size_t mem_free = 0, mem_total = 0;
    MKT_TRY(hipMemGetInfo(&mem_free, &mem_total));
    const uint64_t row_bytes = 2ull * (uint64_t)E * 8ull, budget_rows = (uint64_t)(mem_free / 2) / row_bytes;
    uint64_t slab = o.slab_rows ? (uint64_t)o.slab_rows : (budget_rows > 2ull * h ? (budget_rows - 2ull * h) / kSccChunk * kSccChunk : 0);
    if (slab < kSccChunk || slab + 2ull * h > budget_rows) {
        if (why) {
            char msg[256];
            snprintf(msg, sizeof msg, "the two bands of %llu rows by %lld diagonals (%llu bytes a row) do not fit half of the %zu free bytes", (unsigned long long)((slab < kSccChunk ? kSccChunk : slab) + 2ull * h),
                     (long long)E, (unsigned long long)row_bytes, mem_free);
            *why = msg;
        }
        return hipErrorOutOfMemory;
    }
    slab = std::min(slab, std::max<uint64_t>(rows_max, kSccChunk));
    if ((slab / kSccChunk) * (uint64_t)ntiles >= (1ull << 31)) return hipErrorInvalidValue;
    // the jointly valid bins, as a prefix count
    std::vector<uint32_t> V;
    DevBuf<uint32_t> d_V;
    if (o.use_weights) {
        std::vector<double> wa(nbins), wb(nbins);
        if (nbins) {
            MKT_TRY(hipMemcpyAsync(wa.data(), a.w, (size_t)nbins * 8, hipMemcpyDeviceToHost, st));
            MKT_TRY(hipMemcpyAsync(wb.data(), b.w, (size_t)nbins * 8, hipMemcpyDeviceToHost, st));
        }
        MKT_TRY(hipStreamSynchronize(st));
        V.assign(nbins + 1, 0);
        for (uint64_t k = 0; k < nbins; ++k) V[k + 1] = V[k] + (wa[k] == wa[k] && wb[k] == wb[k] ? 1u : 0u);
        MKT_TRY(d_V.alloc(nbins + 1));
        MKT_TRY(hipMemcpyAsync(d_V, V.data(), (size_t)(nbins + 1) * 4, hipMemcpyHostToDevice, st));
    }
    // the cells of a range of rows, from the row pointers
    std::vector<uint32_t> rpa(nbins + 1), rpb(nbins + 1);
    MKT_TRY(hipMemcpyAsync(rpa.data(), a.rowptr, (size_t)(nbins + 1) * 4, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(rpb.data(), b.rowptr, (size_t)(nbins + 1) * 4, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    DevEvents<3> ev;
    MKT_TRY(ev.create());
    DevBuf<double> d_A, d_B, d_part, d_tab;
    DevBuf<scc_u64> d_ipart, d_itab, d_cs;
    const size_t band_elems = (size_t)(slab + 2ull * h) * (size_t)E;
    MKT_TRY(d_A.alloc(band_elems, 64)); MKT_TRY(d_B.alloc(band_elems, 64));
    MKT_TRY(d_part.alloc(std::max<size_t>(chunks_max, 1) * 5 * D)); MKT_TRY(d_ipart.alloc(std::max<size_t>(chunks_max, 1) * 2 * D));
    MKT_TRY(d_tab.alloc(5 * rows)); MKT_TRY(d_itab.alloc(2 * rows)); MKT_TRY(d_cs.alloc(2));
    MKT_TRY(hipMemsetAsync(d_cs, 0, 16, st));
    const size_t lds = 2 * (size_t)(SCC_SUB + 2 * h) * (size_t)(SCC_TILE + 2 * h + 1) * 8;
    double fill_ms = 0, sweep_ms = 0;
    for (uint32_t c = 0; c < nchr; ++c) {
        const int64_t nc = (int64_t)((c + 1 < nchr ? off[c + 1] : nbins) - off[c]);
        const int64_t rows_c = (nc + kSccChunk - 1) / kSccChunk * kSccChunk;
        for (int64_t s0 = 0; s0 < rows_c || (s0 == 0 && rows_c == 0); s0 += (int64_t)slab) {
            SccGeo g;
            g.h = h; g.min_d = o.min_diag; g.D = (int)D; g.E = E; g.e_lo = e_lo;
            g.s0 = s0; g.s1 = std::min<int64_t>(s0 + (int64_t)slab, rows_c); g.rb0 = g.s0 - h; g.rb1 = g.s1 + h;
            g.off = off[c]; g.nc = (uint32_t)nc; g.ntiles = ntiles;
            const bool last = g.s1 >= rows_c;
            MKT_TRY(hipEventRecord(ev[0], st));
            if (rows_c) {
                const size_t bytes = (size_t)(g.rb1 - g.rb0) * (size_t)E * 8;
                MKT_TRY(hipMemsetAsync(d_A, 0, bytes, st)); MKT_TRY(hipMemsetAsync(d_B, 0, bytes, st));
                const int64_t lo = std::min<int64_t>(std::max<int64_t>(g.rb0 - std::max<int64_t>(0, -e_lo), 0), nc), hi = std::min<int64_t>(std::max<int64_t>(g.rb1, 0), nc);
                const uint64_t ka0 = rpa[off[c] + lo], ka1 = rpa[off[c] + hi], kb0 = rpb[off[c] + lo], kb1 = rpb[off[c] + hi];
                if (ka1 > ka0) hipLaunchKernelGGL(k_scc_fill, dim3(grid_for(ka1 - ka0, SCC_WG)), dim3(SCC_WG), 0, st, a, (const uint32_t*)d_V.get(), g, ka0, ka1, d_A.get(), d_cs.get());
                if (kb1 > kb0) hipLaunchKernelGGL(k_scc_fill, dim3(grid_for(kb1 - kb0, SCC_WG)), dim3(SCC_WG), 0, st, b, (const uint32_t*)d_V.get(), g, kb0, kb1, d_B.get(), d_cs.get() + 1);
            }
            MKT_TRY(hipEventRecord(ev[1], st));
            if (rows_c) {
                const unsigned grid = (unsigned)((uint64_t)((g.s1 - g.s0) / kSccChunk) * ntiles);
                hipLaunchKernelGGL(k_scc_sweep, dim3(grid), dim3(SCC_WG), lds, st, (const double*)d_A.get(), (const double*)d_B.get(), (const uint32_t*)d_V.get(), g, d_part.get(), d_ipart.get());
            }
            if (last) hipLaunchKernelGGL(k_scc_fold, dim3(grid_for(D, 256)), dim3(256), 0, st, (const double*)d_part.get(), (const scc_u64*)d_ipart.get(), (uint32_t)(rows_c / kSccChunk), D, (size_t)c * D, rows, d_tab.get(), d_itab.get());
            MKT_TRY(hipEventRecord(ev[2], st));
            MKT_TRY(hipGetLastError());
            MKT_TRY(hipStreamSynchronize(st));                                    // the events are read and recorded again
            float ms = 0;
            MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); fill_ms += ms;
            MKT_TRY(hipEventElapsedTime(&ms, ev[1], ev[2])); sweep_ms += ms;
            if (rows_c == 0) break;
        }
    }
    std::vector<double> tab(5 * rows);
    std::vector<uint64_t> itab(2 * rows);
    uint64_t cs[2] = {0, 0};
    if (rows) {
        MKT_TRY(hipMemcpyAsync(tab.data(), d_tab, 5 * rows * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipMemcpyAsync(itab.data(), d_itab, 2 * rows * 8, hipMemcpyDeviceToHost, st));
    }
    MKT_TRY(hipMemcpyAsync(cs, d_cs, 16, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    s.n_cand.assign(itab.begin(), itab.begin() + rows); s.n.assign(itab.begin() + rows, itab.end());
    s.sx.assign(tab.begin(), tab.begin() + rows); s.sy.assign(tab.begin() + rows, tab.begin() + 2 * rows); s.sxx.assign(tab.begin() + 2 * rows, tab.begin() + 3 * rows);
    s.syy.assign(tab.begin() + 3 * rows, tab.begin() + 4 * rows); s.sxy.assign(tab.begin() + 4 * rows, tab.end());
    memset(&s.info, 0, sizeof s.info);
    s.info.n_chrom = nchr; s.info.strata = D; s.info.count_a = cs[0]; s.info.count_b = cs[1];
    for (size_t k = 0; k < rows; ++k) { s.info.candidates += s.n_cand[k]; s.info.used += s.n[k]; }
    scc_scores(s, nchr, D, o.weighting, (uint64_t)o.min_n);
    s.fill_ms = fill_ms; s.sweep_ms = sweep_ms;
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points (comparisons and copies only: nothing here rounds) ------------------------------------------------------------
using namespace mkt;
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
    mkt_scc_opts o = mx_opts(opts, mkt_scc_opts_default);
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
    mx_ms(fill_ms, have, s.fill_ms); mx_ms(sweep_ms, have, s.sweep_ms);
    return MKT_OK;
}

}  // extern "C"
