// mkt_loops.hip -- loop calling over one resolution's binned contact matrix on the GPU: donut enrichment of every candidate cell
// against its neighbourhood, the (expected chunk x count) histogram, the flags against the FDR thresholds; include/mkt.h has the
// definition; the entry points (mkt_matrix_loops, mkt_matrix_fetch_loop_*) are at the end, on the object of mkt_matrix_obj.h.
//
// The neighbourhood pass.  A GROUP of lanes owns one candidate cell (i, j) and its window w.  The group stages what all its lanes
// share: E[d] for the 4 w + 1 diagonals (j - i) - 2 w .. (j - i) + 2 w in LDS, the validity of the columns j - w .. j + w as a bit
// mask.  Lane l then takes the rows a = -w + l, -w + l + lanes, ..: for a valid row inside the chromosome it adds E over the kept
// positions of the four regions in ascending b (that sum does not look at the cells), finds column j - w of row i + a by a binary
// search between the row pointers and walks the short run of stored cells up to column j + w, adding v and (for LL) the count.
// The lane tree adds the lanes.  Nothing depends on the order anything ran in: the sums have one shape per (w, lanes).
//
// Window growth makes the work uneven, so there are two launches.  The first gives every cell 16 lanes and the starting window; a
// candidate whose Csum_LL is below min_ll_count is appended to a list instead of being written (the list's order is arbitrary and
// never shows: every cell is computed on its own).  The second gives every listed cell a wave: its lanes count the LL cells of the
// rows 1 .. window_max into rings m = max(a, -b) (integer LDS atomics), every lane derives the final w from the ring sums, and the
// same sums run at that w.
//
// The histogram (integer atomics, the low columns pre-added per workgroup in LDS) and the flags are one thread per cell; thresholds and clustering are host code in this file, which
// is compiled without floating-point contraction (the thresholds are compared bit for bit with tests/loopsdef.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

#pragma clang fp contract(off)

namespace mkt {

constexpr int LPWG = 256;
constexpr int kLpE = 4 * kLpWmax + 1;
typedef unsigned long long lp_u64;

struct LpOut {
    uint8_t *status, *window, *chunk;
    uint16_t* kept;
    lp_u64* csum;
    double *r, *e, *bsum, *esum;
    uint32_t *grow_list, *grow_n;
};
struct LpOpts { int p, window, wmax; lp_u64 min_ll; uint32_t min_dist, max_dist; };

__constant__ double c_lp_edges[kLpChunks];

__device__ inline bool lp_valid(const double* w, int64_t k, int64_t lo, int64_t hi) {
    if (k < lo || k >= hi) return false;
    if (!w) return true;
    const double x = w[k];
    return x == x;
}
struct LpCell { int64_t i, j, lo, hi; uint32_t count; bool cand; };
__device__ inline LpCell lp_cell(const LoopsIn& in, const LpOpts& o, uint64_t s) {
    LpCell c;
    c.i = in.b1[s]; c.j = in.b2[s]; c.count = in.cnt[s];
    const uint32_t ca = in.chr[c.i], cb = in.chr[c.j];
    c.lo = in.off[ca];
    c.hi = ca + 1u < in.nchr ? (int64_t)in.off[ca + 1u] : (int64_t)in.nbins;
    const int64_t d = c.j - c.i;
    c.cand = ca == cb && d >= (int64_t)o.min_dist && (o.max_dist == 0 || d <= (int64_t)o.max_dist) && lp_valid(in.w, c.i, c.lo, c.hi) && lp_valid(in.w, c.j, c.lo, c.hi);
    return c;
}
__device__ inline void lp_write_none(const LpOut& out, uint64_t s) {
    const double nan = dev_nan();
    out.status[s] = MKT_LOOP_NONE; out.window[s] = 0; out.csum[s] = 0;
    for (int R = 0; R < 4; ++R) {
        out.chunk[4 * s + R] = kLpNoChunk; out.kept[4 * s + R] = 0;
        out.r[4 * s + R] = nan; out.e[4 * s + R] = nan; out.bsum[4 * s + R] = 0.0; out.esum[4 * s + R] = 0.0;
    }
}

// The sums of cell c at window w (w < 0: nothing to do, the group only keeps the barriers company) by the G lanes of its group, lane
// gl.  E: the group's kLpE doubles of LDS.  Valid in lane 0 afterwards.  Every thread of the workgroup calls this.
template <int G>
__device__ inline void lp_sums(const LoopsIn& in, const LpOpts& o, const LpCell& c, int w, uint32_t gl, double* E, double (&B)[4], double (&Es)[4], uint32_t (&P)[4], lp_u64& cs) {
    const int64_t dmid = c.j - c.i;
    for (int t = (int)gl; t <= 4 * w; t += G) {
        const int64_t d = dmid - 2 * w + t;
        E[t] = d >= 0 && d < (int64_t)in.genome_rows ? in.E[d] : 0.0;
    }
    lp_u64 cm = 0;                                                         // bit t: column j - w + t is inside the chromosome and valid
    for (int t = (int)gl; t <= 2 * w; t += G) if (lp_valid(in.w, c.j - w + t, c.lo, c.hi)) cm |= 1ull << t;
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) cm |= __shfl_xor(cm, d, G);
    __syncthreads();
    for (int R = 0; R < 4; ++R) { B[R] = 0.0; Es[R] = 0.0; P[R] = 0; }
    cs = 0;
    const int p = o.p;
    for (int a = -w + (int)gl; a <= w; a += G) {
        const int64_t row = c.i + a;
        if (!lp_valid(in.w, row, c.lo, c.hi)) continue;
        const double wr = in.w ? in.w[row] : 1.0;
        const int aa = a < 0 ? -a : a;
        for (int b = -w; b <= w; ++b) {                                    // E over the kept positions, ascending b
            if (!((cm >> (b + w)) & 1ull) || (c.j + b) - row < 1) continue;
            const double ev = E[b - a + 2 * w];
            const int bb = b < 0 ? -b : b;
            const bool inpk = aa <= p && bb <= p;
            if (!inpk && a != 0 && b != 0) { Es[0] += ev; ++P[0]; }
            if (!inpk && a >= 1 && b <= -1) { Es[1] += ev; ++P[1]; }
            if (aa <= 1 && bb > p) { Es[2] += ev; ++P[2]; }
            if (aa > p && bb <= 1) { Es[3] += ev; ++P[3]; }
        }
        const uint32_t r1 = in.rowptr[row + 1];
        const int64_t c0 = c.j - w;
        for (uint32_t s = seg_lower_bound(in.b2, in.rowptr[row], r1, c0 < 0 ? 0u : (uint32_t)c0); s < r1; ++s) {       // the stored cells of the row, ascending b
            const int64_t col = in.b2[s];
            if (col > c.j + w) break;
            const int b = (int)(col - c.j);
            if (!((cm >> (b + w)) & 1ull) || col - row < 1) continue;
            const uint32_t n = in.cnt[s];
            const double v = ((double)n * wr) * (in.w ? in.w[col] : 1.0);
            const int bb = b < 0 ? -b : b;
            const bool inpk = aa <= p && bb <= p;
            if (!inpk && a != 0 && b != 0) B[0] += v;
            if (!inpk && a >= 1 && b <= -1) { B[1] += v; cs += n; }
            if (aa <= 1 && bb > p) B[2] += v;
            if (aa > p && bb <= 1) B[3] += v;
        }
    }
    lane_tree_v<G>(AddPlain(), B[0], Es[0], P[0], B[1], Es[1], P[1], B[2], Es[2], P[2], B[3], Es[3], P[3], cs);
}
// lane 0 of the group: steps 4 and 5 from the sums.  Ecen = E[j - i].
__device__ inline void lp_finish(const LoopsIn& in, const LpOut& out, const LpCell& c, uint64_t s, int w, double Ecen, const double* B, const double* Es, const uint32_t* P, lp_u64 cs) {
    const double nan = dev_nan();
    const double ww = (in.w ? in.w[c.i] : 1.0) * (in.w ? in.w[c.j] : 1.0);
    bool undef = false, over = false;
    for (int R = 0; R < 4; ++R) {
        double e = nan, r = nan;
        uint8_t k = kLpNoChunk;
        if (P[R] > 0 && Es[R] != 0.0) {
            e = (B[R] / Es[R]) * Ecen;
            r = e / ww;
            if (r <= c_lp_edges[kLpChunks - 1]) { k = 0; while (!(r <= c_lp_edges[k])) ++k; }
            else over = true;
        } else undef = true;
        out.chunk[4 * s + R] = k; out.kept[4 * s + R] = (uint16_t)P[R];
        out.r[4 * s + R] = r; out.e[4 * s + R] = e; out.bsum[4 * s + R] = B[R]; out.esum[4 * s + R] = Es[R];
    }
    out.status[s] = undef ? MKT_LOOP_UNDEFINED : over ? MKT_LOOP_OVER : MKT_LOOP_TESTED;
    out.window[s] = (uint8_t)w; out.csum[s] = cs;
}

// first launch: 16 lanes per cell, the starting window
__global__ __launch_bounds__(LPWG) void k_lp_pass(LoopsIn in, LpOpts o, LpOut out) {
    constexpr int G = 16;
    __shared__ double shE[LPWG / G][kLpE + 3];
    const uint64_t s = (uint64_t)blockIdx.x * (LPWG / G) + threadIdx.x / G;
    const uint32_t gl = threadIdx.x & (G - 1), g = threadIdx.x / G;
    LpCell c = {0, 0, 0, 0, 0, false};
    if (s < in.nnz) c = lp_cell(in, o, s);
    double B[4], Es[4];
    uint32_t P[4];
    lp_u64 cs;
    lp_sums<G>(in, o, c, c.cand ? o.window : -1, gl, shE[g], B, Es, P, cs);
    if (s >= in.nnz || gl != 0) return;
    if (!c.cand) { lp_write_none(out, s); return; }
    if (cs < o.min_ll && o.window < o.wmax) { out.grow_list[atomicAdd(out.grow_n, 1u)] = (uint32_t)s; return; }
    lp_finish(in, out, c, s, o.window, shE[g][2 * o.window], B, Es, P, cs);
}
// second launch: a wave per cell whose window grows
__global__ __launch_bounds__(LPWG) void k_lp_grow(LoopsIn in, LpOpts o, LpOut out, uint32_t ngrow) {
    constexpr int G = 64;
    __shared__ double shE[LPWG / G][kLpE + 3];
    __shared__ lp_u64 ring[LPWG / G][kLpWmax + 1];
    const uint32_t t = blockIdx.x * (LPWG / G) + threadIdx.x / G;
    const uint32_t gl = threadIdx.x & (G - 1), g = threadIdx.x / G;
    const bool mine = t < ngrow;
    uint64_t s = 0;
    LpCell c = {0, 0, 0, 0, 0, false};
    if (mine) { s = out.grow_list[t]; c = lp_cell(in, o, s); }
    if (gl <= (uint32_t)kLpWmax) ring[g][gl] = 0;
    __syncthreads();
    const int a = 1 + (int)gl;
    if (c.cand && a <= o.wmax) {
        const int64_t row = c.i + a;
        if (lp_valid(in.w, row, c.lo, c.hi)) {
            const uint32_t r1 = in.rowptr[row + 1];
            const int64_t c0 = c.j - o.wmax < c.lo ? c.lo : c.j - o.wmax;
            for (uint32_t q = seg_lower_bound(in.b2, in.rowptr[row], r1, (uint32_t)c0); q < r1; ++q) {
                const int64_t col = in.b2[q];
                if (col >= c.j) break;
                const int bb = (int)(c.j - col);
                if (col - row < 1 || (a <= o.p && bb <= o.p) || !lp_valid(in.w, col, c.lo, c.hi)) continue;
                atomicAdd(&ring[g][a > bb ? a : bb], (lp_u64)in.cnt[q]);    // integers: the same sum in any order
            }
        }
    }
    __syncthreads();
    int w = -1;
    if (c.cand) {
        lp_u64 cum = 0;
        for (int m = 1; m <= o.window; ++m) cum += ring[g][m];
        w = o.window;
        while (cum < o.min_ll && w < o.wmax) { ++w; cum += ring[g][w]; }
    }
    double B[4], Es[4];
    uint32_t P[4];
    lp_u64 cs;
    lp_sums<G>(in, o, c, w, gl, shE[g], B, Es, P, cs);
    if (c.cand && gl == 0) lp_finish(in, out, c, s, w, shE[g][2 * w], B, Es, P, cs);
}

// counters: 0 candidates, 1 tested, 2 undefined, 3 over, 4 grew, 5 at_max, 6 enriched
// A workgroup takes kLpHistCells consecutive cells.  On sparse matrices nearly every tested cell has the same small (chunk, count), so the
// columns below kLpHistLow are first counted in LDS (integer atomics) and added to H once per workgroup; the rest go to H directly.
constexpr int kLpHistCells = 16 * LPWG, kLpHistLow = 8;
__global__ __launch_bounds__(LPWG) void k_lp_hist(const uint8_t* status, const uint8_t* window, const uint8_t* chunk, const lp_u64* csum, const uint32_t* cnt, uint64_t nnz,
                                                  LpOpts o, lp_u64* H, lp_u64* counters) {
    __shared__ uint32_t sh[6];
    __shared__ uint32_t low[4 * kLpChunks * kLpHistLow];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0;
    for (int t = threadIdx.x; t < 4 * kLpChunks * kLpHistLow; t += LPWG) low[t] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kLpHistCells;
    for (int q = 0; q < kLpHistCells / LPWG; ++q) {
        const uint64_t s = base + (uint64_t)q * LPWG + threadIdx.x;
        if (s >= nnz) break;
        const uint8_t st = status[s];
        if (st != MKT_LOOP_NONE) {
            atomicAdd(&sh[0], 1u);
            atomicAdd(&sh[st], 1u);
            if ((int)window[s] > o.window) atomicAdd(&sh[4], 1u);
            if ((int)window[s] == o.wmax && csum[s] < o.min_ll) atomicAdd(&sh[5], 1u);
        }
        if (st == MKT_LOOP_TESTED) {
            const uint32_t x = cnt[s] < (uint32_t)(kLpCols - 1) ? cnt[s] : (uint32_t)(kLpCols - 1);
            for (int R = 0; R < 4; ++R) {
                const uint32_t k = chunk[4 * s + R];                        // < kLpChunks for a tested cell
                if (x < (uint32_t)kLpHistLow) atomicAdd(&low[(R * kLpChunks + k) * kLpHistLow + x], 1u);
                else atomicAdd(&H[((uint64_t)R * kLpChunks + k) * kLpCols + x], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (lp_u64)sh[threadIdx.x]);
    for (int t = threadIdx.x; t < 4 * kLpChunks * kLpHistLow; t += LPWG)
        if (low[t]) atomicAdd(&H[(uint64_t)(t / kLpHistLow) * kLpCols + (t % kLpHistLow)], (lp_u64)low[t]);
}
__global__ __launch_bounds__(LPWG) void k_lp_flag(const uint8_t* status, const uint8_t* chunk, const uint32_t* cnt, uint64_t nnz, const uint32_t* T, uint8_t* enriched,
                                                  uint32_t* list, lp_u64* counters) {
    const uint64_t s = (uint64_t)blockIdx.x * LPWG + threadIdx.x;
    if (s >= nnz) return;
    bool en = status[s] == MKT_LOOP_TESTED;
    if (en) for (int R = 0; R < 4; ++R) en = en && cnt[s] >= T[R * kLpChunks + chunk[4 * s + R]];
    enriched[s] = en ? 1 : 0;
    if (en) list[(uint32_t)atomicAdd(&counters[6], 1ull)] = (uint32_t)s;     // sorted by the host before anything reads it
}
struct LpPeak { uint32_t b1, b2, count, window; double r[4]; };
__global__ __launch_bounds__(LPWG) void k_lp_gather(const uint32_t* list, uint32_t n, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, const uint8_t* window, const double* r, LpPeak* out) {
    const uint32_t t = blockIdx.x * LPWG + threadIdx.x;
    if (t >= n) return;
    const uint32_t s = list[t];
    LpPeak x;
    x.b1 = b1[s]; x.b2 = b2[s]; x.count = cnt[s]; x.window = window[s];
    for (int R = 0; R < 4; ++R) x.r[R] = r[4 * (uint64_t)s + R];
    out[t] = x;
}

// ---------------------------------------------------------------------------------------------------------------
double loops_edge(int k) {
    static const double C[3] = {1.0, 1.2599210498948732, 1.5874010519681994};
    return std::ldexp(C[k % 3], k / 3);
}

void loops_thresholds(const uint64_t* hist, double fdr, uint32_t* thr) {
    std::vector<double> Q(kLpCols + 1);
    std::vector<uint64_t> O(kLpCols + 1);
    for (int k = 0; k < kLpChunks; ++k) {
        const double lambda = loops_edge(k);
        double pmf = std::exp(-lambda), cdf = pmf;                       // cdf_0
        Q[0] = 1.0;
        for (int x = 1; x <= kLpCols; ++x) {
            const double q = 1.0 - cdf;                                   // 1 - cdf_(x-1)
            Q[x] = q > 0.0 ? q : 0.0;
            pmf = (pmf * lambda) / (double)x;
            cdf = cdf + pmf;
        }
        for (int R = 0; R < 4; ++R) {
            const uint64_t* H = hist + ((size_t)R * kLpChunks + k) * kLpCols;
            O[kLpCols] = 0;
            for (int x = kLpCols - 1; x >= 0; --x) O[x] = O[x + 1] + H[x];
            const double n = (double)O[0];
            uint32_t T = kLpCols;
            for (int x = 1; x < kLpCols; ++x)
                if (O[x] > 0 && n * Q[x] <= fdr * (double)O[x]) { T = (uint32_t)x; break; }
            thr[R * kLpChunks + k] = T;
        }
    }
}

// step 9: the components of the enriched cells (ascending cell index), linked within `radius` inside one chromosome
static void lp_cluster(const std::vector<uint32_t>& cell, const std::vector<LpPeak>& pk, const std::vector<uint32_t>& off, uint64_t nbins, int radius, std::vector<mkt_loop>& loops) {
    const size_t n = cell.size();
    std::vector<uint32_t> parent(n), chrom(n);
    std::unordered_map<uint64_t, uint32_t> at;
    at.reserve(n * 2);
    for (size_t t = 0; t < n; ++t) {
        parent[t] = (uint32_t)t;
        chrom[t] = (uint32_t)(std::upper_bound(off.begin(), off.end(), pk[t].b1) - off.begin() - 1);
        at[((uint64_t)pk[t].b1 << 32) | pk[t].b2] = (uint32_t)t;
    }
    auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t t = 0; t < n; ++t)
        for (int64_t da = -radius; da <= radius; ++da)
            for (int64_t db = -radius; db <= radius; ++db) {
                const int64_t x = (int64_t)pk[t].b1 + da, y = (int64_t)pk[t].b2 + db;
                if (x < 0 || y < 0 || x >= (int64_t)nbins || y >= (int64_t)nbins) continue;
                auto it = at.find(((uint64_t)x << 32) | (uint64_t)y);
                if (it == at.end() || chrom[it->second] != chrom[t]) continue;
                const uint32_t ra = find((uint32_t)t), rb = find(it->second);
                if (ra != rb) parent[ra > rb ? ra : rb] = ra > rb ? rb : ra;
            }
    std::unordered_map<uint32_t, size_t> row;                             // root -> its loop
    for (size_t t = 0; t < n; ++t) {                                      // ascending cell index: a tie keeps the smaller index
        const uint32_t root = find((uint32_t)t);
        auto it = row.find(root);
        if (it == row.end()) {
            mkt_loop L;
            memset(&L, 0, sizeof L);
            L.cell = cell[t]; L.bin1 = pk[t].b1; L.bin2 = pk[t].b2; L.count = pk[t].count; L.window = pk[t].window; L.n_cells = 1;
            L.box[0] = L.box[1] = pk[t].b1; L.box[2] = L.box[3] = pk[t].b2;
            for (int R = 0; R < 4; ++R) L.r[R] = pk[t].r[R];
            row[root] = loops.size();
            loops.push_back(L);
            continue;
        }
        mkt_loop& L = loops[it->second];
        ++L.n_cells;
        L.box[0] = std::min(L.box[0], pk[t].b1); L.box[1] = std::max(L.box[1], pk[t].b1);
        L.box[2] = std::min(L.box[2], pk[t].b2); L.box[3] = std::max(L.box[3], pk[t].b2);
        if (pk[t].count > L.count) {
            L.cell = cell[t]; L.bin1 = pk[t].b1; L.bin2 = pk[t].b2; L.count = pk[t].count; L.window = pk[t].window;
            for (int R = 0; R < 4; ++R) L.r[R] = pk[t].r[R];
        }
    }
    std::sort(loops.begin(), loops.end(), [](const mkt_loop& a, const mkt_loop& b) { return a.cell < b.cell; });
}

hipError_t loops_run(LoopsState& s, const LoopsIn& in, const std::vector<uint32_t>& off, const mkt_loops_opts& opts, hipStream_t st) {
    const uint64_t nnz = in.nnz;
    if (nnz >= (1ull << 32)) return hipErrorInvalidValue;
    DevBuf<lp_u64> d_H, d_counters;
    DevBuf<uint32_t> d_T, d_list;
    DevBuf<LpPeak> d_peaks;
    DevEvents<6> ev;
    MKT_TRY(ev.create());
    const size_t n1 = (size_t)nnz + 64, n4 = 4 * (size_t)nnz + 64, hbytes = (size_t)4 * kLpChunks * kLpCols * 8;
    MKT_TRY(s.status.alloc(n1)); MKT_TRY(s.window.alloc(n1)); MKT_TRY(s.chunk.alloc(n4)); MKT_TRY(s.enriched.alloc(n1));
    MKT_TRY(s.kept.alloc(n4)); MKT_TRY(s.csum.alloc(n1));
    MKT_TRY(s.r.alloc(n4)); MKT_TRY(s.e.alloc(n4)); MKT_TRY(s.bsum.alloc(n4)); MKT_TRY(s.esum.alloc(n4));
    MKT_TRY(d_H.alloc(4 * kLpChunks * kLpCols)); MKT_TRY(d_counters.alloc(8)); MKT_TRY(d_T.alloc(4 * kLpChunks));
    MKT_TRY(d_list.alloc(n1));
    MKT_TRY(hipMemsetAsync(d_H, 0, hbytes, st)); MKT_TRY(hipMemsetAsync(d_counters, 0, 8 * 8, st));
    double edges[kLpChunks];
    for (int k = 0; k < kLpChunks; ++k) edges[k] = loops_edge(k);
    MKT_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_lp_edges), edges, sizeof edges, 0, hipMemcpyHostToDevice, st));
    LpOpts o;
    o.p = opts.peak; o.window = opts.window; o.wmax = opts.window_max; o.min_ll = (lp_u64)opts.min_ll_count; o.min_dist = (uint32_t)opts.min_dist; o.max_dist = (uint32_t)opts.max_dist;
    LpOut out;
    out.status = s.status; out.window = s.window; out.chunk = s.chunk; out.kept = s.kept; out.csum = (lp_u64*)s.csum.get();
    out.r = s.r; out.e = s.e; out.bsum = s.bsum; out.esum = s.esum;
    out.grow_list = d_list; out.grow_n = (uint32_t*)(d_counters.get() + 7);
    const unsigned cgrid = grid_for(nnz, LPWG);
    uint32_t ngrow = 0;
    MKT_TRY(hipEventRecord(ev[0], st));
    if (nnz) {
        hipLaunchKernelGGL(k_lp_pass, dim3(grid_for(nnz, LPWG / 16)), dim3(LPWG), 0, st, in, o, out);
        MKT_TRY(hipMemcpyAsync(&ngrow, out.grow_n, 4, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipStreamSynchronize(st));
        if (ngrow) hipLaunchKernelGGL(k_lp_grow, dim3(grid_for(ngrow, LPWG / 64)), dim3(LPWG), 0, st, in, o, out, ngrow);
    }
    MKT_TRY(hipEventRecord(ev[1], st));
    MKT_TRY(hipEventRecord(ev[2], st));
    if (nnz) hipLaunchKernelGGL(k_lp_hist, dim3(grid_for(nnz, kLpHistCells)), dim3(LPWG), 0, st, (const uint8_t*)s.status, (const uint8_t*)s.window, (const uint8_t*)s.chunk, (const lp_u64*)s.csum.get(), in.cnt, nnz, o, d_H, d_counters);
    MKT_TRY(hipEventRecord(ev[3], st));
    MKT_TRY(hipGetLastError());
    s.hist.assign((size_t)4 * kLpChunks * kLpCols, 0);
    s.thr.assign(4 * kLpChunks, 0);
    MKT_TRY(hipMemcpyAsync(s.hist.data(), d_H, hbytes, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    loops_thresholds(s.hist.data(), opts.fdr, s.thr.data());
    MKT_TRY(hipMemcpyAsync(d_T, s.thr.data(), 4 * kLpChunks * 4, hipMemcpyHostToDevice, st));
    MKT_TRY(hipEventRecord(ev[4], st));
    if (nnz) hipLaunchKernelGGL(k_lp_flag, dim3(cgrid), dim3(LPWG), 0, st, (const uint8_t*)s.status, (const uint8_t*)s.chunk, in.cnt, nnz, (const uint32_t*)d_T, s.enriched, d_list, d_counters);
    MKT_TRY(hipEventRecord(ev[5], st));
    MKT_TRY(hipGetLastError());
    lp_u64 hc[8];
    MKT_TRY(hipMemcpyAsync(hc, d_counters, sizeof hc, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); s.pass_ms = ms;
    MKT_TRY(hipEventElapsedTime(&ms, ev[2], ev[3])); s.hist_ms = ms;
    MKT_TRY(hipEventElapsedTime(&ms, ev[4], ev[5])); s.flag_ms = ms;
    const uint32_t nen = (uint32_t)hc[6];
    std::vector<uint32_t> cell(nen);
    std::vector<LpPeak> pk(nen);
    if (nen) {
        MKT_TRY(hipMemcpyAsync(cell.data(), d_list, (size_t)nen * 4, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipStreamSynchronize(st));
        std::sort(cell.begin(), cell.end());
        MKT_TRY(hipMemcpyAsync(d_list, cell.data(), (size_t)nen * 4, hipMemcpyHostToDevice, st));          // `cell` is not touched before the next synchronise
        MKT_TRY(d_peaks.alloc(nen));
        hipLaunchKernelGGL(k_lp_gather, dim3(grid_for(nen, LPWG)), dim3(LPWG), 0, st, (const uint32_t*)d_list, nen, in.b1, in.b2, in.cnt, (const uint8_t*)s.window, (const double*)s.r, d_peaks);
        MKT_TRY(hipGetLastError());
        MKT_TRY(hipMemcpyAsync(pk.data(), d_peaks, (size_t)nen * sizeof(LpPeak), hipMemcpyDeviceToHost, st));
        MKT_TRY(hipStreamSynchronize(st));
    }
    s.loops.clear();
    lp_cluster(cell, pk, off, in.nbins, opts.cluster_radius, s.loops);
    s.info.cells = nnz; s.info.candidates = hc[0]; s.info.tested = hc[1]; s.info.undefined = hc[2]; s.info.over = hc[3];
    s.info.grew = hc[4]; s.info.at_max = hc[5]; s.info.enriched = nen; s.info.loops = s.loops.size();
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points (comparisons and copies only: nothing here rounds) ------------------------------------------------------------
using namespace mkt;
extern "C" {

void mkt_loops_opts_default(mkt_loops_opts* o) {
    if (!o) return;
    o->peak = 2; o->window = 5; o->window_max = 20; o->min_ll_count = 16; o->min_dist = 8; o->max_dist = 0; o->fdr = 0.1; o->cluster_radius = 2; o->reserved = 0;
}

int mkt_matrix_loops(mkt_matrix* m, uint32_t res_index, const mkt_loops_opts* opts, mkt_loops_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    const mkt_loops_opts o = mx_opts(opts, mkt_loops_opts_default);
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
    MX_OR_RESET(m, "loops: ", r.lps, layout_rows(r.lay, mx_cells(r), st));   // the row pointers are all the pass needs
    LoopsIn in;
    in.b1 = r.d_b1; in.b2 = r.d_b2; in.cnt = r.d_cnt; in.rowptr = r.lay.rowptr; in.off = r.d_off; in.chr = r.lay.chr;
    in.w = r.ext.use_weights ? r.d_w.get() : nullptr; in.E = r.ext.d_cis_sm;
    in.nnz = r.nnz; in.nbins = r.nbins; in.genome_rows = r.exs.genome_rows; in.nchr = (uint32_t)r.off.size();
    MX_OR_RESET(m, "loops: ", r.lps, loops_run(r.lps, in, r.off, o, st));
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
    if (hist) memcpy(hist, rp->lps.hist.data(), rp->lps.hist.size() * 8);
    return MKT_OK;
}
int mkt_matrix_fetch_loop_thresholds(mkt_matrix* m, uint32_t res_index, uint32_t* thresholds) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp, MX_LOOPS);
    if (thresholds) memcpy(thresholds, rp->lps.thr.data(), rp->lps.thr.size() * 4);
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
    mx_ms(pass_ms, have, s.pass_ms); mx_ms(hist_ms, have, s.hist_ms); mx_ms(flag_ms, have, s.flag_ms);
    return MKT_OK;
}

}  // extern "C"
