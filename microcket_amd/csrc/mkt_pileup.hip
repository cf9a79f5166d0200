// mkt_pileup.hip -- the pileup of one resolution's binned contact matrix around a list of features on the GPU, and the scores formed
// from it on the host; include/mkt.h has the definition; the entry points (mkt_matrix_pileup, .._fetch_pileup) are at the end (mkt_matrix_obj.h).
//
// The sweep.  One workgroup owns one CHUNK of 256 features, and inside it one thread owns a position (p, q) of the window (a thread
// takes the positions t, t + threads, ..), so a position's values are added by one thread in ascending feature index and no sum is
// ever shared: no barrier orders an addition.  The chunk is walked in pieces of 32 features.  Per piece the threads first find, for
// every (feature, row p), where the columns max(b - flank, i) .. of row i = a + p start among the (bin1, bin2)-sorted cells: one binary
// search between the row pointers, kept in LDS.  A position (p, q) with j >= i then looks for its cell in at most q + 1 cells behind
// that start (columns are distinct and ascending, so column j cannot lie further); a mirrored position (j < i: features nearer to the
// diagonal than the window is wide) searches row j for column i on its own.  The partial sums T_c of the chunk live in global memory
// between pieces, read and written by their one owner.  k_pile_fold then adds the chunks' partial sums to the running totals in
// ascending chunk order, one thread per position; the totals carry over from one batch of 4096 chunks to the next, so the bits do not
// depend on the batch.
//
// Statuses (step 1) and scores (step 6) are host code in this file, which is compiled without floating-point contraction (the scores
// are compared bit for bit with tests/piledef.py).
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

constexpr int PILE_SUB = 32;                                  // features of one piece
constexpr int PILE_SIDE_MAX = 2 * kPileFlankMax + 1;
typedef unsigned long long pile_u64;

struct PileOpts { int flank, S, S2, kind, ig; };
struct PilePart { double* v; pile_u64* c; uint32_t* n; };     // [chunks][S2] partial sums of a batch

// fa, fb, fst: the features of this batch; chunk blockIdx.x holds the features [256 blockIdx.x, +256) of them
__global__ __launch_bounds__(256) void k_pile_chunk(PileIn in, PileOpts o, const uint32_t* fa, const uint32_t* fb, const uint8_t* fst, uint64_t nfeat, PilePart T) {
    __shared__ int64_t f_a[PILE_SUB], f_b[PILE_SUB], f_lo[PILE_SUB], f_hi[PILE_SUB];      // f_a < 0: the feature is not used
    __shared__ uint32_t rs[PILE_SUB * PILE_SIDE_MAX], re[PILE_SUB * PILE_SIDE_MAX];       // per (feature, row p): first cell at a column >= max(b - flank, i), end of the row
    const int S = o.S, F = o.flank;
    const uint64_t f0 = (uint64_t)blockIdx.x * kPileChunk;
    const size_t base = (size_t)blockIdx.x * (size_t)o.S2;
    for (int sub = 0; sub < (int)kPileChunk / PILE_SUB; ++sub) {
        const uint64_t g0 = f0 + (uint64_t)sub * PILE_SUB;
        if (sub && g0 >= nfeat) break;                                            // the same for every thread
        if (threadIdx.x < PILE_SUB) {
            const uint64_t g = g0 + threadIdx.x;
            int64_t a = -1, b = 0, lo = 0, hi = 0;
            if (g < nfeat && fst[g] == MKT_PILE_USED) {
                a = fa[g]; b = fb[g];
                const uint32_t c = in.chr[a];
                lo = in.off[c]; hi = c + 1u < in.nchr ? (int64_t)in.off[c + 1u] : (int64_t)in.nbins;
            }
            f_a[threadIdx.x] = a; f_b[threadIdx.x] = b; f_lo[threadIdx.x] = lo; f_hi[threadIdx.x] = hi;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < PILE_SUB * S; t += blockDim.x) {
            const int k = t / S;
            const int64_t a = f_a[k], i = a + (t - k * S) - F;
            uint32_t s = 0, e = 0;
            if (a >= 0 && i >= f_lo[k] && i < f_hi[k]) {
                const int64_t jlo = f_b[k] - F > i ? f_b[k] - F : i;
                e = in.rowptr[i + 1];
                s = seg_lower_bound(in.b2, in.rowptr[i], e, jlo);
            }
            rs[t] = s; re[t] = e;
        }
        __syncthreads();
        for (int pos = threadIdx.x; pos < o.S2; pos += blockDim.x) {
            const int pi = pos / S, p = pi - F, q = pos - pi * S - F;
            double v = sub ? T.v[base + pos] : 0.0;
            pile_u64 cs = sub ? T.c[base + pos] : 0;
            uint32_t n = sub ? T.n[base + pos] : 0;
            for (int k = 0; k < PILE_SUB; ++k) {                                  // ascending feature index
                const int64_t a = f_a[k];
                if (a < 0) continue;
                const int64_t b = f_b[k], lo = f_lo[k], hi = f_hi[k], i = a + p, j = b + q;
                if (i < lo || i >= hi || j < lo || j >= hi) continue;
                const int64_t x = i < j ? i : j, y = i < j ? j : i, d = y - x;    // the cell looked up is (x, y)
                if (d < o.ig) continue;
                double wx = 1.0, wy = 1.0;
                if (in.w) { wx = in.w[x]; wy = in.w[y]; if (wx != wx || wy != wy) continue; }
                ++n;                                                              // a kept position, with or without a cell
                uint32_t s, e;
                if (j >= i) {
                    const int64_t jlo = b - F > i ? b - F : i;
                    const uint32_t s0 = rs[k * S + pi], e0 = re[k * S + pi];
                    const uint64_t far = (uint64_t)s0 + (uint64_t)(j - jlo) + 1u;
                    e = far < e0 ? (uint32_t)far : e0;
                    s = seg_lower_bound(in.b2, s0, e, y);
                } else {
                    e = in.rowptr[x + 1];
                    s = seg_lower_bound(in.b2, in.rowptr[x], e, y);
                }
                if (s >= e || (int64_t)in.b2[s] != y) continue;
                const uint32_t cnt = in.cnt[s];
                double val = __dmul_rn(__dmul_rn((double)cnt, wx), wy);
                if (o.kind != MKT_VALUE_BALANCED) val = __ddiv_rn(val, in.E[d]);
                v = __dadd_rn(v, val);
                cs += cnt;
            }
            T.v[base + pos] = v; T.c[base + pos] = cs; T.n[base + pos] = n;
        }
        __syncthreads();                                                          // the piece's LDS is read no more
    }
}

// totals += T_0, T_1, .. in this order; one thread per position
__global__ __launch_bounds__(256) void k_pile_fold(PilePart T, uint32_t chunks, int S2, double* v, pile_u64* c, pile_u64* n) {
    const int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pos >= S2) return;
    double sv = v[pos];
    pile_u64 sc = c[pos], sn = n[pos];
    for (uint32_t k = 0; k < chunks; ++k) {
        const size_t at = (size_t)k * (size_t)S2 + (size_t)pos;
        sv = __dadd_rn(sv, T.v[at]); sc += T.c[at]; sn += T.n[at];
    }
    v[pos] = sv; c[pos] = sc; n[pos] = sn;
}

// ---------------------------------------------------------------------------------------------------------------
bool pileup_status(const uint32_t* a, const uint32_t* b, uint64_t n, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_pileup_opts& o,
                   std::vector<uint8_t>& status, std::string& why) {
    status.assign(n, 0);
    char msg[200];
    for (uint64_t f = 0; f < n; ++f) {
        const uint64_t x = a[f], y = b[f];
        if (x > y) { snprintf(msg, sizeof msg, "pileup: feature %llu (%u, %u): bin1 is larger than bin2", (unsigned long long)f, a[f], b[f]); why = msg; return false; }
        if (y >= nbins) { snprintf(msg, sizeof msg, "pileup: feature %llu (%u, %u): a bin past the last of %llu", (unsigned long long)f, a[f], b[f], (unsigned long long)nbins); why = msg; return false; }
        const size_t cx = (size_t)(std::upper_bound(off.begin(), off.end(), (uint32_t)x) - off.begin()) - 1;
        const size_t cy = (size_t)(std::upper_bound(off.begin(), off.end(), (uint32_t)y) - off.begin()) - 1;
        const int64_t lo = off[cx], hi = cx + 1 < off.size() ? (int64_t)off[cx + 1] : (int64_t)nbins, d = (int64_t)(y - x);
        uint8_t st = MKT_PILE_USED;
        if (cx != cy) st = MKT_PILE_TRANS;
        else if (d < o.min_dist || (o.max_dist && d > o.max_dist)) st = MKT_PILE_DIST;
        else if (!o.edges && ((int64_t)x - o.flank < lo || (int64_t)y + o.flank >= hi)) st = MKT_PILE_EDGE;      // x <= y: these two are the outermost bins
        status[f] = st;
    }
    return true;
}

// the finite values of mean over rows [p0, p1] x columns [q0, q1] (indices into [S][S]) without (skip, skip), in ascending (p, q): their
// mean and, for sd, the root of the sum of squared deviations over k - 1
static double pile_box(const double* mean, int S, int p0, int p1, int q0, int q1, int skip, double* sd) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double sum = 0.0;
    uint64_t k = 0;
    for (int p = p0; p <= p1; ++p)
        for (int q = q0; q <= q1; ++q) {
            if (p == skip && q == skip) continue;
            const double x = mean[p * S + q];
            if (std::isfinite(x)) { sum += x; ++k; }
        }
    const double mu = k ? sum / (double)k : nan;
    if (sd) {
        double ss = 0.0;
        for (int p = p0; p <= p1; ++p)
            for (int q = q0; q <= q1; ++q) {
                const double x = mean[p * S + q];
                if (std::isfinite(x)) { const double dx = x - mu; ss += dx * dx; }
            }
        *sd = k >= 2 ? std::sqrt(ss / (double)(k - 1)) : nan;
    }
    return mu;
}

// a quotient as IEEE gives it; every NaN is the one quiet NaN (the scores are compared as bytes)
static double pile_q(double x) { return x != x ? std::numeric_limits<double>::quiet_NaN() : x; }

void pileup_scores(const double* mean, int flank, int corner, mkt_pileup_info& info) {
    const int S = 2 * flank + 1, lo1 = corner - 1, hi0 = S - corner, hi1 = S - 1;      // low box indices [0, lo1], high [hi0, hi1]
    double sd = 0;
    const double peak = mean[flank * S + flank];
    const double ll = pile_box(mean, S, hi0, hi1, 0, lo1, -1, &sd);
    info.peak = pile_q(peak);
    info.p2ll = pile_q(peak / ll);
    info.p2ul = pile_q(peak / pile_box(mean, S, 0, lo1, 0, lo1, -1, nullptr));
    info.p2ur = pile_q(peak / pile_box(mean, S, 0, lo1, hi0, hi1, -1, nullptr));
    info.p2lr = pile_q(peak / pile_box(mean, S, hi0, hi1, hi0, hi1, -1, nullptr));
    info.p2m = pile_q(peak / pile_box(mean, S, 0, hi1, 0, hi1, flank, nullptr));
    info.z_ll = pile_q(pile_q(peak - ll) / sd);
}

hipError_t pileup_run(PileState& s, const PileIn& in, const uint32_t* a, const uint32_t* b, uint64_t n, const mkt_pileup_opts& opts, hipStream_t st) {
    if (in.nbins >= (1ull << 32) || in.nnz >= (1ull << 32) || n >= (1ull << 32) || s.status.size() != n) return hipErrorInvalidValue;
    PileOpts o;
    o.flank = opts.flank; o.S = 2 * opts.flank + 1; o.S2 = o.S * o.S; o.kind = opts.kind; o.ig = opts.ignore_diags;
    const size_t S2 = (size_t)o.S2;
    const uint64_t chunks = (n + kPileChunk - 1) / kPileChunk;
    const uint64_t bchunks = chunks < kPileBatchChunks ? chunks : kPileBatchChunks;           // chunks of the largest batch
    const uint64_t bfeat = bchunks * kPileChunk < n ? bchunks * kPileChunk : n;
    DevEvents<3> ev;
    MKT_TRY(ev.create());
    DevBuf<uint32_t> d_a, d_b, d_pn;
    DevBuf<uint8_t> d_st;
    DevBuf<double> d_pv, d_v;
    DevBuf<pile_u64> d_pc, d_c, d_n;
    MKT_TRY(d_a.alloc(bfeat, 64)); MKT_TRY(d_b.alloc(bfeat, 64)); MKT_TRY(d_st.alloc(bfeat, 64));
    MKT_TRY(d_pv.alloc(bchunks * S2, 64)); MKT_TRY(d_pc.alloc(bchunks * S2, 64)); MKT_TRY(d_pn.alloc(bchunks * S2, 64));
    MKT_TRY(d_v.alloc(S2)); MKT_TRY(d_c.alloc(S2)); MKT_TRY(d_n.alloc(S2));
    MKT_TRY(hipMemsetAsync(d_v, 0, S2 * 8, st)); MKT_TRY(hipMemsetAsync(d_c, 0, S2 * 8, st)); MKT_TRY(hipMemsetAsync(d_n, 0, S2 * 8, st));
    PilePart T;
    T.v = d_pv; T.c = d_pc; T.n = d_pn;
    const unsigned wg = o.S2 <= 64 ? 64u : o.S2 <= 128 ? 128u : 256u;                         // a small window leaves room for more chunks per CU
    s.setup_ms = s.sweep_ms = 0;
    for (uint64_t c0 = 0; c0 < chunks; c0 += kPileBatchChunks) {
        const uint64_t f0 = c0 * kPileChunk, nc = chunks - c0 < kPileBatchChunks ? chunks - c0 : kPileBatchChunks;
        const uint64_t nf = n - f0 < nc * kPileChunk ? n - f0 : nc * kPileChunk;
        MKT_TRY(hipEventRecord(ev[0], st));
        MKT_TRY(hipMemcpyAsync(d_a, a + f0, (size_t)nf * 4, hipMemcpyHostToDevice, st));
        MKT_TRY(hipMemcpyAsync(d_b, b + f0, (size_t)nf * 4, hipMemcpyHostToDevice, st));
        MKT_TRY(hipMemcpyAsync(d_st, s.status.data() + f0, (size_t)nf, hipMemcpyHostToDevice, st));
        MKT_TRY(hipEventRecord(ev[1], st));
        hipLaunchKernelGGL(k_pile_chunk, dim3((unsigned)nc), dim3(wg), 0, st, in, o, (const uint32_t*)d_a.get(), (const uint32_t*)d_b.get(), (const uint8_t*)d_st.get(), nf, T);
        hipLaunchKernelGGL(k_pile_fold, dim3(grid_for(S2, 256)), dim3(256), 0, st, T, (uint32_t)nc, o.S2, d_v.get(), d_c.get(), d_n.get());
        MKT_TRY(hipEventRecord(ev[2], st));
        MKT_TRY(hipGetLastError());
        MKT_TRY(hipStreamSynchronize(st));                                                    // the batch's features are read no more
        float ms = 0;
        MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); s.setup_ms += ms;
        MKT_TRY(hipEventElapsedTime(&ms, ev[1], ev[2])); s.sweep_ms += ms;
    }
    s.n.assign(S2, 0); s.csum.assign(S2, 0); s.vsum.assign(S2, 0.0); s.mean.assign(S2, 0.0);
    MKT_TRY(hipMemcpyAsync(s.n.data(), d_n, S2 * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(s.csum.data(), d_c, S2 * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(s.vsum.data(), d_v, S2 * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    for (size_t k = 0; k < S2; ++k) s.mean[k] = s.n[k] ? s.vsum[k] / (double)s.n[k] : std::numeric_limits<double>::quiet_NaN();
    memset(&s.info, 0, sizeof s.info);
    s.info.features = n; s.info.side = (uint32_t)o.S; s.info.chunks = (uint32_t)chunks;
    for (uint8_t x : s.status) {
        if (x == MKT_PILE_USED) ++s.info.used; else if (x == MKT_PILE_TRANS) ++s.info.trans; else if (x == MKT_PILE_EDGE) ++s.info.edge; else ++s.info.dist;
    }
    pileup_scores(s.mean.data(), opts.flank, opts.corner, s.info);
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points (comparisons and copies only: nothing here rounds) ------------------------------------------------------------
using namespace mkt;
extern "C" {

void mkt_pileup_opts_default(mkt_pileup_opts* o) {
    if (!o) return;
    o->flank = 10; o->corner = 6; o->kind = MKT_VALUE_OE_SMOOTH; o->ignore_diags = 2; o->edges = 0; o->min_dist = 0; o->max_dist = 0; o->reserved = 0;
}

int mkt_matrix_pileup(mkt_matrix* m, uint32_t res_index, const uint32_t* bin1, const uint32_t* bin2, uint64_t n, const mkt_pileup_opts* opts, mkt_pileup_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    const mkt_pileup_opts o = mx_opts(opts, mkt_pileup_opts_default);
    if (o.flank < 1 || o.flank > kPileFlankMax) return mfail(m, MKT_E_ARG, "pileup: flank %d is outside 1 .. %d", o.flank, kPileFlankMax);
    if (o.corner < 1 || o.corner > o.flank) return mfail(m, MKT_E_ARG, "pileup: corner %d is outside 1 .. flank %d", o.corner, o.flank);
    if (const int rc = mx_kind(m, "pileup", o.kind)) return rc;
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "pileup: ignore_diags %d is negative", o.ignore_diags);
    if (o.edges != 0 && o.edges != 1) return mfail(m, MKT_E_ARG, "pileup: edges %d (0 or 1)", o.edges);
    if (o.min_dist < 0 || o.max_dist < 0) return mfail(m, MKT_E_ARG, "pileup: min_dist %d / max_dist %d is negative", o.min_dist, o.max_dist);
    if (o.max_dist && o.max_dist < o.min_dist) return mfail(m, MKT_E_ARG, "pileup: max_dist %d is below min_dist %d", o.max_dist, o.min_dist);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "pileup: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN | MX_TABLES, "pileup")) return rc;
    if (n && (!bin1 || !bin2)) return mfail(m, MKT_E_ARG, "pileup: %llu features without their bins (bin1 or bin2 is NULL)", (unsigned long long)n);
    if (n >= (1ull << 32)) return mfail(m, MKT_E_CAPACITY, "pileup: %llu features: fewer than 2^32 are needed", (unsigned long long)n);
    if (const int rc = mx_cells32(m, "pileup", r.nnz)) return rc;
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
    mx_ms(setup_ms, have, s.setup_ms); mx_ms(sweep_ms, have, s.sweep_ms);
    return MKT_OK;
}

}  // extern "C"
