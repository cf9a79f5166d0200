// mkt_saddle.hip -- the saddle tables of one resolution's binned contact matrix on the GPU (the sum of observed / expected over the
// cells of every pair of groups of bins ranked by a track), and the groups, the positions and the compartment strength formed on the
// host; include/mkt.h has the definition; the entry points (mkt_matrix_saddle, mkt_matrix_fetch_saddle*) are at the end (mkt_matrix_obj.h).
//
// The sweep.  One workgroup owns one CHUNK of 4096 cells in stored order and keeps the chunk's table T_c in LDS, one double per unordered
// pair of groups (a <= b; Q (Q + 1) / 2 of them).  The chunk is walked in pieces of 1024 cells.  Per piece every thread first works out,
// for four cells, the entry (a, b) and the value x = v / E (or "not used") and leaves both in LDS.  Then the waves go through the piece in
// ascending cell index: wave w takes the cells whose row group a has a % 4 == w, found 64 cells at a time with one ballot, and for each
// of them lane b alone adds x to T_c[a][b].  An entry is therefore owned by exactly one lane of one wave, which meets its cells in program
// order: the ascending order of the definition is there without a floating-point atomic.  The exact integers ride on an LDS integer atomic
// per used cell (cells << 48 | counts in one 64-bit word: a chunk holds at most 2^12 cells and 2^44 counts) and go to the totals with one
// global integer atomic per touched entry.  k_saddle_fold then adds T_0, T_1, .. per entry in ascending chunk order, one thread per entry.
//
// Groups (step 1), positions (step 4) and scores (step 6) are host code in this file, which is compiled without floating-point
// contraction (the scores are compared bit for bit with tests/saddledef.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

#pragma clang fp contract(off)

namespace mkt {

constexpr int SAD_WG = 256, SAD_WAVES = SAD_WG / 64, SAD_PIECE = 1024;
constexpr uint16_t SAD_UNUSED = 0xFFFF;
typedef unsigned long long sad_u64;
static_assert(kSaddleChunk % SAD_PIECE == 0 && SAD_PIECE % SAD_WG == 0 && (SAD_WAVES & (SAD_WAVES - 1)) == 0, "a chunk is whole pieces, a piece whole rounds of the workgroup");

struct SadOpts { int Q, U, contact, min_diag, max_diag; };

// the unordered entry (a <= b) in the packed upper triangle of [Q][Q], row-major
__host__ __device__ inline int sad_entry(int a, int b, int Q) { return a * (2 * Q - a + 1) / 2 + (b - a); }
// the row of a trans block in the expected tables (a < b): the formula of the expected section
__device__ inline uint64_t sad_trans_row(uint32_t a, uint32_t b, uint32_t nchr) { return (uint64_t)a * (2ull * nchr - a - 1ull) / 2ull + (b - a - 1u); }

// T[chunk][U]: the chunk's sums; nnz, csum [U]: the totals of the exact integers
__global__ __launch_bounds__(SAD_WG) void k_saddle_chunk(SaddleIn in, SadOpts o, const uint8_t* grp, double* T, sad_u64* nnz, sad_u64* csum) {
    extern __shared__ double sad_lds[];                                           // [U] T_c, then [U] cells << 48 | counts
    __shared__ uint16_t ent[SAD_PIECE];                                           // a << 8 | b of a used cell
    __shared__ double val[SAD_PIECE];
    double* tab = sad_lds;
    sad_u64* ints = reinterpret_cast<sad_u64*>(sad_lds + o.U);
    const int Q = o.Q, U = o.U;
    for (int t = threadIdx.x; t < U; t += SAD_WG) { tab[t] = 0.0; ints[t] = 0; }
    __syncthreads();
    const uint64_t c0 = (uint64_t)blockIdx.x * kSaddleChunk;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int piece = 0; piece < (int)kSaddleChunk / SAD_PIECE; ++piece) {
        const uint64_t p0 = c0 + (uint64_t)piece * SAD_PIECE;
        if (p0 >= in.nnz) break;                                                  // the same for every thread
        for (int s = threadIdx.x; s < SAD_PIECE; s += SAD_WG) {
            const uint64_t k = p0 + (uint64_t)s;
            uint16_t e = SAD_UNUSED;
            double x = 0.0;
            if (k < in.nnz) {
                const uint32_t i = in.b1[k], j = in.b2[k];
                const uint32_t gi = grp[i], gj = grp[j];
                if (gi != kSaddleNone && gj != kSaddleNone) {                     // a bin with a group is a valid bin
                    const uint32_t ci = in.chr[i], cj = in.chr[j], d = j - i;
                    const bool use = o.contact == 0 ? (ci == cj && d >= (uint32_t)o.min_diag && (o.max_diag == 0 || d <= (uint32_t)o.max_diag)) : ci != cj;
                    if (use) {
                        const uint32_t cnt = in.cnt[k];
                        const double wi = in.w ? in.w[i] : 1.0, wj = in.w ? in.w[j] : 1.0;
                        const double div = o.contact == 0 ? in.cis_div[d] : in.tr_div[sad_trans_row(ci, cj, in.nchr)];
                        x = __ddiv_rn(__dmul_rn(__dmul_rn((double)cnt, wi), wj), div);
                        const uint32_t a = gi < gj ? gi : gj, b = gi < gj ? gj : gi;
                        e = (uint16_t)(a << 8 | b);
                        atomicAdd(&ints[sad_entry((int)a, (int)b, Q)], (1ull << 48) | (sad_u64)cnt);
                    }
                }
            }
            ent[s] = e; val[s] = x;
        }
        __syncthreads();
        for (int blk = 0; blk < SAD_PIECE / 64; ++blk) {                          // ascending cell index
            const int e = ent[blk * 64 + lane];
            sad_u64 mask = __ballot(e != SAD_UNUSED && ((e >> 8) & (SAD_WAVES - 1)) == wave);
            while (mask) {
                const int p = __ffsll(mask) - 1;
                mask &= mask - 1;
                const int ee = __builtin_amdgcn_readlane(e, p);
                const int a = ee >> 8, b = ee & 255;
                if (lane == b) {                                                  // the one owner of (a, b)
                    const int at = sad_entry(a, b, Q);
                    tab[at] = __dadd_rn(tab[at], val[blk * 64 + p]);
                }
            }
        }
        __syncthreads();                                                          // the piece's LDS is read no more
    }
    const size_t base = (size_t)blockIdx.x * (size_t)U;
    for (int t = threadIdx.x; t < U; t += SAD_WG) {
        T[base + t] = tab[t];
        const sad_u64 c = ints[t];
        if (c) { atomicAdd(&nnz[t], c >> 48); atomicAdd(&csum[t], c & ((1ull << 48) - 1)); }
    }
}

// vsum = T_0 + T_1 + .. in this order; one thread per entry
__global__ __launch_bounds__(256) void k_saddle_fold(const double* T, uint32_t chunks, int U, double* vsum) {
    const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (u >= U) return;
    double s = 0.0;
    uint32_t c = 0;
    for (; c + 8 <= chunks; c += 8) {                                             // eight loads in flight, the additions in order
        double t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = T[(size_t)(c + k) * (size_t)U + (size_t)u];
#pragma unroll
        for (int k = 0; k < 8; ++k) s = __dadd_rn(s, t[k]);
    }
    for (; c < chunks; ++c) s = __dadd_rn(s, T[(size_t)c * (size_t)U + (size_t)u]);
    vsum[u] = s;
}

// ---------------------------------------------------------------------------------------------------------------
void saddle_groups(const double* track, const double* w, uint64_t nbins, const mkt_saddle_opts& o, SaddleState& s) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const uint64_t Q = (uint64_t)o.n_groups;
    s.group.assign(nbins, kSaddleNone);
    s.g_bins.assign(Q, 0); s.g_lo.assign(Q, nan); s.g_hi.assign(Q, nan);
    std::vector<uint32_t> cand;
    for (uint64_t k = 0; k < nbins; ++k)
        if ((!w || w[k] == w[k]) && track[k] == track[k]) cand.push_back((uint32_t)k);
    // ascending bins to begin with and a stable sort: ties (-0.0 and 0.0 are one) go to the lower bin
    std::stable_sort(cand.begin(), cand.end(), [track](uint32_t a, uint32_t b) { return track[a] < track[b]; });
    const uint64_t T = cand.size(), lo = T * (uint64_t)o.trim_lo / 10000, hi = T * (uint64_t)o.trim_hi / 10000, K = T - hi - lo;
    for (uint64_t r = lo; r < T - hi; ++r) {
        const uint64_t g = (r - lo) * Q / K;
        s.group[cand[r]] = (uint8_t)g;
        if (s.g_bins[g]++ == 0) s.g_lo[g] = track[cand[r]];
        s.g_hi[g] = track[cand[r]];
    }
    s.info.candidates = T; s.info.kept = K;
}

void saddle_positions(const uint8_t* group, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_saddle_opts& o, uint64_t* n) {
    const int Q = o.n_groups;
    std::fill(n, n + (size_t)Q * Q, (uint64_t)0);
    const size_t nchr = off.size();
    if (o.contact == 1) {
        // pairs of bins of two different chromosomes = all pairs of different bins minus those inside one chromosome, per pair of groups
        std::vector<uint64_t> H(Q, 0), h(Q), same((size_t)Q * Q, 0);
        for (size_t c = 0; c < nchr; ++c) {
            std::fill(h.begin(), h.end(), (uint64_t)0);
            const uint64_t e = c + 1 < nchr ? off[c + 1] : nbins;
            for (uint64_t k = off[c]; k < e; ++k) if (group[k] != kSaddleNone) ++h[group[k]];
            for (int a = 0; a < Q; ++a) {
                H[a] += h[a];
                for (int b = a; b < Q; ++b) same[(size_t)a * Q + b] += h[a] * h[b];
            }
        }
        for (int a = 0; a < Q; ++a)
            for (int b = a; b < Q; ++b) {
                const uint64_t x = H[a] * H[b] - same[(size_t)a * Q + b];
                n[(size_t)a * Q + b] = a == b ? x / 2 : x;
            }
        return;
    }
    // cis: for a bin i the bins j in [i + min_diag, i + max_diag] of its chromosome, per group from prefix counts
    std::vector<uint32_t> P;
    for (size_t c = 0; c < nchr; ++c) {
        const uint64_t b0 = off[c], nc = (c + 1 < nchr ? off[c + 1] : nbins) - b0;
        P.assign((size_t)(nc + 1) * Q, 0);                                         // P[k][g]: the bins before local bin k with group g
        for (uint64_t k = 0; k < nc; ++k) {
            for (int g = 0; g < Q; ++g) P[(size_t)(k + 1) * Q + g] = P[(size_t)k * Q + g];
            if (group[b0 + k] != kSaddleNone) ++P[(size_t)(k + 1) * Q + group[b0 + k]];
        }
        for (uint64_t i = 0; i < nc; ++i) {
            const int a = group[b0 + i];
            if (a == kSaddleNone) continue;
            const uint64_t lo = std::min<uint64_t>(i + (uint64_t)o.min_diag, nc), hi = o.max_diag ? std::min<uint64_t>(i + (uint64_t)o.max_diag + 1, nc) : nc;
            if (hi <= lo) continue;
            for (int b = 0; b < Q; ++b) {
                const uint64_t x = P[(size_t)hi * Q + b] - P[(size_t)lo * Q + b];
                n[(size_t)(a < b ? a : b) * Q + (a < b ? b : a)] += x;
            }
        }
    }
}

// x / y; a zero denominator and every NaN give the one quiet NaN (the scores are compared as bytes)
static double sad_q(double x, double y) {
    const double r = y == 0.0 ? std::numeric_limits<double>::quiet_NaN() : x / y;
    return r != r ? std::numeric_limits<double>::quiet_NaN() : r;
}

void saddle_scores(const double* vsum, const uint64_t* n, int Q, int corner, SaddleState& s) {
    const int half = Q / 2;
    s.strength.assign(half, 0.0); s.aa_ab.assign(half, 0.0); s.bb_ab.assign(half, 0.0);
    for (int k = 1; k <= half; ++k) {
        double bbs = 0.0, aas = 0.0, abs_ = 0.0;
        uint64_t bbn = 0, aan = 0, abn = 0;
        for (int a = 0; a < Q; ++a)
            for (int b = a; b < Q; ++b) {                                         // ascending (a, b), row-major
                const double v = vsum[(size_t)a * Q + b];
                const uint64_t c = n[(size_t)a * Q + b];
                if (b < k) { bbs += v; bbn += c; }
                if (a >= Q - k) { aas += v; aan += c; }
                if (a < k && b >= Q - k) { abs_ += v; abn += c; }
            }
        const double ab = sad_q(abs_, (double)abn);
        s.strength[k - 1] = sad_q(sad_q(bbs + aas, (double)(bbn + aan)), ab);
        s.aa_ab[k - 1] = sad_q(sad_q(aas, (double)aan), ab);
        s.bb_ab[k - 1] = sad_q(sad_q(bbs, (double)bbn), ab);
    }
    s.info.strength = s.strength[corner - 1]; s.info.aa_ab = s.aa_ab[corner - 1]; s.info.bb_ab = s.bb_ab[corner - 1];
}

hipError_t saddle_run(SaddleState& s, const SaddleIn& in, const std::vector<uint32_t>& off, const double* track, const mkt_saddle_opts& opts, hipStream_t st) {
    if (in.nbins >= (1ull << 32) || in.nnz >= (1ull << 32)) return hipErrorInvalidValue;
    const int Q = opts.n_groups, U = Q * (Q + 1) / 2;
    const size_t Q2 = (size_t)Q * Q;
    SadOpts o;
    o.Q = Q; o.U = U; o.contact = opts.contact; o.min_diag = opts.min_diag; o.max_diag = opts.max_diag;
    const uint64_t chunks = (in.nnz + kSaddleChunk - 1) / kSaddleChunk;
    memset(&s.info, 0, sizeof s.info);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> w_host;                                                   // valid(k) of step 1 is read on the host
    if (in.w && in.nbins) {
        w_host.resize(in.nbins);
        MKT_TRY(hipMemcpyAsync(w_host.data(), in.w, (size_t)in.nbins * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipStreamSynchronize(st));
    }
    saddle_groups(track, in.w ? w_host.data() : nullptr, in.nbins, opts, s);
    std::vector<uint64_t> un(Q2);
    saddle_positions(s.group.data(), off, in.nbins, opts, un.data());
    DevEvents<2> ev;
    MKT_TRY(ev.create());
    DevBuf<uint8_t> d_grp;
    DevBuf<double> d_T, d_vs;
    DevBuf<sad_u64> d_nnz, d_cs;
    MKT_TRY(d_grp.alloc(in.nbins, 64));
    MKT_TRY(d_T.alloc(chunks * (size_t)U, 64));                                   // every chunk's table at once
    MKT_TRY(d_vs.alloc(U)); MKT_TRY(d_nnz.alloc(U)); MKT_TRY(d_cs.alloc(U));
    if (in.nbins) MKT_TRY(hipMemcpyAsync(d_grp, s.group.data(), (size_t)in.nbins, hipMemcpyHostToDevice, st));
    MKT_TRY(hipMemsetAsync(d_nnz, 0, (size_t)U * 8, st)); MKT_TRY(hipMemsetAsync(d_cs, 0, (size_t)U * 8, st));
    MKT_TRY(hipStreamSynchronize(st));
    s.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    MKT_TRY(hipEventRecord(ev[0], st));
    if (chunks) hipLaunchKernelGGL(k_saddle_chunk, dim3((unsigned)chunks), dim3(SAD_WG), (size_t)U * 16, st, in, o, (const uint8_t*)d_grp.get(), d_T.get(), d_nnz.get(), d_cs.get());
    hipLaunchKernelGGL(k_saddle_fold, dim3(grid_for((uint64_t)U, 256)), dim3(256), 0, st, (const double*)d_T.get(), (uint32_t)chunks, U, d_vs.get());
    MKT_TRY(hipEventRecord(ev[1], st));
    MKT_TRY(hipGetLastError());
    std::vector<uint64_t> unnz(U), ucs(U);
    std::vector<double> uvs(U);
    MKT_TRY(hipMemcpyAsync(unnz.data(), d_nnz, (size_t)U * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(ucs.data(), d_cs, (size_t)U * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(uvs.data(), d_vs, (size_t)U * 8, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    s.sweep_ms = ms;
    s.n.assign(Q2, 0); s.nnz.assign(Q2, 0); s.csum.assign(Q2, 0); s.vsum.assign(Q2, 0.0); s.mean.assign(Q2, 0.0);
    uint64_t used = 0;
    for (int a = 0; a < Q; ++a)
        for (int b = a; b < Q; ++b) {
            const size_t u = (size_t)sad_entry(a, b, Q), x = (size_t)a * Q + b, y = (size_t)b * Q + a;
            s.n[x] = s.n[y] = un[x]; s.nnz[x] = s.nnz[y] = unnz[u]; s.csum[x] = s.csum[y] = ucs[u]; s.vsum[x] = s.vsum[y] = uvs[u];
            s.mean[x] = s.mean[y] = un[x] ? uvs[u] / (double)un[x] : std::numeric_limits<double>::quiet_NaN();
            used += unnz[u];
        }
    s.info.n_groups = (uint32_t)Q; s.info.cells_used = used; s.info.chunks = (uint32_t)chunks;
    s.info.corner = (uint32_t)(opts.corner ? opts.corner : std::max(1, Q / 5));
    saddle_scores(s.vsum.data(), s.n.data(), Q, (int)s.info.corner, s);
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points (comparisons and copies only: nothing here rounds) ------------------------------------------------------------
using namespace mkt;
extern "C" {

void mkt_saddle_opts_default(mkt_saddle_opts* o) {
    if (!o) return;
    o->n_groups = 50; o->trim_lo = 250; o->trim_hi = 250; o->contact = 0; o->kind = MKT_VALUE_OE; o->min_diag = 2; o->max_diag = 0; o->corner = 0; o->reserved = 0;
}

int mkt_matrix_saddle(mkt_matrix* m, uint32_t res_index, const mkt_saddle_opts* opts, const double* track, mkt_saddle_info* info) {
    if (m && info) memset(info, 0, sizeof *info);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    const mkt_saddle_opts o = mx_opts(opts, mkt_saddle_opts_default);
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
    if (const int rc = mx_cells32(m, "saddle", r.nnz)) return rc;
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
    mx_ms(setup_ms, have, s.setup_ms); mx_ms(sweep_ms, have, s.sweep_ms);
    return MKT_OK;
}

}  // extern "C"
