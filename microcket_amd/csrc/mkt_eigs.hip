// mkt_eigs.hip -- compartment eigenvectors: the leading eigenpairs of every chromosome's cis observed / expected - 1 matrix on the
// GPU; include/mkt.h has the definition; the entry points (mkt_matrix_eigs, .._eigs_apply, the fetches) are at the end (mkt_matrix_obj.h).
//
// The matrix A = S - (g g^T - B) is never formed.  One sweep Y = A X multiplies a block of 8 columns: bin k's lanes walk its row
// segment of the cells and its column segment of the layout's transposed copy (as the balance sweep does), form oe from the
// count, the two weights and E[d], gather the 64 contiguous bytes X[other bin][0 .. 8) and keep 8 accumulators; the rank-one term
// g (g^T X) comes from the previous reduction and the band term B X from the up to 2 ignore_diags - 1 neighbouring rows of X.
// Cis, good bins and d >= ignore_diags are compares in the walk.
//
// Nothing depends on the order anything ran in.  A row's sums are formed by MxLayout::width lanes with a fixed stride
// and the lane tree; rows of more than kBalLong cells get one workgroup and the workgroup tree.  Per-chromosome dot products (X^T Y, Y^T Y, norms, g^T X) are sums over chunks of kEgChunk bins, four
// interleaved slices per chunk added in slice order, then the chunks of a chromosome in chunk order.  The 8 x 8 Rayleigh-Ritz step and
// the Cholesky factor that re-orthonormalises the block run on the host, per chromosome, between two launches: two looks at the
// device per iteration (DESIGN.md 7e has what that costs).  A chromosome that is done is skipped by every kernel through done[c].
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

namespace mkt {

constexpr int EGWG = 256;
constexpr int EG_T = 136;                         // per chromosome: S[8][8], theta[8], T2[8][8]
constexpr int EG_HM = 128, EG_NR = 24;            // sums per chromosome: H and M; |R_j|^2, |V_j|^2 and g^T X

struct EgArgs {
    const uint32_t *rowptr, *colptr, *b2, *cnt, *off, *done;
    const uint2* tr;
    const uint8_t* act;                           // good bins of the chromosomes that are not skipped
    const uint16_t* chr;
    const double *w, *E, *X, *gx;                 // gx: g^T X of chromosome c at gx[c * EG_NR + 16 ..]
    double* Y;
    uint64_t nbins;
    uint32_t nchr, ig;
    double clip;
};

__device__ inline void eg_axpy(double (&acc)[8], double f, const double* row) {
    const double2* p = (const double2*)row;                              // one 64-byte row of X
    const double2 a = p[0], b = p[1], c = p[2], d = p[3];
    acc[0] += f * a.x; acc[1] += f * a.y; acc[2] += f * b.x; acc[3] += f * b.y;
    acc[4] += f * c.x; acc[5] += f * c.y; acc[6] += f * d.x; acc[7] += f * d.y;
}
__device__ inline double eg_oe(double v, double e, double clip) {
    const double oe = v / e;
    return clip > 0.0 && oe > clip ? clip : oe;
}
// lane `l` of `W` walks elements l, l + W, ... of bin k's row segment and then of its column segment; [lo, hi): k's chromosome.
// The diagonal cell is in both segments: the column walk leaves it out.
template <bool HASW>
__device__ inline void eg_walk(const EgArgs& a, uint32_t k, uint32_t l, uint32_t W, uint32_t lo, uint32_t hi, double (&acc)[8]) {
    const uint32_t r0 = a.rowptr[k], r1 = a.rowptr[k + 1], c0 = a.colptr[k], c1 = a.colptr[k + 1];
    const uint32_t igc = a.ig > 1u ? a.ig : 1u;
    const double wk = HASW ? a.w[k] : 1.0;
    for (uint32_t s = r0 + l; s < r1; s += W) {
        const uint32_t o = a.b2[s];                                      // o >= k
        if (o < hi && o - k >= a.ig && a.act[o]) {
            double v = (double)a.cnt[s];
            if (HASW) v = __dmul_rn(__dmul_rn(v, wk), a.w[o]);
            eg_axpy(acc, eg_oe(v, a.E[o - k], a.clip), a.X + 8 * (size_t)o);
        }
    }
    for (uint32_t s = c0 + l; s < c1; s += W) {
        const uint2 t = a.tr[s];                                         // t.x <= k
        if (t.x >= lo && k - t.x >= igc && a.act[t.x]) {
            double v = (double)t.y;
            if (HASW) v = __dmul_rn(__dmul_rn(v, a.w[t.x]), wk);
            eg_axpy(acc, eg_oe(v, a.E[k - t.x], a.clip), a.X + 8 * (size_t)t.x);
        }
    }
}
// the row's result from its sum: - g (g^T X) and the band term, rows max(lo, k - ig + 1) .. min(hi - 1, k + ig - 1) in ascending order
__device__ inline void eg_finish(const EgArgs& a, uint32_t k, uint32_t c, uint32_t lo, uint32_t hi, const double (&acc)[8]) {
    double2* y = (double2*)(a.Y + 8 * (size_t)k);
    if (!a.act[k]) { y[0] = y[1] = y[2] = y[3] = make_double2(0.0, 0.0); return; }
    double band[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.ig > 0u) {
        const uint64_t j0 = (uint64_t)(k - lo) >= (uint64_t)(a.ig - 1u) ? (uint64_t)k - (a.ig - 1u) : lo;
        const uint64_t j1 = (uint64_t)k + (a.ig - 1u) < (uint64_t)hi ? (uint64_t)k + (a.ig - 1u) : (uint64_t)hi - 1u;
        for (uint64_t j = j0; j <= j1; ++j)
            if (a.act[j]) eg_axpy(band, 1.0, a.X + 8 * j);
    }
    const double* g = a.gx + (size_t)c * EG_NR + 16;
    y[0] = make_double2((acc[0] - g[0]) + band[0], (acc[1] - g[1]) + band[1]);
    y[1] = make_double2((acc[2] - g[2]) + band[2], (acc[3] - g[3]) + band[3]);
    y[2] = make_double2((acc[4] - g[4]) + band[4], (acc[5] - g[5]) + band[5]);
    y[3] = make_double2((acc[6] - g[6]) + band[6], (acc[7] - g[7]) + band[7]);
}
// W lanes per bin (W = 8 .. 64, a power of two)
template <bool HASW, int W>
__global__ __launch_bounds__(EGWG) void k_eg_sweep(EgArgs a) {
    const uint64_t k64 = ((uint64_t)blockIdx.x * EGWG + threadIdx.x) / W;
    const uint32_t l = threadIdx.x & (W - 1), k = (uint32_t)k64;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool mine = false;
    uint32_t c = 0, lo = 0, hi = 0;
    if (k64 < a.nbins) {
        c = a.chr[k];
        if (!a.done[c]) {
            mine = (uint64_t)(a.rowptr[k + 1] - a.rowptr[k]) + (a.colptr[k + 1] - a.colptr[k]) <= kBalLong;
            lo = a.off[c];
            hi = c + 1u < a.nchr ? a.off[c + 1] : (uint32_t)a.nbins;
            if (mine && a.act[k]) eg_walk<HASW>(a, k, l, W, lo, hi, acc);
        }
    }
    lane_tree_n<W>(acc);
    if (mine && l == 0) eg_finish(a, k, c, lo, hi, acc);
}
// one workgroup per long bin: the same walk with 256 lanes
template <bool HASW>
__global__ __launch_bounds__(EGWG) void k_eg_sweep_long(EgArgs a, const uint32_t* longbins) {
    __shared__ double sh[EGWG / 64][8];
    const uint32_t k = longbins[blockIdx.x], c = a.chr[k];
    if (a.done[c]) return;
    const uint32_t lo = a.off[c], hi = c + 1u < a.nchr ? a.off[c + 1] : (uint32_t)a.nbins;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.act[k]) eg_walk<HASW>(a, k, threadIdx.x, EGWG, lo, hi, acc);
    wg_tree_n(acc, &sh[0][0]);
    if (threadIdx.x == 0) eg_finish(a, k, c, lo, hi, acc);
}

// good(k): valid and one stored cell to a valid bin of its chromosome at a distance of ignore_diags or more.  One lane per bin; the
// row segment ascends in bin2 and the column segment in bin1, so both walks end early.
__global__ __launch_bounds__(EGWG) void k_eg_good(EgArgs a, uint8_t* good) {
    const uint64_t k64 = (uint64_t)blockIdx.x * EGWG + threadIdx.x;
    if (k64 >= a.nbins) return;
    const uint32_t k = (uint32_t)k64, c = a.chr[k];
    const uint32_t lo = a.off[c], hi = c + 1u < a.nchr ? a.off[c + 1] : (uint32_t)a.nbins;
    bool found = false;
    const bool ok = !a.w || a.w[k] == a.w[k];
    if (ok) {
        for (uint32_t s = a.rowptr[k], e = a.rowptr[k + 1]; s < e && !found; ++s) {
            const uint32_t o = a.b2[s];
            if (o >= hi) break;
            found = o - k >= a.ig && (!a.w || a.w[o] == a.w[o]);
        }
        for (uint32_t s = a.colptr[k], e = a.colptr[k + 1]; s < e && !found; ++s) {
            const uint32_t o = a.tr[s].x;
            if (o < lo) continue;
            if (k - o < a.ig) break;
            found = !a.w || a.w[o] == a.w[o];
        }
    }
    good[k] = found ? 1 : 0;
}

// X_0: a fixed integer hash of (bin - off_c, column) in (-1, 1), zero on the other bins; Y gets a copy (the Gram pass reads both)
__device__ inline double eg_hash(uint32_t i, uint32_t col) {
    uint32_t x = i * 8u + col + 1u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return ((double)x + 0.5) / 2147483648.0 - 1.0;
}
__global__ __launch_bounds__(EGWG) void k_eg_init(EgArgs a, double* X, double* Y) {
    const uint64_t i = (uint64_t)blockIdx.x * EGWG + threadIdx.x;
    if (i >= a.nbins * 8) return;
    const uint32_t k = (uint32_t)(i >> 3), col = (uint32_t)(i & 7);
    const double v = a.act[k] ? eg_hash(k - a.off[a.chr[k]], col) : 0.0;
    X[i] = v; Y[i] = v;
}
// X from the caller's [nbins][ncols]: as given on good bins, 0 elsewhere and in the columns past ncols
__global__ __launch_bounds__(EGWG) void k_eg_load(const uint8_t* act, const double* xin, uint32_t ncols, uint64_t nbins, double* X) {
    const uint64_t i = (uint64_t)blockIdx.x * EGWG + threadIdx.x;
    if (i >= nbins * 8) return;
    const uint64_t k = i >> 3;
    const uint32_t col = (uint32_t)(i & 7);
    X[i] = act[k] && col < ncols ? xin[k * ncols + col] : 0.0;
}
__global__ __launch_bounds__(EGWG) void k_eg_store(const double* Y, uint32_t ncols, uint64_t nbins, double* yout) {
    const uint64_t i = (uint64_t)blockIdx.x * EGWG + threadIdx.x;
    if (i >= nbins * ncols) return;
    yout[i] = Y[(i / ncols) * 8 + i % ncols];
}

// ---- per-chromosome dot products: chunk partials (four interleaved slices, one per wave, added in slice order), then the chunks of a
// chromosome in chunk order.  X and Y are 0 on every bin that is not good, so no flag is read.
// H[a][b] = sum X[.][a] Y[.][b] and M[a][b] = sum Y[.][a] Y[.][b]: lane p of a wave owns the pair (p >> 3, p & 7)
__global__ __launch_bounds__(EGWG) void k_eg_dots(const uint4* chunks, const double* X, const double* Y, const uint32_t* done, double* partial) {
    __shared__ double sh[EGWG / 64][EG_HM];
    const uint4 t = chunks[blockIdx.x];
    if (done[t.x]) return;
    const uint32_t p = threadIdx.x & 63, q = threadIdx.x >> 6, ca = p >> 3, cb = p & 7;
    double h = 0.0, m = 0.0;
    for (uint32_t bin = t.y + q; bin < t.z; bin += EGWG / 64) {
        const double xa = X[8 * (size_t)bin + ca], ya = Y[8 * (size_t)bin + ca], yb = Y[8 * (size_t)bin + cb];
        h += xa * yb; m += ya * yb;
    }
    sh[q][p] = h; sh[q][64 + p] = m;
    __syncthreads();
    if (threadIdx.x < EG_HM) partial[(size_t)blockIdx.x * EG_HM + threadIdx.x] = sum4(sh[0][threadIdx.x], sh[1][threadIdx.x], sh[2][threadIdx.x], sh[3][threadIdx.x]);
}
// lanes 0 .. 7: |R_j|^2 (R is in Y's place), 8 .. 15: |V_j|^2, 16 .. 23: g^T X_j
__global__ __launch_bounds__(EGWG) void k_eg_norms(const uint4* chunks, const double* R, const double* V, const double* X, const uint32_t* done, double* partial) {
    __shared__ double sh[EGWG / 64][EG_NR];
    const uint4 t = chunks[blockIdx.x];
    if (done[t.x]) return;
    const uint32_t p = threadIdx.x & 63, q = threadIdx.x >> 6, col = p & 7;
    if (p < EG_NR) {
        const double* src = p < 8 ? R : p < 16 ? V : X;
        double s = 0.0;
        for (uint32_t bin = t.y + q; bin < t.z; bin += EGWG / 64) { const double v = src[8 * (size_t)bin + col]; s += p < 16 ? v * v : v; }
        sh[q][p] = s;
    }
    __syncthreads();
    if (threadIdx.x < EG_NR) partial[(size_t)blockIdx.x * EG_NR + threadIdx.x] = sum4(sh[0][threadIdx.x], sh[1][threadIdx.x], sh[2][threadIdx.x], sh[3][threadIdx.x]);
}
__global__ __launch_bounds__(EG_HM) void k_eg_chrsum(const uint2* cchunks, const double* partial, const uint32_t* done, uint32_t width, double* out) {
    const uint32_t c = blockIdx.x;
    if (done[c] || threadIdx.x >= width) return;
    const uint2 cc = cchunks[c];
    double s = 0.0;
    for (uint32_t t = 0; t < cc.y; ++t) s += partial[(size_t)(cc.x + t) * width + threadIdx.x];
    out[(size_t)c * width + threadIdx.x] = s;
}

// per bin: V = X S (Ritz vectors), R = Y S - V Theta (into Y's place), the next X = Y T2; one lane per bin, the chromosome's three
// small matrices read by every lane of it
__global__ __launch_bounds__(EGWG) void k_eg_transform(const uint16_t* chr, const uint32_t* done, const double* T, uint64_t nbins, double* X, double* Y, double* V) {
    const uint64_t k = (uint64_t)blockIdx.x * EGWG + threadIdx.x;
    if (k >= nbins) return;
    const uint32_t c = chr[k];
    if (done[c]) return;
    const double *S = T + (size_t)c * EG_T, *th = S + 64, *T2 = S + 72;
    double2 *xp = (double2*)(X + 8 * k), *yp = (double2*)(Y + 8 * k), *vp = (double2*)(V + 8 * k);
    double x[8], y[8], v[8], r[8], n[8];
    { const double2 a = xp[0], b = xp[1], cc = xp[2], d = xp[3]; x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y; x[4] = cc.x; x[5] = cc.y; x[6] = d.x; x[7] = d.y; }
    { const double2 a = yp[0], b = yp[1], cc = yp[2], d = yp[3]; y[0] = a.x; y[1] = a.y; y[2] = b.x; y[3] = b.y; y[4] = cc.x; y[5] = cc.y; y[6] = d.x; y[7] = d.y; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        double vs = 0.0, zs = 0.0, ns = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) { vs += x[i] * S[8 * i + j]; zs += y[i] * S[8 * i + j]; ns += y[i] * T2[8 * i + j]; }
        v[j] = vs; r[j] = zs - vs * th[j]; n[j] = ns;
    }
    vp[0] = make_double2(v[0], v[1]); vp[1] = make_double2(v[2], v[3]); vp[2] = make_double2(v[4], v[5]); vp[3] = make_double2(v[6], v[7]);
    yp[0] = make_double2(r[0], r[1]); yp[1] = make_double2(r[2], r[3]); yp[2] = make_double2(r[4], r[5]); yp[3] = make_double2(r[6], r[7]);
    xp[0] = make_double2(n[0], n[1]); xp[1] = make_double2(n[2], n[3]); xp[2] = make_double2(n[4], n[5]); xp[3] = make_double2(n[6], n[7]);
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------
namespace {

// everything one call holds on the device; freed when it goes out of scope
struct EgWork {
    DevBuf<double> X, Y, V, partial, HM, NR, T, io;
    DevBuf<uint8_t> good, act;
    DevBuf<uint32_t> done;
    DevBuf<uint4> chunks;
    DevBuf<uint2> cchunks;
    uint32_t nchunks = 0;
    std::vector<uint8_t> h_good, h_act;
    std::vector<uint32_t> n_good, h_done;
    EgArgs a;
};

template <bool HASW>
hipError_t eg_launch_sweep(const EigsIn& in, const EgArgs& a, hipStream_t st) {
    if (in.nbins == 0) return hipSuccess;
    const MxLayout& s = *in.lay;
    dispatch_width(s.width, [&](auto W) {
        hipLaunchKernelGGL((k_eg_sweep<HASW, decltype(W)::value>), dim3(grid_for(in.nbins * (uint64_t)s.width, EGWG)), dim3(EGWG), 0, st, a);
    });
    if (s.nlong) hipLaunchKernelGGL((k_eg_sweep_long<HASW>), dim3(s.nlong), dim3(EGWG), 0, st, a, (const uint32_t*)s.longbins);
    return hipGetLastError();
}
hipError_t eg_sweep(const EigsIn& in, const EgArgs& a, hipStream_t st) { return in.w ? eg_launch_sweep<true>(in, a, st) : eg_launch_sweep<false>(in, a, st); }

// g^T X (and the norms of whatever is in Y's and V's place) of every chromosome that is not done, into NR
hipError_t eg_norms(EgWork& k, uint32_t nchr, hipStream_t st) {
    if (k.nchunks) hipLaunchKernelGGL(k_eg_norms, dim3(k.nchunks), dim3(EGWG), 0, st, (const uint4*)k.chunks, (const double*)k.Y, (const double*)k.V, (const double*)k.X, (const uint32_t*)k.done, k.partial);
    hipLaunchKernelGGL(k_eg_chrsum, dim3(nchr), dim3(EG_HM), 0, st, (const uint2*)k.cchunks, (const double*)k.partial, (const uint32_t*)k.done, (uint32_t)EG_NR, k.NR);
    return hipGetLastError();
}
hipError_t eg_dots(EgWork& k, uint32_t nchr, hipStream_t st) {
    if (k.nchunks) hipLaunchKernelGGL(k_eg_dots, dim3(k.nchunks), dim3(EGWG), 0, st, (const uint4*)k.chunks, (const double*)k.X, (const double*)k.Y, (const uint32_t*)k.done, k.partial);
    hipLaunchKernelGGL(k_eg_chrsum, dim3(nchr), dim3(EG_HM), 0, st, (const uint2*)k.cchunks, (const double*)k.partial, (const uint32_t*)k.done, (uint32_t)EG_HM, k.HM);
    return hipGetLastError();
}

// buffers, good flags, n_good, the skipped chromosomes (done from the start) and the chunk tables
hipError_t eg_prepare(EgWork& k, const EigsIn& in, const std::vector<uint32_t>& off, const mkt_eigs_opts& o, hipStream_t st) {
    const uint64_t nb = in.nbins;
    const uint32_t nchr = in.nchr;
    const size_t vbytes = (size_t)nb * 64 + 64;
    MKT_TRY(k.X.alloc(nb * 8, 64)); MKT_TRY(k.Y.alloc(nb * 8, 64)); MKT_TRY(k.V.alloc(nb * 8, 64));
    MKT_TRY(k.good.alloc(nb, 64)); MKT_TRY(k.act.alloc(nb, 64));
    MKT_TRY(k.done.alloc(nchr, 64));
    MKT_TRY(k.HM.alloc((size_t)nchr * EG_HM)); MKT_TRY(k.NR.alloc((size_t)nchr * EG_NR)); MKT_TRY(k.T.alloc((size_t)nchr * EG_T));
    MKT_TRY(hipMemsetAsync(k.X, 0, vbytes, st)); MKT_TRY(hipMemsetAsync(k.Y, 0, vbytes, st)); MKT_TRY(hipMemsetAsync(k.V, 0, vbytes, st));
    MKT_TRY(hipMemsetAsync(k.NR, 0, (size_t)nchr * EG_NR * 8, st)); MKT_TRY(hipMemsetAsync(k.HM, 0, (size_t)nchr * EG_HM * 8, st));
    EgArgs& a = k.a;
    a.rowptr = in.lay->rowptr; a.colptr = in.lay->colptr; a.b2 = in.b2; a.cnt = in.cnt; a.off = in.off; a.done = k.done; a.tr = in.lay->tr;
    a.act = k.act; a.chr = in.lay->chr; a.w = in.w; a.E = in.E; a.X = k.X; a.gx = k.NR; a.Y = k.Y;
    a.nbins = nb; a.nchr = nchr; a.ig = (uint32_t)o.ignore_diags; a.clip = o.clip;
    k.h_good.assign(nb, 0);
    if (nb) {
        hipLaunchKernelGGL(k_eg_good, dim3(grid_for(nb, EGWG)), dim3(EGWG), 0, st, a, k.good);
        MKT_TRY(hipGetLastError());
        MKT_TRY(hipMemcpyAsync(k.h_good.data(), k.good, nb, hipMemcpyDeviceToHost, st));
    }
    MKT_TRY(hipStreamSynchronize(st));
    const uint32_t need = (uint32_t)(o.min_good > 9 ? o.min_good : 9);
    k.n_good.assign(nchr, 0); k.h_done.assign(nchr, 0); k.h_act = k.h_good;
    std::vector<uint4> chunks;
    std::vector<uint2> cc(nchr);
    for (uint32_t c = 0; c < nchr; ++c) {
        const uint64_t lo = off[c], hi = c + 1 < nchr ? off[c + 1] : nb;
        for (uint64_t b = lo; b < hi; ++b) k.n_good[c] += k.h_good[b];
        cc[c] = make_uint2((uint32_t)chunks.size(), 0);
        if (k.n_good[c] < need) {
            k.h_done[c] = 1;
            for (uint64_t b = lo; b < hi; ++b) k.h_act[b] = 0;
            continue;
        }
        for (uint64_t b = lo; b < hi; b += kEgChunk) chunks.push_back(make_uint4(c, (uint32_t)b, (uint32_t)(b + kEgChunk < hi ? b + kEgChunk : hi), 0));
        cc[c].y = (uint32_t)chunks.size() - cc[c].x;
    }
    k.nchunks = (uint32_t)chunks.size();
    MKT_TRY(k.chunks.alloc(k.nchunks + 1));
    MKT_TRY(k.cchunks.alloc(nchr));
    MKT_TRY(k.partial.alloc((size_t)(k.nchunks + 1) * EG_HM));
    if (k.nchunks) MKT_TRY(hipMemcpyAsync(k.chunks, chunks.data(), (size_t)k.nchunks * sizeof(uint4), hipMemcpyHostToDevice, st));
    MKT_TRY(hipMemcpyAsync(k.cchunks, cc.data(), (size_t)nchr * sizeof(uint2), hipMemcpyHostToDevice, st));
    MKT_TRY(hipMemcpyAsync(k.done, k.h_done.data(), (size_t)nchr * 4, hipMemcpyHostToDevice, st));
    if (nb) MKT_TRY(hipMemcpyAsync(k.act, k.h_act.data(), nb, hipMemcpyHostToDevice, st));
    return hipStreamSynchronize(st);                                      // the vectors above are read by the copies
}

// cyclic Jacobi of the symmetric 8 x 8 `a` (destroyed): eigenvalues d, eigenvectors the columns of v; a fixed number of sweeps in a fixed order
void eg_jacobi(double a[8][8], double d[8], double v[8][8]) {
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kEgJacobiSweeps; ++sweep)
        for (int p = 0; p < 7; ++p)
            for (int q = p + 1; q < 8; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0 || apq != apq) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 8; ++k) { const double x = a[k][p], y = a[k][q]; a[k][p] = cs * x - sn * y; a[k][q] = sn * x + cs * y; }
                for (int k = 0; k < 8; ++k) { const double x = a[p][k], y = a[q][k]; a[p][k] = cs * x - sn * y; a[q][k] = sn * x + cs * y; }
                for (int k = 0; k < 8; ++k) { const double x = v[k][p], y = v[k][q]; v[k][p] = cs * x - sn * y; v[k][q] = sn * x + cs * y; }
            }
    for (int i = 0; i < 8; ++i) d[i] = a[i][i];
}
// T2 = S L^-T with G = S^T M S = L L^T (lower Cholesky): (Y S) L^-T has orthonormal columns.  false: G is not positive definite.
bool eg_orth(const double S[8][8], const double M[8][8], double T2[8][8]) {
    double MS[8][8], G[8][8], L[8][8] = {}, Li[8][8] = {};
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { double s = 0.0; for (int k = 0; k < 8; ++k) s += M[i][k] * S[k][j]; MS[i][j] = s; }
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { double s = 0.0; for (int k = 0; k < 8; ++k) s += S[k][i] * MS[k][j]; G[i][j] = s; }
    for (int j = 0; j < 8; ++j) {
        double d = 0.5 * (G[j][j] + G[j][j]);
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !(d <= std::numeric_limits<double>::max())) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 8; ++i) {
            double s = 0.5 * (G[i][j] + G[j][i]);
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / L[j][j];
        }
    }
    for (int j = 0; j < 8; ++j) {                                         // Li = L^-1, column by column
        Li[j][j] = 1.0 / L[j][j];
        for (int i = j + 1; i < 8; ++i) { double s = 0.0; for (int k = j; k < i; ++k) s -= L[i][k] * Li[k][j]; Li[i][j] = s / L[i][i]; }
    }
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { double s = 0.0; for (int k = 0; k <= j; ++k) s += S[i][k] * Li[j][k]; T2[i][j] = s; }
    for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) if (T2[i][j] != T2[i][j]) return false;
    return true;
}

}  // namespace

hipError_t eigs_apply(const EigsIn& in, const std::vector<uint32_t>& off, const mkt_eigs_opts& o, const double* x, uint32_t ncols, double* y, hipStream_t st) {
    EgWork k;
    MKT_TRY(eg_prepare(k, in, off, o, st));
    const uint64_t nb = in.nbins;
    if (nb == 0) return hipSuccess;
    const size_t iobytes = (size_t)nb * ncols * 8;
    MKT_TRY(k.io.alloc((size_t)nb * ncols));
    MKT_TRY(hipMemcpyAsync(k.io, x, iobytes, hipMemcpyHostToDevice, st));
    const unsigned grid8 = grid_for(nb * 8, EGWG);
    hipLaunchKernelGGL(k_eg_load, dim3(grid8), dim3(EGWG), 0, st, (const uint8_t*)k.act, (const double*)k.io, ncols, nb, k.X);
    MKT_TRY(eg_norms(k, in.nchr, st));                                         // g^T X
    MKT_TRY(eg_sweep(in, k.a, st));
    hipLaunchKernelGGL(k_eg_store, dim3(grid_for(nb * ncols, EGWG)), dim3(EGWG), 0, st, (const double*)k.Y, ncols, nb, k.io);
    MKT_TRY(hipGetLastError());
    MKT_TRY(hipMemcpyAsync(y, k.io, iobytes, hipMemcpyDeviceToHost, st));
    return hipStreamSynchronize(st);
}

hipError_t eigs_run(EigsState& s, const EigsIn& in, const std::vector<uint32_t>& off, const mkt_eigs_opts& o, const double* phasing, hipStream_t st) {
    s = EigsState();
    const uint64_t nb = in.nbins;
    const uint32_t nchr = in.nchr;
    const int ne = o.n_eigs;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    DevEvents<4> ev;
    MKT_TRY(ev.create());
    EgWork k;
    MKT_TRY(hipEventRecord(ev[0], st));
    MKT_TRY(eg_prepare(k, in, off, o, st));
    s.vec.assign((size_t)ne * nb, nan);
    s.lambda.assign((size_t)nchr * ne, nan); s.resid.assign((size_t)nchr * ne, nan);
    s.n_good = k.n_good; s.iterations.assign(nchr, 0); s.converged.assign(nchr, 0);
    s.n_eigs = ne;
    std::vector<double> hm((size_t)nchr * EG_HM), nr((size_t)nchr * EG_NR), T((size_t)nchr * EG_T, 0.0);
    std::vector<uint8_t> broke(nchr, 0);
    std::vector<uint32_t>& done = k.h_done;
    const unsigned bgrid = grid_for(nb, EGWG);
    auto live = [&]() { for (uint32_t c = 0; c < nchr; ++c) if (!done[c]) return true; return false; };
    auto transform = [&]() -> hipError_t {
        MKT_TRY(hipMemcpyAsync(k.T, T.data(), T.size() * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_eg_transform, dim3(bgrid), dim3(EGWG), 0, st, (const uint16_t*)in.lay->chr, (const uint32_t*)k.done, (const double*)k.T, nb, k.X.get(), k.Y.get(), k.V.get());
        MKT_TRY(eg_norms(k, nchr, st));
        MKT_TRY(hipMemcpyAsync(nr.data(), k.NR, nr.size() * 8, hipMemcpyDeviceToHost, st));
        return hipStreamSynchronize(st);
    };
    auto fetch_hm = [&]() -> hipError_t {
        MKT_TRY(eg_dots(k, nchr, st));
        MKT_TRY(hipMemcpyAsync(hm.data(), k.HM, hm.size() * 8, hipMemcpyDeviceToHost, st));
        return hipStreamSynchronize(st);
    };
    // X_0 and its orthonormalisation: the Gram matrix is M of the dot products with Y = X, S = I
    if (nb && live()) {
        hipLaunchKernelGGL(k_eg_init, dim3(grid_for(nb * 8, EGWG)), dim3(EGWG), 0, st, k.a, k.X, k.Y);
        MKT_TRY(fetch_hm());
        for (uint32_t c = 0; c < nchr; ++c) {
            if (done[c]) continue;
            double S[8][8], M[8][8], T2[8][8];
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { S[i][j] = i == j ? 1.0 : 0.0; M[i][j] = 0.5 * (hm[(size_t)c * EG_HM + 64 + 8 * i + j] + hm[(size_t)c * EG_HM + 64 + 8 * j + i]); }
            double* t = T.data() + (size_t)c * EG_T;
            if (!eg_orth(S, M, T2)) { broke[c] = 1; memset(T2, 0, sizeof T2); }
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { t[8 * i + j] = S[i][j]; t[72 + 8 * i + j] = T2[i][j]; }
            for (int j = 0; j < 8; ++j) t[64 + j] = 0.0;
        }
        MKT_TRY(transform());
        bool changed = false;
        for (uint32_t c = 0; c < nchr; ++c) if (broke[c] && !done[c]) { done[c] = 1; changed = true; }   // a start block without full rank: nothing to iterate
        if (changed) MKT_TRY(hipMemcpyAsync(k.done, done.data(), (size_t)nchr * 4, hipMemcpyHostToDevice, st));
    }
    MKT_TRY(hipEventRecord(ev[1], st));
    MKT_TRY(hipEventSynchronize(ev[1]));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    s.setup_ms = ms;
    double sweep_ms = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < o.max_iters && live(); ++it) {
        MKT_TRY(hipEventRecord(ev[2], st));
        MKT_TRY(eg_sweep(in, k.a, st));
        MKT_TRY(hipEventRecord(ev[3], st));
        MKT_TRY(fetch_hm());
        MKT_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
        sweep_ms += ms;
        for (uint32_t c = 0; c < nchr; ++c) {
            if (done[c]) continue;
            s.iterations[c] += 1;
            const double* h = hm.data() + (size_t)c * EG_HM;
            double A[8][8], d[8], Vv[8][8], S[8][8], M[8][8], T2[8][8];
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { A[i][j] = 0.5 * (h[8 * i + j] + h[8 * j + i]); M[i][j] = 0.5 * (h[64 + 8 * i + j] + h[64 + 8 * j + i]); }
            eg_jacobi(A, d, Vv);
            int order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
            for (int i = 1; i < 8; ++i)                                   // by |theta| descending, ties in index order
                for (int j = i; j > 0 && std::fabs(d[order[j]]) > std::fabs(d[order[j - 1]]); --j) { const int x = order[j]; order[j] = order[j - 1]; order[j - 1] = x; }
            double* t = T.data() + (size_t)c * EG_T;
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) S[i][j] = Vv[i][order[j]];
            if (!eg_orth(S, M, T2)) { broke[c] = 1; memset(T2, 0, sizeof T2); }
            for (int i = 0; i < 8; ++i) for (int j = 0; j < 8; ++j) { t[8 * i + j] = S[i][j]; t[72 + 8 * i + j] = T2[i][j]; }
            for (int j = 0; j < 8; ++j) t[64 + j] = d[order[j]];
        }
        MKT_TRY(transform());
        bool changed = false;
        for (uint32_t c = 0; c < nchr; ++c) {
            if (done[c]) continue;
            const double *t = T.data() + (size_t)c * EG_T, *r = nr.data() + (size_t)c * EG_NR;
            bool ok = true;
            for (int j = 0; j < ne; ++j) {
                s.lambda[(size_t)c * ne + j] = t[64 + j];
                s.resid[(size_t)c * ne + j] = std::sqrt(r[j]) / std::sqrt(r[8 + j]);
                ok = ok && s.resid[(size_t)c * ne + j] <= o.tol * std::fabs(t[64]);
            }
            if (ok) { s.converged[c] = 1; done[c] = 1; changed = true; }
            else if (broke[c]) { done[c] = 1; changed = true; }           // the block lost rank: what it has is reported, not converged
        }
        if (changed) MKT_TRY(hipMemcpyAsync(k.done, done.data(), (size_t)nchr * 4, hipMemcpyHostToDevice, st));
    }
    MKT_TRY(hipStreamSynchronize(st));
    s.sweep_ms = sweep_ms;
    const double loop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    s.small_ms = loop_ms > sweep_ms ? loop_ms - sweep_ms : 0.0;
    // the Ritz vectors of the last iteration of every chromosome: unit norm over the good bins, orientation, NaN elsewhere
    std::vector<double> V((size_t)nb * 8);
    if (nb) MKT_TRY(hipMemcpy(V.data(), k.V, (size_t)nb * 64, hipMemcpyDeviceToHost));
    s.info.n_chrom = nchr;
    for (uint32_t c = 0; c < nchr; ++c) {
        const uint64_t lo = off[c], hi = c + 1 < nchr ? off[c + 1] : nb;
        if (k.n_good[c] < (uint32_t)(o.min_good > 9 ? o.min_good : 9)) { s.info.skipped += 1; continue; }
        s.info.solved += 1;
        if (s.iterations[c] == 0) continue;                               // max_iters == 0 or a start block without full rank: NaN
        s.info.converged += s.converged[c];
        if (s.iterations[c] > s.info.max_iterations) s.info.max_iterations = s.iterations[c];
        for (int j = 0; j < ne; ++j) {
            double* out = s.vec.data() + (size_t)j * nb;
            double ss = 0.0;
            for (uint64_t b = lo; b < hi; ++b) if (k.h_act[b]) ss += V[8 * b + j] * V[8 * b + j];
            const double norm = std::sqrt(ss);
            double psum = 0.0, pmean = 0.0, big = -1.0;
            uint64_t pn = 0, at = lo;
            for (uint64_t b = lo; b < hi; ++b) {
                if (!k.h_act[b]) continue;
                out[b] = V[8 * b + j] / norm;
                if (std::fabs(out[b]) > big) { big = std::fabs(out[b]); at = b; }
                if (phasing && phasing[b] == phasing[b]) { pmean += phasing[b]; ++pn; }
            }
            if (pn) {
                pmean /= (double)pn;
                for (uint64_t b = lo; b < hi; ++b) if (k.h_act[b] && phasing[b] == phasing[b]) psum += out[b] * (phasing[b] - pmean);
            }
            const bool flip = psum != 0.0 && psum == psum ? psum < 0.0 : out[at] < 0.0;
            if (flip) for (uint64_t b = lo; b < hi; ++b) if (k.h_act[b]) out[b] = -out[b];
        }
    }
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points -----------------------------------------------------------------------------------------------------------
using namespace mkt;

extern "C" void mkt_eigs_opts_default(mkt_eigs_opts* o) {
    if (!o) return;
    o->n_eigs = 3; o->ignore_diags = 2; o->min_good = 9; o->max_iters = 300; o->tol = 1e-8; o->clip = 0.0; o->reserved = 0;
}

// the options checked, the tables there and the full layout built: what eigs and apply share
static int mx_eigs_ready(mkt_matrix* m, uint32_t res_index, const mkt_eigs_opts* opts, mkt_eigs_opts& o, EigsIn& in, double* setup_ms) {
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    o = mx_opts(opts, mkt_eigs_opts_default);
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
    mx_ms(setup_ms, have, s.setup_ms); mx_ms(sweep_ms, have, s.sweep_ms); mx_ms(small_ms, have, s.small_ms);
    return MKT_OK;
}

}  // extern "C"
