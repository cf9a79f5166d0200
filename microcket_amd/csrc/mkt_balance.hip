// mkt_balance.hip -- iterative correction (ICE) of one resolution's binned contact matrix on the GPU; include/mkt.h has the
// definition, mkt_matrix.hip the entry points (mkt_matrix_balance) and the host-side filters.
//
// The cells arrive sorted by (bin1, bin2), so row k (the cells with bin1 == k) is a contiguous segment: rowptr is a lower bound per
// bin.  The other half of bin k's marginal are the cells with bin2 == k; for those a transposed copy (bin1, count) ordered by
// (bin2, bin1) is made once: the stable radix passes of the duplicate marker over the bin2 bits of bin2 << 32 | cell index.
// One sweep then reads 8 bytes per cell from each copy and gathers bias[] (nbins doubles, meant to stay in cache).
//
// Nothing depends on the order anything ran in: there are no floating-point atomics.  A bin's sum is formed by a fixed number of
// lanes (BalSetup::width, from nnz / nbins) each walking the row and then the column segment with a fixed stride, and a fixed
// shuffle tree; bins with more than kBalLong cells get one workgroup with the same shape one level up.  Mean and variance of the
// non-zero marginals are two-level reductions of fixed shape (tile partials, then one workgroup), the variance as a second pass
// over (m - mean)^2 so that tol far below 1e-10 still decides the way the definition does.
#include <hip/hip_runtime.h>

#include <vector>

#include "mkt_balance.h"
#include "mkt_launch.h"

namespace mkt {

constexpr int BLWG = 256;
constexpr uint32_t BL_TILE = 8 * BLWG;                // marginals per workgroup in the reductions

__device__ inline uint32_t bl_lower(const uint32_t* a, uint32_t n, uint32_t v) {      // first i with a[i] >= v
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(BLWG) void k_bl_rowptr(const uint32_t* b1, uint32_t nnz, uint64_t nbins, uint32_t* ptr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= nbins) ptr[k] = k == nbins ? nnz : bl_lower(b1, nnz, (uint32_t)k);
}
__global__ __launch_bounds__(BLWG) void k_bl_tkeys(const uint32_t* b2, uint32_t nnz, uint64_t* key) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nnz) key[s] = ((uint64_t)b2[s] << 32) | s;
}
__global__ __launch_bounds__(BLWG) void k_bl_gather(const uint64_t* key, const uint32_t* b1, const uint32_t* cnt, uint32_t nnz, uint2* tr) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nnz) { const uint32_t s = (uint32_t)key[j]; tr[j] = make_uint2(b1[s], cnt[s]); }
}
__global__ __launch_bounds__(BLWG) void k_bl_colptr(const uint64_t* key, uint32_t nnz, uint64_t nbins, uint32_t* ptr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nbins) return;
    uint32_t lo = 0, hi = nnz;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((key[mid] >> 32) < k) lo = mid + 1; else hi = mid; }
    ptr[k] = k == nbins ? nnz : lo;
}

// lane `l` of `W` walks elements l, l + W, ... of the row segment and then of the column segment
template <bool UNIT>
__device__ inline double bl_walk(uint32_t k, uint32_t l, uint32_t W, uint32_t r0, uint32_t r1, uint32_t c0, uint32_t c1, const uint32_t* b2, const uint32_t* cnt,
                                 const uint2* tr, uint32_t ig, const double* bias) {
    double acc = 0.0;
    for (uint32_t s = r0 + l; s < r1; s += W) {
        const uint32_t o = b2[s];
        if (o - k >= ig) acc += UNIT ? 1.0 : (double)cnt[s] * bias[o];
    }
    for (uint32_t s = c0 + l; s < c1; s += W) {
        const uint2 x = tr[s];
        if (k - x.x >= ig) acc += UNIT ? 1.0 : (double)x.y * bias[x.x];
    }
    return acc;
}
// W lanes per bin (W = 8 .. 64, a power of two): the tree adds lane l + d to lane l for d = W / 2 .. 1
template <bool UNIT, int W>
__global__ __launch_bounds__(BLWG) void k_bl_sweep(const uint32_t* rowptr, const uint32_t* colptr, const uint32_t* b2, const uint32_t* cnt, const uint2* tr, uint64_t nbins,
                                                   uint32_t ig, const double* bias, double* m, const BalState* state) {
    if (state && state->done) return;
    const uint64_t k = ((uint64_t)blockIdx.x * BLWG + threadIdx.x) / W;
    const uint32_t l = threadIdx.x & (W - 1);
    double acc = 0.0;
    bool mine = false;
    if (k < nbins) {
        const uint32_t r0 = rowptr[k], r1 = rowptr[k + 1], c0 = colptr[k], c1 = colptr[k + 1];
        mine = (uint64_t)(r1 - r0) + (c1 - c0) <= kBalLong;
        const double bk = UNIT ? 1.0 : bias[k];
        if (mine && bk != 0.0) acc = bl_walk<UNIT>((uint32_t)k, l, W, r0, r1, c0, c1, b2, cnt, tr, ig, bias);
#pragma unroll
        for (int d = W / 2; d >= 1; d >>= 1) acc += __shfl_down(acc, d, W);
        if (mine && l == 0) m[k] = bk * acc;
    }
}
// one workgroup per long bin: the same walk with 256 lanes, the tree per wave, the four wave sums added in wave order
template <bool UNIT>
__global__ __launch_bounds__(BLWG) void k_bl_sweep_long(const uint32_t* longbins, const uint32_t* rowptr, const uint32_t* colptr, const uint32_t* b2, const uint32_t* cnt,
                                                        const uint2* tr, uint32_t ig, const double* bias, double* m, const BalState* state) {
    __shared__ double sh[BLWG / 64];
    if (state && state->done) return;
    const uint32_t k = longbins[blockIdx.x];
    const double bk = UNIT ? 1.0 : bias[k];
    double acc = 0.0;
    if (bk != 0.0) acc = bl_walk<UNIT>(k, threadIdx.x, BLWG, rowptr[k], rowptr[k + 1], colptr[k], colptr[k + 1], b2, cnt, tr, ig, bias);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) m[k] = bk * (((sh[0] + sh[1]) + sh[2]) + sh[3]);
}

// a workgroup's sum of a (and of b): lane tree, then the four wave sums in wave order; the result is valid in thread 0
__device__ inline void bl_wgsum(double& a, double& b, double* sh /* [2 * BLWG / 64] */) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_down(a, d, 64); b += __shfl_down(b, d, 64); }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = a; sh[BLWG / 64 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        b = ((sh[4] + sh[5]) + sh[6]) + sh[7];
    }
    __syncthreads();
}
// pass 1, level 1: per tile the sum and the number of the non-zero marginals (the count is an integer: exact as a double)
__global__ __launch_bounds__(BLWG) void k_bl_sum1(const double* m, uint64_t nbins, double* partial, const BalState* state) {
    __shared__ double sh[2 * BLWG / 64];
    if (state->done) return;
    const uint64_t b = (uint64_t)blockIdx.x * BL_TILE;
    double s = 0.0, c = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < BL_TILE / BLWG; ++j) {
        const uint64_t k = b + j * BLWG + threadIdx.x;
        if (k < nbins) { const double x = m[k]; if (x != 0.0) { s += x; c += 1.0; } }
    }
    bl_wgsum(s, c, sh);
    if (threadIdx.x == 0) { partial[2 * (uint64_t)blockIdx.x] = s; partial[2 * (uint64_t)blockIdx.x + 1] = c; }
}
// pass 1, level 2 (one workgroup): the mean; no non-zero marginal ends the iteration here
__global__ __launch_bounds__(BLWG) void k_bl_sum2(const double* partial, uint32_t tiles, BalState* state) {
    __shared__ double sh[2 * BLWG / 64];
    if (state->done) return;
    double s = 0.0, c = 0.0;
    for (uint32_t t = threadIdx.x; t < tiles; t += BLWG) { s += partial[2 * (uint64_t)t]; c += partial[2 * (uint64_t)t + 1]; }
    bl_wgsum(s, c, sh);
    if (threadIdx.x == 0) {
        state->iters += 1;
        state->sum = s; state->cnt = (unsigned long long)c;
        if (c == 0.0) { state->empty = 1; state->done = 1; state->mean = s / c; state->var = s / c; }       // 0 / 0: NaN
        else state->mean = s / c;
    }
}
// pass 2, level 1: per tile the sum of (m - mean)^2 over the non-zero marginals; and the step itself: bias /= (m / mean, 0 -> 1)
__global__ __launch_bounds__(BLWG) void k_bl_var1(const double* m, uint64_t nbins, double* bias, double* partial, const BalState* state) {
    __shared__ double sh[2 * BLWG / 64];
    if (state->done) return;
    const double mean = state->mean;
    const uint64_t b = (uint64_t)blockIdx.x * BL_TILE;
    double s = 0.0, unused = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < BL_TILE / BLWG; ++j) {
        const uint64_t k = b + j * BLWG + threadIdx.x;
        if (k < nbins) {
            const double x = m[k];
            if (x != 0.0) { const double d = x - mean; s += d * d; }
            double q = x / mean;
            if (q == 0.0) q = 1.0;
            bias[k] = bias[k] / q;
        }
    }
    bl_wgsum(s, unused, sh);
    if (threadIdx.x == 0) partial[2 * (uint64_t)blockIdx.x] = s;
}
__global__ __launch_bounds__(BLWG) void k_bl_var2(const double* partial, uint32_t tiles, double tol, BalState* state) {
    __shared__ double sh[2 * BLWG / 64];
    if (state->done) return;
    double s = 0.0, unused = 0.0;
    for (uint32_t t = threadIdx.x; t < tiles; t += BLWG) s += partial[2 * (uint64_t)t];
    bl_wgsum(s, unused, sh);
    if (threadIdx.x == 0) {
        const double var = s / (double)state->cnt / state->mean;
        state->ssq = s; state->var = var;
        if (var < tol) { state->converged = 1; state->done = 1; }
    }
}
__global__ __launch_bounds__(BLWG) void k_bl_weights(const double* bias, uint64_t nbins, const BalState* state, double* w) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nbins) return;
    const double b = bias[k], nan = __longlong_as_double(0x7FF8000000000000ll);
    w[k] = (b == 0.0 || state->empty) ? nan : b / sqrt(state->mean);
}

// ---------------------------------------------------------------------------------------------------------------
void bal_free(BalSetup& s) {
    if (s.rowptr) (void)hipFree(s.rowptr);
    if (s.colptr) (void)hipFree(s.colptr);
    if (s.tr) (void)hipFree(s.tr);
    if (s.longbins) (void)hipFree(s.longbins);
    s = BalSetup();
}

hipError_t bal_rowptr(uint32_t* rowptr, const uint32_t* b1, uint64_t nnz, uint64_t nbins, hipStream_t st) {
    if (nnz >= (1ull << 32) || nbins >= (1ull << 32)) return hipErrorInvalidValue;
    if (nnz == 0) return hipMemsetAsync(rowptr, 0, (size_t)(nbins + 1) * 4, st);
    hipLaunchKernelGGL(k_bl_rowptr, dim3((unsigned)((nbins + 1 + BLWG - 1) / BLWG)), dim3(BLWG), 0, st, b1, (uint32_t)nnz, nbins, rowptr);
    return hipGetLastError();
}

hipError_t bal_setup(BalSetup& s, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t nnz, uint64_t nbins, int B, hipStream_t st) {
    bal_free(s);
    if (nnz >= (1ull << 32) || nbins >= (1ull << 32)) return hipErrorInvalidValue;
    hipError_t e;
    uint64_t *kA = nullptr, *kB = nullptr;
    uint32_t* d_radix = nullptr;
    auto done = [&](hipError_t r) {
        if (kA) (void)hipFree(kA);
        if (kB) (void)hipFree(kB);
        if (d_radix) (void)hipFree(d_radix);
        if (r != hipSuccess) bal_free(s);
        return r;
    };
    const size_t pbytes = (size_t)(nbins + 1) * 4;
    if ((e = hipMalloc((void**)&s.rowptr, pbytes)) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&s.colptr, pbytes)) != hipSuccess) return done(e);
    if ((e = hipMalloc((void**)&s.tr, (size_t)nnz * 8 + 64)) != hipSuccess) return done(e);
    const unsigned pgrid = (unsigned)((nbins + 1 + BLWG - 1) / BLWG), cgrid = (unsigned)((nnz + BLWG - 1) / BLWG);
    if (nnz == 0) {
        if ((e = hipMemsetAsync(s.rowptr, 0, pbytes, st)) != hipSuccess) return done(e);
        if ((e = hipMemsetAsync(s.colptr, 0, pbytes, st)) != hipSuccess) return done(e);
    } else {
        if ((e = hipMalloc((void**)&kA, (size_t)nnz * 8 + 64)) != hipSuccess) return done(e);
        if ((e = hipMalloc((void**)&kB, (size_t)nnz * 8 + 64)) != hipSuccess) return done(e);
        if ((e = hipMalloc((void**)&d_radix, radix64_count_bytes(nnz))) != hipSuccess) return done(e);
        if ((e = bal_rowptr(s.rowptr, b1, nnz, nbins, st)) != hipSuccess) return done(e);
        hipLaunchKernelGGL(k_bl_tkeys, dim3(cgrid), dim3(BLWG), 0, st, b2, (uint32_t)nnz, kA);
        if ((e = launch_radix64(kA, kB, nnz, 32, B, d_radix, st)) != hipSuccess) return done(e);       // stable: (bin2, bin1) order from (bin1, bin2) order
        hipLaunchKernelGGL(k_bl_gather, dim3(cgrid), dim3(BLWG), 0, st, (const uint64_t*)kA, b1, cnt, (uint32_t)nnz, s.tr);
        hipLaunchKernelGGL(k_bl_colptr, dim3(pgrid), dim3(BLWG), 0, st, (const uint64_t*)kA, (uint32_t)nnz, nbins, s.colptr);
        if ((e = hipGetLastError()) != hipSuccess) return done(e);
    }
    // the long bins, from the two pointer arrays (once per resolution)
    std::vector<uint32_t> rp(nbins + 1), cp(nbins + 1), lb;
    if ((e = hipMemcpyAsync(rp.data(), s.rowptr, pbytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return done(e);
    if ((e = hipMemcpyAsync(cp.data(), s.colptr, pbytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return done(e);
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return done(e);
    for (uint64_t k = 0; k < nbins; ++k)
        if ((uint64_t)(rp[k + 1] - rp[k]) + (cp[k + 1] - cp[k]) > kBalLong) lb.push_back((uint32_t)k);
    s.nlong = (uint32_t)lb.size();
    if (s.nlong) {
        if ((e = hipMalloc((void**)&s.longbins, (size_t)s.nlong * 4)) != hipSuccess) return done(e);
        if ((e = hipMemcpy(s.longbins, lb.data(), (size_t)s.nlong * 4, hipMemcpyHostToDevice)) != hipSuccess) return done(e);
    }
    const uint64_t avg = nbins ? 2 * nnz / nbins : 0;                  // cells a bin walks on average
    s.width = avg >= 48 ? 64 : avg >= 24 ? 32 : avg >= 12 ? 16 : 8;
    s.built = true;
    return done(hipSuccess);
}

template <bool UNIT>
static hipError_t bl_launch_sweep(const BalSetup& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ig, const double* bias, double* m,
                                  const BalState* state, hipStream_t st) {
    if (nbins == 0) return hipSuccess;
    const unsigned grid = (unsigned)((nbins * (uint64_t)s.width + BLWG - 1) / BLWG);
#define BL_SWEEP(W) hipLaunchKernelGGL((k_bl_sweep<UNIT, W>), dim3(grid), dim3(BLWG), 0, st, (const uint32_t*)s.rowptr, (const uint32_t*)s.colptr, b2, cnt, (const uint2*)s.tr, nbins, ig, bias, m, state)
    switch (s.width) {
        case 64: BL_SWEEP(64); break;
        case 32: BL_SWEEP(32); break;
        case 16: BL_SWEEP(16); break;
        default: BL_SWEEP(8); break;
    }
#undef BL_SWEEP
    if (s.nlong)
        hipLaunchKernelGGL((k_bl_sweep_long<UNIT>), dim3(s.nlong), dim3(BLWG), 0, st, (const uint32_t*)s.longbins, (const uint32_t*)s.rowptr, (const uint32_t*)s.colptr, b2, cnt,
                           (const uint2*)s.tr, ig, bias, m, state);
    return hipGetLastError();
}

hipError_t bal_marginal(const BalSetup& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, bool unit, const double* bias, double* m, hipStream_t st) {
    return unit ? bl_launch_sweep<true>(s, b2, cnt, nbins, ignore_diags, bias, m, nullptr, st) : bl_launch_sweep<false>(s, b2, cnt, nbins, ignore_diags, bias, m, nullptr, st);
}

size_t bal_partial_bytes(uint64_t nbins) { return (size_t)((nbins + BL_TILE - 1) / BL_TILE + 1) * 16; }

hipError_t bal_iterate(const BalSetup& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, double tol, uint32_t count,
                       double* bias, double* m, double* partial, BalState* state, hipStream_t st) {
    const uint32_t tiles = (uint32_t)((nbins + BL_TILE - 1) / BL_TILE);
    for (uint32_t it = 0; it < count; ++it) {
        hipError_t e = bl_launch_sweep<false>(s, b2, cnt, nbins, ignore_diags, bias, m, state, st);
        if (e != hipSuccess) return e;
        if (tiles) hipLaunchKernelGGL(k_bl_sum1, dim3(tiles), dim3(BLWG), 0, st, (const double*)m, nbins, partial, (const BalState*)state);
        hipLaunchKernelGGL(k_bl_sum2, dim3(1), dim3(BLWG), 0, st, (const double*)partial, tiles, state);
        if (tiles) hipLaunchKernelGGL(k_bl_var1, dim3(tiles), dim3(BLWG), 0, st, (const double*)m, nbins, bias, partial, (const BalState*)state);
        hipLaunchKernelGGL(k_bl_var2, dim3(1), dim3(BLWG), 0, st, (const double*)partial, tiles, tol, state);
    }
    return hipGetLastError();
}

hipError_t bal_weights(const double* bias, uint64_t nbins, const BalState* state, double* w, hipStream_t st) {
    if (nbins == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bl_weights, dim3((unsigned)((nbins + BLWG - 1) / BLWG)), dim3(BLWG), 0, st, bias, nbins, state, w);
    return hipGetLastError();
}

}  // namespace mkt
