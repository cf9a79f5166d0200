// mkt_balance.hip -- iterative correction (ICE) of one resolution's binned contact matrix on the GPU; include/mkt.h has the
// definition, mkt_matrix.hip the entry points (mkt_matrix_balance) and the host-side filters.
//
// One sweep reads 8 bytes per cell from each half of the cell layout (mkt_layout.h: the rows of the cells and the transposed copy)
// and gathers bias[] (nbins doubles, meant to stay in cache).
//
// Nothing depends on the order anything ran in: a bin's sum is formed by MxLayout::width lanes each walking the row
// and then the column segment with a fixed stride, and the lane tree; bins with more than kBalLong cells get one workgroup and the
// workgroup tree.  Mean and variance of the non-zero marginals are two-level reductions of fixed shape (tile partials, then one
// workgroup), the variance as a second pass over (m - mean)^2 so that tol far below 1e-10 still decides the way the definition does.
#include <hip/hip_runtime.h>

#include "mkt_balance.h"
#include "mkt_segred.h"

namespace mkt {

constexpr int BLWG = 256;
constexpr uint32_t BL_TILE = 8 * BLWG;                // marginals per workgroup in the reductions

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
// W lanes per bin (W = 8 .. 64, a power of two)
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
        acc = lane_tree<W>(acc);
        if (mine && l == 0) m[k] = bk * acc;
    }
}
// one workgroup per long bin: the same walk with 256 lanes
template <bool UNIT>
__global__ __launch_bounds__(BLWG) void k_bl_sweep_long(const uint32_t* longbins, const uint32_t* rowptr, const uint32_t* colptr, const uint32_t* b2, const uint32_t* cnt,
                                                        const uint2* tr, uint32_t ig, const double* bias, double* m, const BalState* state) {
    __shared__ double sh[BLWG / 64];
    if (state && state->done) return;
    const uint32_t k = longbins[blockIdx.x];
    const double bk = UNIT ? 1.0 : bias[k];
    double acc = 0.0;
    if (bk != 0.0) acc = bl_walk<UNIT>(k, threadIdx.x, BLWG, rowptr[k], rowptr[k + 1], colptr[k], colptr[k + 1], b2, cnt, tr, ig, bias);
    acc = wg_tree(acc, sh);
    if (threadIdx.x == 0) m[k] = bk * acc;
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
    double v[2] = {s, c};
    wg_tree_n(v, sh);
    if (threadIdx.x == 0) { partial[2 * (uint64_t)blockIdx.x] = v[0]; partial[2 * (uint64_t)blockIdx.x + 1] = v[1]; }
}
// pass 1, level 2 (one workgroup): the mean; no non-zero marginal ends the iteration here
__global__ __launch_bounds__(BLWG) void k_bl_sum2(const double* partial, uint32_t tiles, BalState* state) {
    __shared__ double sh[2 * BLWG / 64];
    if (state->done) return;
    double v[2] = {0.0, 0.0};
    for (uint32_t t = threadIdx.x; t < tiles; t += BLWG) { v[0] += partial[2 * (uint64_t)t]; v[1] += partial[2 * (uint64_t)t + 1]; }
    wg_tree_n(v, sh);
    if (threadIdx.x == 0) {
        const double s = v[0], c = v[1];
        state->iters += 1;
        state->sum = s; state->cnt = (unsigned long long)c;
        if (c == 0.0) { state->empty = 1; state->done = 1; state->mean = s / c; state->var = s / c; }       // 0 / 0: NaN
        else state->mean = s / c;
    }
}
// pass 2, level 1: per tile the sum of (m - mean)^2 over the non-zero marginals; and the step itself: bias /= (m / mean, 0 -> 1)
__global__ __launch_bounds__(BLWG) void k_bl_var1(const double* m, uint64_t nbins, double* bias, double* partial, const BalState* state) {
    __shared__ double sh[2 * BLWG / 64];                   // one sum; sized like pass 1
    if (state->done) return;
    const double mean = state->mean;
    const uint64_t b = (uint64_t)blockIdx.x * BL_TILE;
    double s = 0.0;
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
    s = wg_tree(s, sh);
    if (threadIdx.x == 0) partial[2 * (uint64_t)blockIdx.x] = s;
}
__global__ __launch_bounds__(BLWG) void k_bl_var2(const double* partial, uint32_t tiles, double tol, BalState* state) {
    __shared__ double sh[2 * BLWG / 64];                   // one sum; sized like pass 1
    if (state->done) return;
    double s = 0.0;
    for (uint32_t t = threadIdx.x; t < tiles; t += BLWG) s += partial[2 * (uint64_t)t];
    s = wg_tree(s, sh);
    if (threadIdx.x == 0) {
        const double var = s / (double)state->cnt / state->mean;
        state->ssq = s; state->var = var;
        if (var < tol) { state->converged = 1; state->done = 1; }
    }
}
__global__ __launch_bounds__(BLWG) void k_bl_weights(const double* bias, uint64_t nbins, const BalState* state, double* w) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nbins) return;
    const double b = bias[k];
    w[k] = (b == 0.0 || state->empty) ? dev_nan() : b / sqrt(state->mean);
}

// ---------------------------------------------------------------------------------------------------------------
template <bool UNIT>
static hipError_t bl_launch_sweep(const MxLayout& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ig, const double* bias, double* m,
                                  const BalState* state, hipStream_t st) {
    if (nbins == 0) return hipSuccess;
    dispatch_width(s.width, [&](auto W) {
        hipLaunchKernelGGL((k_bl_sweep<UNIT, decltype(W)::value>), dim3(grid_for(nbins * (uint64_t)s.width, BLWG)), dim3(BLWG), 0, st, (const uint32_t*)s.rowptr,
                           (const uint32_t*)s.colptr, b2, cnt, (const uint2*)s.tr, nbins, ig, bias, m, state);
    });
    if (s.nlong)
        hipLaunchKernelGGL((k_bl_sweep_long<UNIT>), dim3(s.nlong), dim3(BLWG), 0, st, (const uint32_t*)s.longbins, (const uint32_t*)s.rowptr, (const uint32_t*)s.colptr, b2, cnt,
                           (const uint2*)s.tr, ig, bias, m, state);
    return hipGetLastError();
}

hipError_t bal_marginal(const MxLayout& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, bool unit, const double* bias, double* m, hipStream_t st) {
    return unit ? bl_launch_sweep<true>(s, b2, cnt, nbins, ignore_diags, bias, m, nullptr, st) : bl_launch_sweep<false>(s, b2, cnt, nbins, ignore_diags, bias, m, nullptr, st);
}

size_t bal_partial_bytes(uint64_t nbins) { return (size_t)((nbins + BL_TILE - 1) / BL_TILE + 1) * 16; }

hipError_t bal_iterate(const MxLayout& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, double tol, uint32_t count,
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
    hipLaunchKernelGGL(k_bl_weights, dim3(grid_for(nbins, BLWG)), dim3(BLWG), 0, st, bias, nbins, state, w);
    return hipGetLastError();
}

}  // namespace mkt
