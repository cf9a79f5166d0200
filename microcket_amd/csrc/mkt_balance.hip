// mkt_balance.hip -- iterative correction (ICE) of one resolution's binned contact matrix on the GPU; include/mkt.h has the
// definition; the entry points (mkt_matrix_balance) and the host-side filters are at the end, on the object of mkt_matrix_obj.h.
//
// One sweep reads 8 bytes per cell from each half of the cell layout (mkt_layout.h: the rows of the cells and the transposed copy)
// and gathers bias[] (nbins doubles, meant to stay in cache).
//
// Nothing depends on the order anything ran in: a bin's sum is formed by MxLayout::width lanes each walking the row
// and then the column segment with a fixed stride, and the lane tree; bins with more than kBalLong cells get one workgroup and the
// workgroup tree.  Mean and variance of the non-zero marginals are two-level reductions of fixed shape (tile partials, then one
// workgroup), the variance as a second pass over (m - mean)^2 so that tol far below 1e-10 still decides the way the definition does.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <algorithm>
#include <cmath>

#include "mkt_matrix_obj.h"
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

// ---- the entry points -----------------------------------------------------------------------------------------------------------
using namespace mkt;
extern "C" {

void mkt_balance_opts_default(mkt_balance_opts* o) {
    if (!o) return;
    o->ignore_diags = 2; o->min_nnz = 10; o->min_count = 0.0; o->mad_max = 5.0; o->tol = 1e-5; o->max_iters = 200; o->reserved = 0;
}

int mkt_matrix_balance(mkt_matrix* m, uint32_t res_index, const mkt_balance_opts* opts, mkt_balance_stats* stats) {
    if (m && stats) memset(stats, 0, sizeof *stats);
    MxRes* rp = nullptr;
    MX_RES(m, res_index, &rp);
    const mkt_balance_opts o = mx_opts(opts, mkt_balance_opts_default);
    if (o.ignore_diags < 0) return mfail(m, MKT_E_ARG, "balance: ignore_diags %d is negative", o.ignore_diags);
    if (o.min_nnz < 0) return mfail(m, MKT_E_ARG, "balance: min_nnz %d is negative", o.min_nnz);
    if (!(o.min_count >= 0.0)) return mfail(m, MKT_E_ARG, "balance: min_count %g is negative or NaN", o.min_count);
    if (!(o.mad_max >= 0.0)) return mfail(m, MKT_E_ARG, "balance: mad_max %g is negative or NaN", o.mad_max);
    if (!(o.tol >= 0.0)) return mfail(m, MKT_E_ARG, "balance: tol %g is negative or NaN", o.tol);
    if (o.max_iters <= 0) return mfail(m, MKT_E_ARG, "balance: max_iters %d (at least 1 is needed)", o.max_iters);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "balance: the reserved field is not 0");
    MxRes& r = *rp;
    if (const int rc = mx_need(m, res_index, r, MX_RAN, "balance")) return rc;
    if (const int rc = mx_cells32(m, "balance", r.nnz)) return rc;
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const uint64_t nb = r.nbins;
    mx_invalidate(r, MX_NEW_WEIGHTS);
    r.bal_setup_ms = r.bal_iter_ms = 0;
    DevBuf<double> d_bias, d_m, d_part, d_w;                            // d_w becomes r.d_w at the end: a failure leaves no weights
    DevBuf<BalState> d_state;
#define BRUN(call) MX(m, "balance: ", call)
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
    const bool have = m->ran && r.balanced;
    mx_ms(setup_ms, have, r.bal_setup_ms); mx_ms(iter_ms, have, r.bal_iter_ms);
    return MKT_OK;
}

}  // extern "C"
