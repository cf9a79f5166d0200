// mkt_insulation.hip -- the diamond insulation score of every bin over one resolution's binned contact matrix on the GPU, and the
// boundaries called from it on the host; include/mkt.h has the definition; the entry points (mkt_matrix_insulation,
// mkt_matrix_fetch_insulation) are at the end, on the object of mkt_matrix_obj.h.
//
// The sweep.  A GROUP of G lanes owns one bin i of chromosome [lo, hi).  The diamond of the largest window W_max is the rows
// a = i - p (0 <= p < W_max, a >= lo) and in each row the columns max(i, a + ignore_diags) <= b < min(i + W_max, hi).  Lane l takes
// the rows p = l, l + G, ..: a row with a masked bin is skipped; otherwise the lane adds the row's kept positions per window from the
// prefix count of the valid bins (integers), finds the row's first column by a binary search between the row pointers and walks
// the stored cells in ascending b up to the last column: at most W_max cells, so no row is long.  A cell goes to the partial sums
// of its SHELL k = the smallest k with max(p, q) < window[k]: the windows are nested, so one walk of the largest diamond serves all
// of them.  The lane tree adds the lanes shell by shell, lane 0 adds the shells 0 .. k in that order for window k and
// divides.  Nothing depends on the order anything ran in: the sums have one shape per (G, windows).
//
// Steps 4 .. 7 (normalisation, minima, strengths, flags) are host code in this file, which is compiled without floating-point
// contraction (the division and the subtraction are compared bit for bit with tests/insuldef.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>

#include "mkt_matrix_obj.h"
#include "mkt_segred.h"

#pragma clang fp contract(off)

namespace mkt {

constexpr int INSWG = 256;
typedef unsigned long long ins_u64;

// win[k >= K] is INT32_MAX: no cell is that far out, so the shell of a cell never counts them
struct InsOpts { int K, wmax, ig; int win[kInsWindows]; ins_u64 n_full[kInsWindows]; double min_frac; };
struct InsOut { ins_u64 *n_valid, *csum; double *bsum, *score; };

// V: [nbins + 1] valid bins below k, or nullptr when every bin is valid
template <int G>
__global__ __launch_bounds__(INSWG) void k_ins_sweep(InsIn in, InsOpts o, const uint32_t* V, InsOut out) {
    const uint64_t i = (uint64_t)blockIdx.x * (INSWG / G) + threadIdx.x / G;
    const int gl = (int)(threadIdx.x & (G - 1));
    double bs[kInsWindows] = {0.0, 0.0, 0.0, 0.0};
    ins_u64 cs[kInsWindows] = {0, 0, 0, 0}, nv[kInsWindows] = {0, 0, 0, 0};
    if (i < in.nbins) {
        const uint32_t c = in.chr[i];
        const int64_t ii = (int64_t)i, lo = in.off[c], hi = c + 1u < in.nchr ? (int64_t)in.off[c + 1u] : (int64_t)in.nbins;
        const int64_t rows = ii - lo + 1 < o.wmax ? ii - lo + 1 : o.wmax;
        const int64_t bend = ii + o.wmax < hi ? ii + o.wmax : hi;
        for (int p = gl; p < rows; p += G) {
            const int64_t a = ii - p;
            double wr = 1.0;
            if (in.w) { wr = in.w[a]; if (wr != wr) continue; }
            const int64_t blo = a + o.ig > ii ? a + o.ig : ii;
#pragma unroll
            for (int k = 0; k < kInsWindows; ++k) {                               // the kept positions of this row, per window
                if (k >= o.K || p >= o.win[k]) continue;
                const int64_t bh = ii + o.win[k] < hi ? ii + o.win[k] : hi;
                if (blo < bh) nv[k] += V ? (ins_u64)(V[bh] - V[blo]) : (ins_u64)(bh - blo);
            }
            if (blo >= bend) continue;
            const uint32_t r1 = in.rowptr[a + 1];
            for (uint32_t s = seg_lower_bound(in.b2, in.rowptr[a], r1, (uint32_t)blo); s < r1; ++s) {      // the stored cells of the row, ascending b
                const int64_t col = in.b2[s];
                if (col >= bend) break;
                double wc = 1.0;
                if (in.w) { wc = in.w[col]; if (wc != wc) continue; }
                const uint32_t n = in.cnt[s];
                const double v = __dmul_rn(__dmul_rn((double)n, wr), wc);
                const int q = (int)(col - ii), far = p > q ? p : q;
                const int sh = (far >= o.win[0]) + (far >= o.win[1]) + (far >= o.win[2]);
#pragma unroll
                for (int k = 0; k < kInsWindows; ++k)
                    if (sh == k) { bs[k] = __dadd_rn(bs[k], v); cs[k] += n; }
            }
        }
    }
    lane_tree_v<G>(AddRn(), bs[0], cs[0], nv[0], bs[1], cs[1], nv[1], bs[2], cs[2], nv[2], bs[3], cs[3], nv[3]);
    if (i >= in.nbins || gl != 0) return;
    double B = 0.0;
    ins_u64 Cs = 0;
#pragma unroll
    for (int k = 0; k < kInsWindows; ++k) {
        if (k >= o.K) break;
        B = k ? __dadd_rn(B, bs[k]) : bs[0];
        Cs += cs[k];
        const uint64_t at = (uint64_t)k * in.nbins + i;
        const bool none = o.n_full[k] == 0 || nv[k] == 0 || (double)nv[k] < __dmul_rn(o.min_frac, (double)o.n_full[k]);
        out.n_valid[at] = nv[k]; out.csum[at] = Cs; out.bsum[at] = B;
        out.score[at] = none ? dev_nan() : B / (double)nv[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------
uint64_t insulation_n_full(int window, int ignore_diags) {
    uint64_t n = 0;
    for (int64_t p = 0; p < window; ++p) {
        const int64_t q0 = (int64_t)ignore_diags - p;                         // q0 <= q < window
        n += (uint64_t)(q0 <= 0 ? window : q0 >= window ? 0 : window - q0);
    }
    return n;
}

// One lane per row of the largest diamond up to a wave; half of that when a row's walk meets less than one stored cell on average
// (rows = nnz / nbins cells, of which the walk sees at most W_max): a lane then takes two rows that are mostly a search alone.
int insulation_width(uint64_t nbins, uint64_t nnz, int wmax) {
    const uint64_t per_row = nbins ? nnz / nbins : 0;
    return seg_width(per_row >= 1 ? (uint64_t)wmax : (uint64_t)wmax / 2);
}

void insulation_call(const double* score, uint64_t nbins, const std::vector<uint32_t>& off, double min_strength, double* L, double* strength, uint8_t* boundary,
                     uint64_t* counts) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    counts[0] = counts[1] = counts[2] = 0;
    const size_t nc = off.size();
    for (size_t c = 0; c < nc; ++c) {
        const uint64_t lo = off[c], hi = c + 1 < nc ? off[c + 1] : nbins;
        double sum = 0.0;                                                     // step 4: ascending bins
        uint64_t n = 0;
        for (uint64_t k = lo; k < hi; ++k) if (std::isfinite(score[k]) && score[k] > 0.0) { sum += score[k]; ++n; }
        const double mean = n ? sum / (double)n : nan;
        for (uint64_t k = lo; k < hi; ++k) {
            const double x = score[k];
            L[k] = n && x == x && x != 0.0 ? std::log2(x / mean) : nan;
            strength[k] = nan; boundary[k] = 0;
            counts[0] += std::isfinite(L[k]);
        }
        for (uint64_t s0 = lo; s0 < hi;) {                                    // steps 5 .. 7, segment by segment
            if (!std::isfinite(L[s0])) { ++s0; continue; }
            uint64_t e0 = s0;
            while (e0 + 1 < hi && std::isfinite(L[e0 + 1])) ++e0;
            for (uint64_t s = s0; s <= e0;) {
                const double x = L[s];
                uint64_t e = s;
                while (e < e0 && L[e + 1] == x) ++e;
                if (s > s0 && e < e0 && L[s - 1] > x && L[e + 1] > x) {
                    double lm = -inf, rm = -inf;
                    for (uint64_t j = s; j > s0 && L[j - 1] >= x; --j) lm = L[j - 1] > lm ? L[j - 1] : lm;
                    for (uint64_t j = e + 1; j <= e0 && L[j] >= x; ++j) rm = L[j] > rm ? L[j] : rm;
                    strength[s] = (lm < rm ? lm : rm) - x;
                    ++counts[1];
                    if (strength[s] >= min_strength) { boundary[s] = 1; ++counts[2]; }
                }
                s = e + 1;
            }
            s0 = e0 + 1;
        }
    }
}

hipError_t insulation_run(InsState& s, const InsIn& in, const std::vector<uint32_t>& off, const mkt_insulation_opts& opts, hipStream_t st) {
    const uint64_t nb = in.nbins;
    const int K = opts.n_windows;
    if (nb >= (1ull << 32) || in.nnz >= (1ull << 32)) return hipErrorInvalidValue;
    DevEvents<4> ev;
    MKT_TRY(ev.create());
    DevBuf<uint32_t> d_V;
    DevBuf<ins_u64> d_nv, d_cs;
    DevBuf<double> d_bs, d_sc;
    const size_t rows = (size_t)K * nb;
    std::vector<uint32_t> V;
    MKT_TRY(hipEventRecord(ev[0], st));
    if (in.w) {                                                           // the prefix count of the valid bins, from one copy of the weights
        std::vector<double> w(nb);
        if (nb) MKT_TRY(hipMemcpyAsync(w.data(), in.w, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipStreamSynchronize(st));
        V.assign(nb + 1, 0);
        for (uint64_t k = 0; k < nb; ++k) V[k + 1] = V[k] + (w[k] == w[k] ? 1u : 0u);
        MKT_TRY(d_V.alloc(nb + 1));
        MKT_TRY(hipMemcpyAsync(d_V, V.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, st));     // V is not touched before the next synchronise
    }
    MKT_TRY(hipEventRecord(ev[1], st));
    MKT_TRY(d_nv.alloc(rows, 64)); MKT_TRY(d_cs.alloc(rows, 64)); MKT_TRY(d_bs.alloc(rows, 64)); MKT_TRY(d_sc.alloc(rows, 64));
    InsOpts o;
    o.K = K; o.wmax = opts.window[K - 1]; o.ig = opts.ignore_diags; o.min_frac = opts.min_frac_valid;
    for (int k = 0; k < kInsWindows; ++k) {
        o.win[k] = k < K ? opts.window[k] : std::numeric_limits<int32_t>::max();
        o.n_full[k] = k < K ? insulation_n_full(opts.window[k], opts.ignore_diags) : 0;
    }
    InsOut out;
    out.n_valid = d_nv; out.csum = d_cs; out.bsum = d_bs; out.score = d_sc;
    MKT_TRY(hipEventRecord(ev[2], st));
    if (nb) dispatch_width(insulation_width(nb, in.nnz, o.wmax), [&](auto Wc) {
        constexpr int G = decltype(Wc)::value;
        hipLaunchKernelGGL(k_ins_sweep<G>, dim3(grid_for(nb, INSWG / G)), dim3(INSWG), 0, st, in, o, (const uint32_t*)d_V.get(), out);
    });
    MKT_TRY(hipEventRecord(ev[3], st));
    MKT_TRY(hipGetLastError());
    s.n_valid.assign(rows, 0); s.csum.assign(rows, 0); s.bsum.assign(rows, 0.0); s.score.assign(rows, 0.0);
    if (rows) {
        MKT_TRY(hipMemcpyAsync(s.n_valid.data(), d_nv, rows * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipMemcpyAsync(s.csum.data(), d_cs, rows * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipMemcpyAsync(s.bsum.data(), d_bs, rows * 8, hipMemcpyDeviceToHost, st));
        MKT_TRY(hipMemcpyAsync(s.score.data(), d_sc, rows * 8, hipMemcpyDeviceToHost, st));
    }
    MKT_TRY(hipStreamSynchronize(st));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, ev[0], ev[1])); s.setup_ms = ms;
    MKT_TRY(hipEventElapsedTime(&ms, ev[2], ev[3])); s.sweep_ms = ms;
    s.log2_score.assign(rows, 0.0); s.strength.assign(rows, 0.0); s.boundary.assign(rows, 0);
    memset(&s.info, 0, sizeof s.info);
    s.info.n_chrom = (uint32_t)off.size();
    for (int k = 0; k < K; ++k) {
        uint64_t counts[3];
        const size_t at = (size_t)k * nb;
        insulation_call(s.score.data() + at, nb, off, opts.min_strength, s.log2_score.data() + at, s.strength.data() + at, s.boundary.data() + at, counts);
        s.info.defined[k] = counts[0]; s.info.minima[k] = counts[1]; s.info.boundaries[k] = counts[2];
    }
    s.n_windows = K;
    s.built = true;
    return hipSuccess;
}

}  // namespace mkt

// ---- the entry points (comparisons and copies only: nothing here rounds) ------------------------------------------------------------
using namespace mkt;
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
    const mkt_insulation_opts o = mx_opts(opts, mkt_insulation_opts_default);
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
    if (const int rc = mx_cells32(m, "insulation", r.nnz)) return rc;
    MCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    r.ins = InsState();
    MX_OR_RESET(m, "insulation: ", r.ins, layout_rows(r.lay, mx_cells(r), st));   // the row pointers and the chromosome of a bin are all the sweep needs
    InsIn in;
    in.b2 = r.d_b2; in.cnt = r.d_cnt; in.rowptr = r.lay.rowptr; in.off = r.d_off; in.chr = r.lay.chr;
    in.w = o.use_weights ? r.d_w.get() : nullptr;
    in.nnz = r.nnz; in.nbins = r.nbins; in.nchr = (uint32_t)r.off.size();
    MX_OR_RESET(m, "insulation: ", r.ins, insulation_run(r.ins, in, r.off, o, st));
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
    mx_ms(setup_ms, have, s.setup_ms); mx_ms(sweep_ms, have, s.sweep_ms);
    return MKT_OK;
}

}  // extern "C"
