// mkt_scc.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_scc.hip: the stratum-adjusted correlation of two binned contact matrices of one
// resolution (both smoothed with a box filter, correlated diagonal by diagonal, the correlations combined with weights).
// include/mkt.h has the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mkt.h"

namespace mkt {

constexpr int kSccHMax = 16;                      // the largest half width of the box filter
constexpr uint32_t kSccChunk = 256;               // positions of a stratum per chunk: the unit of the summation order (include/mkt.h, step 5)

// one matrix as the fill kernel reads it: the cells in (bin1, bin2) order, the row pointers of the layout and the weights
// (nullptr: weight 1)
struct SccSide {
    const uint32_t *b1, *b2, *cnt, *rowptr;
    const double* w;
    uint64_t nnz;
};

// the results of the last mkt_matrix_scc of one resolution, on the host; the strata table is [n_chr][strata], chromosome-major
struct SccState {
    std::vector<uint64_t> n_cand, n;
    std::vector<double> sx, sy, sxx, syy, sxy, rho, w;
    std::vector<double> c_scc, c_num, c_den;      // [n_chr]
    std::vector<uint64_t> c_scored;               // [n_chr]
    mkt_scc_info info = {};
    double fill_ms = 0, sweep_ms = 0;
    bool built = false;
};

// steps 6 .. 8 on the host from the sums of the strata table: rho and w per stratum, the per-chromosome arrays and scc, scored of info
void scc_scores(SccState& s, uint32_t nchr, uint32_t strata, int weighting, uint64_t min_n);
// steps 1 .. 8.  off: the first bin of every chromosome; o: checked options with max_diag resolved.  fill_ms and sweep_ms are device
// times (HIP events) added over the slabs.  Synchronises the stream.  hipErrorOutOfMemory with *why set when the bands do not fit
// at the smallest slab.
hipError_t scc_run(SccState& s, const SccSide& a, const SccSide& b, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_scc_opts& o, hipStream_t st, std::string* why);

}  // namespace mkt
