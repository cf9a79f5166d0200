// mkt_balance.h -- what mkt_matrix.hip needs of mkt_balance.hip: iterative correction over one resolution's resident cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mkt {

// What is built once per resolution from the cells sorted by (bin1, bin2) and kept until the cells go away.
struct BalSetup {
    uint32_t* rowptr = nullptr;      // [nbins + 1] into the cells: row k = cells [rowptr[k], rowptr[k + 1]) (those with bin1 == k)
    uint32_t* colptr = nullptr;      // [nbins + 1] into tr: column k = the cells with bin2 == k, ascending in bin1
    uint2* tr = nullptr;             // [nnz] (bin1, count) ordered by (bin2, bin1): the transposed copy
    uint32_t* longbins = nullptr;    // bins whose row + column hold more than kBalLong cells: one workgroup each
    uint32_t nlong = 0;
    int width = 8;                   // lanes per bin for all the others (8 .. 64), fixed by nnz / nbins
    bool built = false;
};
constexpr uint32_t kBalLong = 1024;

// device state of the iteration (one per balance call)
struct BalState {
    double sum, mean, ssq, var;
    unsigned long long cnt;
    uint32_t iters, done, converged, empty;
};

void bal_free(BalSetup& s);
// the row pointers alone, into rowptr[nbins + 1] (what the loop caller needs when no balance has built a BalSetup)
hipError_t bal_rowptr(uint32_t* rowptr, const uint32_t* b1, uint64_t nnz, uint64_t nbins, hipStream_t st);
// rowptr, the transposed copy and colptr.  b1 / b2 / cnt: the nnz cells ascending in (bin1, bin2).  Synchronises the stream.
hipError_t bal_setup(BalSetup& s, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t nnz, uint64_t nbins, int B, hipStream_t st);
// m[k] = marg(x)[k] over the used cells; unit: x = 1 (bias is not read), else x = count * bias[bin1] * bias[bin2]
hipError_t bal_marginal(const BalSetup& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, bool unit, const double* bias, double* m, hipStream_t st);
size_t bal_partial_bytes(uint64_t nbins);
// `count` iterations of step 4 behind each other; each is a no-op once state->done is set.  state is zeroed by the caller.
hipError_t bal_iterate(const BalSetup& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, double tol, uint32_t count,
                       double* bias, double* m, double* partial, BalState* state, hipStream_t st);
// weight = bias / sqrt(state->mean), NaN where bias == 0 or state->empty
hipError_t bal_weights(const double* bias, uint64_t nbins, const BalState* state, double* w, hipStream_t st);

}  // namespace mkt
