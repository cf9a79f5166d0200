// mkt_balance.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_balance.hip: iterative correction over one resolution's resident cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkt_layout.h"

namespace mkt {

// device state of the iteration (one per balance call)
struct BalState {
    double sum, mean, ssq, var;
    unsigned long long cnt;
    uint32_t iters, done, converged, empty;
};

// m[k] = marg(x)[k] over the used cells; unit: x = 1 (bias is not read), else x = count * bias[bin1] * bias[bin2]
hipError_t bal_marginal(const MxLayout& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, bool unit, const double* bias, double* m, hipStream_t st);
size_t bal_partial_bytes(uint64_t nbins);
// `count` iterations of step 4 behind each other; each is a no-op once state->done is set.  state is zeroed by the caller.
hipError_t bal_iterate(const MxLayout& s, const uint32_t* b2, const uint32_t* cnt, uint64_t nbins, uint32_t ignore_diags, double tol, uint32_t count,
                       double* bias, double* m, double* partial, BalState* state, hipStream_t st);
// weight = bias / sqrt(state->mean), NaN where bias == 0 or state->empty
hipError_t bal_weights(const double* bias, uint64_t nbins, const BalState* state, double* w, hipStream_t st);

}  // namespace mkt
