// mkt_eigs.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_eigs.hip: the leading eigenvectors of every chromosome's cis observed / expected - 1
// matrix (compartments) over one resolution's resident cells, by a block iteration whose product A X never forms the matrix.
// include/mkt.h has the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mkt.h"
#include "mkt_layout.h"

namespace mkt {

constexpr int kEgCols = 8;                        // columns of the block: X and Y are stored [bin][8]
constexpr uint32_t kEgChunk = 256;                // bins per chunk of the per-chromosome dot products
constexpr int kEgJacobiSweeps = 12;               // cyclic Jacobi sweeps of the 8 x 8 Rayleigh-Ritz step

// what the sweep reads: the cells sorted by (bin1, bin2) with their full layout (row pointers, transposed copy, chromosome of a bin),
// the ranges, the weights (nullptr: every bin valid, weight 1) and E = expected_smooth of the genome-wide table
struct EigsIn {
    const MxLayout* lay;
    const uint32_t *b2, *cnt, *off;
    const double *w, *E;
    uint64_t nbins;
    uint32_t nchr;
};

// the results of the last mkt_matrix_eigs of one resolution, on the host
struct EigsState {
    std::vector<double> vec;                      // [n_eigs][nbins]
    std::vector<double> lambda, resid;            // [nchr][n_eigs]
    std::vector<uint32_t> n_good, iterations;     // [nchr]
    std::vector<uint8_t> converged;               // [nchr]
    mkt_eigs_info info = {};
    int n_eigs = 0;
    double setup_ms = 0, sweep_ms = 0, small_ms = 0;
    bool built = false;
};

// steps 1 .. 4.  phasing: nbins doubles on the host or nullptr.  Synchronises the stream.
hipError_t eigs_run(EigsState& s, const EigsIn& in, const std::vector<uint32_t>& off, const mkt_eigs_opts& o, const double* phasing, hipStream_t st);
// y = A x through the sweep kernel of the iteration; x, y: [nbins][ncols] on the host.  Synchronises the stream.
hipError_t eigs_apply(const EigsIn& in, const std::vector<uint32_t>& off, const mkt_eigs_opts& o, const double* x, uint32_t ncols, double* y, hipStream_t st);

}  // namespace mkt
