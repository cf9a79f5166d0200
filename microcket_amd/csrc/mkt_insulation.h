// mkt_insulation.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_insulation.hip: the diamond insulation score of every bin at up to four nested
// windows over one resolution's resident cells, and the boundaries called from it.  include/mkt.h has the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mkt.h"

namespace mkt {

constexpr int kInsWindows = 4;                    // the most windows of one call
constexpr int kInsWmax = 1024;                    // the largest window, in bins

// what the sweep reads: the cells sorted by (bin1, bin2) with their row pointers, the chromosome of a bin and the ranges, and the
// weights (nullptr: every bin valid, weight 1)
struct InsIn {
    const uint32_t *b2, *cnt, *rowptr, *off;
    const uint16_t* chr;
    const double* w;
    uint64_t nnz, nbins;
    uint32_t nchr;
};

// the results of the last mkt_matrix_insulation of one resolution, on the host: [n_windows][nbins] each
struct InsState {
    std::vector<uint64_t> n_valid, csum;
    std::vector<double> bsum, score, log2_score, strength;
    std::vector<uint8_t> boundary;
    mkt_insulation_info info = {};
    int n_windows = 0;
    double setup_ms = 0, sweep_ms = 0;
    bool built = false;
};

// n_full of step 1: the unclipped positions of a window
uint64_t insulation_n_full(int window, int ignore_diags);
// lanes per bin (8 .. 64) of the sweep
int insulation_width(uint64_t nbins, uint64_t nnz, int wmax);
// steps 4 .. 7 for one window: from score[nbins] the log2 track, the strengths and the flags; counts[3] = defined, minima, boundaries
void insulation_call(const double* score, uint64_t nbins, const std::vector<uint32_t>& off, double min_strength, double* log2_score, double* strength, uint8_t* boundary,
                     uint64_t* counts);
// steps 1 .. 7.  Synchronises the stream.
hipError_t insulation_run(InsState& s, const InsIn& in, const std::vector<uint32_t>& off, const mkt_insulation_opts& o, hipStream_t st);

}  // namespace mkt
