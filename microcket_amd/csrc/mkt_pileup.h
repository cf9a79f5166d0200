// mkt_pileup.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_pileup.hip: the pileup (the average contact map in a window of 2 * flank + 1 bins
// around a list of features) over one resolution's resident cells, and the scores formed from it.  include/mkt.h has the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mkt.h"

namespace mkt {

constexpr int kPileFlankMax = 32;
constexpr uint32_t kPileChunk = 256;              // features per chunk: the unit of the summation order (include/mkt.h, step 5)
constexpr uint32_t kPileBatchChunks = 4096;       // chunks whose partial sums are resident at one time

// what the sweep reads: the cells sorted by (bin1, bin2) with their row pointers, the chromosome of a bin and the ranges, the weights
// (nullptr: every bin valid, weight 1) and the divisor of a distance (nullptr for MKT_VALUE_BALANCED)
struct PileIn {
    const uint32_t *b2, *cnt, *rowptr, *off;
    const uint16_t* chr;
    const double *w, *E;
    uint64_t nnz, nbins;
    uint32_t nchr;
};

// the results of the last mkt_matrix_pileup of one resolution, on the host: [side][side] each, row p, column q
struct PileState {
    std::vector<uint64_t> n, csum;
    std::vector<double> vsum, mean;
    std::vector<uint8_t> status;                  // one MKT_PILE_* per feature
    mkt_pileup_info info = {};
    double setup_ms = 0, sweep_ms = 0;
    bool built = false;
};

// step 1 on the host: status[n]; false with `why` naming the feature when one is out of order or past the last bin
bool pileup_status(const uint32_t* a, const uint32_t* b, uint64_t n, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_pileup_opts& o,
                   std::vector<uint8_t>& status, std::string& why);
// step 6 on the host: the seven scores of info from mean[side][side]
void pileup_scores(const double* mean, int flank, int corner, mkt_pileup_info& info);
// steps 2 .. 6 for the features (a, b) whose status pileup_status gave.  Synchronises the stream.
hipError_t pileup_run(PileState& s, const PileIn& in, const uint32_t* a, const uint32_t* b, uint64_t n, const mkt_pileup_opts& o, hipStream_t st);

}  // namespace mkt
