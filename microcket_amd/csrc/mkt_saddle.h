// mkt_saddle.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_saddle.hip: the saddle tables (the mean observed / expected of every pair of groups
// of bins ranked by a track) over one resolution's resident cells, and the compartment strength formed from them.  include/mkt.h has
// the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mkt.h"

namespace mkt {

constexpr int kSaddleGroupsMax = 64;
constexpr uint32_t kSaddleChunk = 4096;           // cells per chunk: the unit of the summation order (include/mkt.h, step 3)
constexpr uint8_t kSaddleNone = 255;              // the group byte of a bin without a group

// what the sweep reads: the cells in (bin1, bin2) order, the chromosome of a bin, the weights (nullptr: weight 1) and the divisors: of a
// distance (cis) or of a trans block
struct SaddleIn {
    const uint32_t *b1, *b2, *cnt;
    const uint16_t* chr;
    const double *w, *cis_div, *tr_div;
    uint64_t nnz, nbins;
    uint32_t nchr;
};

// the results of the last mkt_matrix_saddle of one resolution, on the host; the tables are [Q][Q], symmetric
struct SaddleState {
    std::vector<uint64_t> n, nnz, csum;
    std::vector<double> vsum, mean;
    std::vector<uint8_t> group;                   // [nbins]
    std::vector<uint64_t> g_bins;                 // [Q] bins of a group
    std::vector<double> g_lo, g_hi;               // [Q] the track value of its lowest and highest rank, NaN for an empty group
    std::vector<double> strength, aa_ab, bb_ab;   // [Q / 2], index k - 1
    mkt_saddle_info info = {};
    double setup_ms = 0, sweep_ms = 0;
    bool built = false;
};

// step 1 on the host: group[nbins] and the per-group bins, lo and hi, candidates and kept of info; w: the weights (NaN = masked), nullptr = every bin valid
void saddle_groups(const double* track, const double* w, uint64_t nbins, const mkt_saddle_opts& o, SaddleState& s);
// step 4 on the host: n of the unordered entries, [Q][Q] with only a <= b filled
void saddle_positions(const uint8_t* group, const std::vector<uint32_t>& off, uint64_t nbins, const mkt_saddle_opts& o, uint64_t* n);
// step 6 on the host: the profile and the three scores of info at k = corner, from the symmetric vsum and n
void saddle_scores(const double* vsum, const uint64_t* n, int Q, int corner, SaddleState& s);
// steps 1 .. 6; setup_ms is the host's wall time of steps 1 and 4, the copy of the weights and the upload of the groups, sweep_ms the
// device time of the chunk kernel and the fold.  Synchronises the stream.
hipError_t saddle_run(SaddleState& s, const SaddleIn& in, const std::vector<uint32_t>& off, const double* track, const mkt_saddle_opts& o, hipStream_t st);

}  // namespace mkt
