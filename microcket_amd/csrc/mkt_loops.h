// mkt_loops.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_loops.hip: loop calling (donut enrichment, FDR thresholds, clustering) over one
// resolution's resident cells, the weights and the smoothed genome-wide expected.  include/mkt.h has the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/mkt.h"
#include "mkt_devbuf.h"

namespace mkt {

constexpr int kLpWmax = 20;                       // the largest window_max
constexpr int kLpChunks = 28, kLpCols = 2048;     // histogram: expected chunks x min(count, 2047)
constexpr uint8_t kLpNoChunk = 255;               // chunk of an undefined region or of r > 512

// what the neighbourhood pass reads: the cells sorted by (bin1, bin2), their row pointers, the chromosome of a bin and the ranges,
// the weights (nullptr: every bin valid, weight 1) and E = expected_smooth of the genome-wide table
struct LoopsIn {
    const uint32_t *b1, *b2, *cnt, *rowptr, *off;
    const uint16_t* chr;
    const double *w, *E;
    uint64_t nnz, nbins, genome_rows;
    uint32_t nchr;
};

// the results of the last mkt_matrix_loops of one resolution: per cell on the device, tables and loops on the host
struct LoopsState {
    DevBuf<uint8_t> status, window, chunk, enriched;   // [nnz], [nnz], [4 nnz], [nnz]
    DevBuf<uint16_t> kept;                          // [4 nnz] kept positions of a region
    DevBuf<uint64_t> csum;                          // [nnz] Csum_LL of the final window
    DevBuf<double> r, e, bsum, esum;                // [4 nnz] each, cell-major
    std::vector<uint64_t> hist;                     // [4][28][2048]
    std::vector<uint32_t> thr;                      // [4][28]
    std::vector<mkt_loop> loops;
    mkt_loops_info info = {};
    double pass_ms = 0, hist_ms = 0, flag_ms = 0;
    bool built = false;
};

// edge_k of step 5
double loops_edge(int k);
// step 7 on the host: T[R][k] from H[R][k][x]
void loops_thresholds(const uint64_t* hist, double fdr, uint32_t* thr);
// steps 1 .. 9.  Synchronises the stream.
hipError_t loops_run(LoopsState& s, const LoopsIn& in, const std::vector<uint32_t>& off, const mkt_loops_opts& o, hipStream_t st);

}  // namespace mkt
