// mkt_expected.h -- what the matrix object (mkt_matrix_obj.h) needs of mkt_expected.hip: expected-contact tables (distance decay per chromosome and
// genome-wide, trans block means) and per-cell observed / expected values over one resolution's resident cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mkt_layout.h"

namespace mkt {

// Built once per resolution from the cells sorted by (bin1, bin2) and kept until the cells go away: the cells grouped by segment.
// Segment off_c + d: the cells of chromosome c on diagonal d; segment nbins + row: the cells of one trans block.
struct ExpSetup {
    DevBuf<uint32_t> sb1, sb2, scnt; // [nnz] the cells ordered by (segment, cell index)
    DevBuf<uint32_t> segptr;         // [nseg + 1] into the grouped copy
    DevBuf<uint2> ltask;             // long segments (more than kExpLong cells) in chunks of kExpChunk cells: [p0, p1) per chunk
    DevBuf<uint64_t> lseg;           // per long segment: segment id, first chunk, chunks
    uint32_t ntask = 0, nlong = 0;
    DevBuf<uint64_t> moff;           // [nchr + 1] first word of a chromosome's validity bits
    uint64_t mwords = 0;
    uint64_t nseg = 0, trans_rows = 0, genome_rows = 0;
    int width = 8;                   // lanes per segment for all the others (8 .. 64), fixed by nnz / nseg
    bool built = false;
};
constexpr uint32_t kExpLong = 1024;
constexpr uint32_t kExpChunk = 4096;

// The tables of the last mkt_matrix_expected: a host mirror that the fetches read, and on the device what the values divide by.
struct ExpTables {
    std::vector<uint64_t> cis_n, cis_c, tr_n, tr_c, g_n, g_c;
    std::vector<double> cis_s, tr_s, tr_e, g_s, g_e, g_sm;
    uint32_t smooth_groups = 0;
    DevBuf<uint64_t> d_n, d_c;                  // [nbins] n_valid, [nseg] count_sum
    DevBuf<double> d_s;                         // [nseg] balanced_sum
    DevBuf<uint64_t> d_mask;
    DevBuf<double> d_part;                      // [2 * ntask] partial sums of the long segments' chunks
    DevBuf<double> d_cis_e, d_cis_sm, d_tr_e;   // [genome_rows], [genome_rows], [trans_rows]
    int use_weights = 0;
    bool built = false;
};

// the grouping.  chr: MxLayout::chr; off / nchr: the chromosomes' first bins (device and host).  Synchronises the stream; the sort
// scratch is gone when it returns.  hipErrorInvalidValue: segment id and cell index do not fit 64 bits together.
hipError_t exp_setup(ExpSetup& s, const uint16_t* chr, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t nnz, uint64_t nbins, const uint32_t* d_off,
                     const std::vector<uint32_t>& off, hipStream_t st);
// n_valid, count_sum and balanced_sum of every segment into t.d_n / t.d_c / t.d_s (w: the weights, nullptr = every bin valid, weight 1)
hipError_t exp_sums(const ExpSetup& s, ExpTables& t, const uint16_t* chr, uint64_t nbins, const uint32_t* d_off, const double* w, hipStream_t st);
// the host side: copies the sums back, forms the trans, genome-wide and smoothed tables in the fixed order of the definition and
// puts the divisors on the device.  Synchronises the stream.
hipError_t exp_finish(const ExpSetup& s, ExpTables& t, uint64_t nbins, const std::vector<uint32_t>& off, hipStream_t st);
// out[i] = value of cell first + i (kind: MKT_VALUE_*); t and chr may be nullptr for kind 0
hipError_t exp_values(const ExpTables* t, const uint16_t* chr, const uint32_t* b1, const uint32_t* b2, const uint32_t* cnt, uint64_t first, uint64_t n,
                      const uint32_t* d_off, uint32_t nchr, const double* w, int kind, double* out, hipStream_t st);

}  // namespace mkt
