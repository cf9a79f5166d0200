// mkt_layout.h -- one resolution's cell layout, built on demand and kept as long as the cells: what balance, expected, loops and eigs
// all read next to the cells themselves.  And the one grouping of cells by a key that the layout and the expected tables use.
// DESIGN.md 7f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkt_devbuf.h"

namespace mkt {

constexpr uint32_t kBalLong = 1024;

// the resident cells of one resolution, ascending in (bin1, bin2)
struct MxCells {
    const uint32_t *b1, *b2, *cnt, *off;  // off: [nchr] first bin of a chromosome
    uint64_t nnz, nbins;
    uint32_t nchr;
    int B;                                // bits of a bin id
};

struct MxLayout {
    DevBuf<uint16_t> chr;                 // [nbins] chromosome (table index) of a bin
    DevBuf<uint32_t> rowptr;              // [nbins + 1] into the cells: row k = cells [rowptr[k], rowptr[k + 1]) (those with bin1 == k)
    DevBuf<uint32_t> colptr;              // [nbins + 1] into tr: column k = the cells with bin2 == k, ascending in bin1
    DevBuf<uint2> tr;                     // [nnz] (bin1, count) ordered by (bin2, bin1): the transposed copy
    DevBuf<uint32_t> longbins;            // bins whose row + column hold more than kBalLong cells: one workgroup each
    uint32_t nlong = 0;
    int width = 8;                        // lanes per bin for all the others (8 .. 64), fixed by nnz / nbins
    bool has_chr = false, has_rows = false, has_full = false;
};

// each step builds what is missing and nothing else: chr; + rowptr (all the loop caller needs); + the transposed half, which
// synchronises the stream.  hipErrorInvalidValue: 2^32 cells or bins, or more.
hipError_t layout_chr(MxLayout& L, const MxCells& c, hipStream_t st);
hipError_t layout_rows(MxLayout& L, const MxCells& c, hipStream_t st);
hipError_t layout_full(MxLayout& L, const MxCells& c, hipStream_t st);

// Grouping n cells by a key.  The owner writes key << shift | cell index into keys(); group() sorts them by bits
// [lo_bit, lo_bit + nbits) with the stable radix passes of the duplicate marker (cell order survives inside a group) and sets
// ptr_out[k] = first j with keys()[j] >> shift >= k for k < nptr - 1, ptr_out[nptr - 1] = n.  The owner then gathers its payload
// through the low bits of keys().  The scratch goes with the object.
class KeyGroup {
    DevBuf<uint64_t> a_, b_;
    DevBuf<uint32_t> radix_;
    uint64_t *ka_ = nullptr, *kb_ = nullptr;

public:
    hipError_t alloc(uint64_t n);
    uint64_t* keys() const { return ka_; }
    hipError_t group(uint64_t n, int lo_bit, int nbits, int shift, uint64_t nptr, uint32_t* ptr_out, hipStream_t st);
};

}  // namespace mkt
