// mkt_hic.h -- the .hic container from the resident cells of a matrix object: what the matrix object (mkt_matrix_obj.h) hands to mkt_hic.hip and what it keeps.
// include/mkt.h has the file definition, DESIGN.md 7l the design.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_devbuf.h"
#include "mkt_layout.h"

namespace mkt {

constexpr uint32_t kHicBlockBinsMax = 32767;        // local coordinates, row and record counts are int16
constexpr uint32_t kHicCountShort = 32767;          // the largest count a short block holds

struct HicResIn {                                   // one resolution of the object, in the object's order
    MxCells cells;                                  // ascending in (bin1, bin2); nnz may be 0 (then the pointers may be null)
    const uint16_t* chr = nullptr;                  // [nbins] chromosome of a bin (MxLayout::chr); unused when nnz is 0
    const std::vector<uint32_t>* off = nullptr;     // first bin of a chromosome, host copy
    uint32_t bin_size = 0;
    const double* d_w = nullptr;                    // [nbins] balancing weights on the device, or null
};
struct HicTiming { double sort_ms = 0, serialise_ms = 0, deflate_ms = 0, pack_ms = 0; };
struct HicState {
    bool built = false;
    DevBuf<uint8_t> image;                          // the file
    mkt_hic_info info = {};
    std::vector<HicTiming> timing;                  // by resolution index of the object
};

// the file of `res` into s; on an error s is left empty and *why says what is wrong.  Returns an MKT_* code.
int hic_build(HicState& s, const std::vector<HicResIn>& res, const std::vector<std::string>& names, const std::vector<uint32_t>& lens,
              const mkt_hic_opts& o, hipStream_t st, std::string* why);

}  // namespace mkt
