// mkt_rle.h -- the run-length reduction of sorted 64-bit keys that the binning (mx_bin) and the viewpoint profiles (vp_run) share: head
// flags on key[j] != key[j - 1], a scan for the output slots, and a run's count is the DIFFERENCE of two neighbouring head positions
// (exact for runs of any length across tiles and workgroups, no atomics).  The kernels are in mkt_matrix.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkt_devbuf.h"

namespace mkt {

// the words `sums` needs for nv sorted keys (the head passes and the byte sums of the text passes, which are more)
size_t rle_sums_words(uint64_t nv);
// The runs of key[0, nv), keys being hi << B | lo with B <= 32 and hi < 2^32.  *runs: their number; when it is 0 or above nv (which
// cannot be) nothing more is done.  Otherwise hi, lo, cnt (allocated here, *runs each) hold the runs in key order, pos (allocated here) the
// head positions, sums[0, text blocks) the exclusive prefixes of the bytes of the lines "hi \t lo \t count \n" per 1024 runs and
// *text_bytes their total.  Synchronises the stream.
hipError_t rle_reduce(const uint64_t* key, uint64_t nv, int B, uint64_t* sums, DevBuf<uint32_t>& hi, DevBuf<uint32_t>& lo, DevBuf<uint32_t>& cnt, DevBuf<uint32_t>& pos,
                      uint64_t* runs, uint64_t* text_bytes, hipStream_t st);

}  // namespace mkt
