// mkt_sortlib.h -- the building blocks of mkt_sort.hip that mkt_rmdup.hip, mkt_bam.hip and mkt_matrix.hip use as well: newline
// index, 16-byte records, stable LSD radix passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mkt_devbuf.h"

namespace mkt {

struct SortRec { uint64_t hi; uint32_t lo; uint32_t idx; };

// The newline index of text[0, n) (readable up to 64 bytes past n; it must end with a newline), in two phases, because every caller
// decides something from the line count before it pays for the starts.
struct LineIndex {
    DevBuf<uint64_t> cnt, starts;      // newlines per 64 KiB chunk, scanned; starts[0] = 0, starts[k + 1] = 1 + position of newline k
    uint64_t nlines = 0;
    uint32_t chunks = 0;
    size_t asked = 0;                  // bytes of the allocation tried last: hipErrorOutOfMemory from either phase is that one failing
    hipError_t count(const uint8_t* d_text, uint64_t n, hipStream_t st);      // -> nlines; the stream is idle afterwards
    hipError_t fill(const uint8_t* d_text, uint64_t n, hipStream_t st);       // nlines + 2 starts, queued on st (no synchronisation)
};
// the same in one call, synchronised (starts: hipMalloc'ed here, nlines + 2 entries; the caller frees)
hipError_t sort_line_index(const uint8_t* d_text, uint64_t n, hipStream_t st, uint64_t** d_starts, uint64_t* nlines);
// stable LSD passes (4 bits each) over bits [lo_bit, lo_bit + nbits) of rec.hi (which = 1) or rec.lo (which = 0); the sorted
// records end up in rA (the two buffers are swapped as needed).  d_hist: 16 * 1024 + 64 uint32.
void sort_radix_passes(SortRec*& rA, SortRec*& rB, uint64_t n, uint32_t* d_hist, int which, int lo_bit, int nbits, hipStream_t st);
constexpr size_t kSortHistBytes = (size_t)16 * 1024 * 4 + 256;

}  // namespace mkt
