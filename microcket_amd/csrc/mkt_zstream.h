// mkt_zstream.h -- zlib streams (RFC 1950) out of deflate pieces: the second framing of the LZ77 + Huffman stage of mkt_bam.hip, next to
// BGZF.  A payload is cut into pieces of at most kZsPiece bytes; a piece becomes deflate block(s) with BFINAL = 0 that end on a byte (an
// empty stored block closes a coded piece; a piece that does not shrink is one stored block), so a stream is
//     78 9C | the pieces, copied one behind the other | 03 00 | Adler-32, big-endian
// (03 00: the empty fixed block with BFINAL = 1).  The Adler-32 of a piece is made with it; zs_adler_join combines them.
// A piece must start on a multiple of 16 in `raw`, and `raw` must be readable up to the next multiple of 16 behind every piece.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mkt {

constexpr uint32_t kZsPiece = 0xff00;               // raw bytes per piece at the most (the BGZF block size: the same kernel body)
constexpr uint32_t kZsStride = 0x10000;             // room for one deflated piece in the work buffer (a piece is <= kZsPiece + 5 bytes)
constexpr uint32_t kZsFrame = 2 + 2 + 4;            // bytes of a stream that are not pieces

struct ZsPieces { const uint64_t* off; const uint32_t* len; uint32_t* adler; };     // per piece: where it starts in raw, its bytes; out: its Adler-32

// Adler-32 of X followed by Y (len_y bytes) from the two values
__host__ __device__ inline uint32_t zs_adler_join(uint32_t x, uint32_t y, uint64_t len_y) {
    const uint32_t M = 65521u;
    const uint32_t ax = x & 0xFFFFu, bx = x >> 16, ay = y & 0xFFFFu, by = y >> 16;
    const uint32_t a = (ax + ay + M - 1u) % M;
    const uint32_t b = (uint32_t)(((uint64_t)bx + by + (len_y % M) * (uint64_t)((ax + M - 1u) % M)) % M);
    return (b << 16) | a;
}

size_t zs_scratch_bytes(uint64_t batch);            // deflate scratch for `batch` pieces per launch (levels 1 and 2; 0 for level 0)
// npieces pieces of raw -> comp (kZsStride apart), their sizes -> csize, their Adler-32 -> zp.adler; level 0 stored, 1 fixed codes, 2 dynamic
hipError_t zs_deflate(const uint8_t* raw, ZsPieces zp, uint64_t npieces, int level, uint8_t* comp, uint64_t* csize, uint32_t* scratch, uint64_t batch, hipStream_t st);

}  // namespace mkt
