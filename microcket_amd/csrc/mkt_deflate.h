// mkt_deflate.h -- the GPU deflate (mkt_deflate.hip: LZ77 + Huffman codes per block of at most BGZF_RAW bytes) behind its two framings.
// BGZF (SAMv1 4.1): every block of BGZF_RAW bytes becomes a gzip member of its own, with its CRC-32 (sam2bam, mkt_bam.hip).
// zlib streams (RFC 1950) out of deflate pieces (the .hic writer, mkt_hic.hip): a payload is cut into pieces of at most kZsPiece bytes; a piece
// becomes deflate block(s) with BFINAL = 0 that end on a byte (an empty stored block closes a coded piece; one that does not shrink is stored), so a stream is
//     78 9C | the pieces, copied one behind the other | 03 00 | Adler-32, big-endian
// (03 00: the empty fixed block with BFINAL = 1).  The Adler-32 of a piece is made with it; zs_adler_join combines them.
// A block or piece starts on a multiple of 16 in `raw`, which is readable 64 bytes past its end.  Levels: 0 stored, 1 the fixed code, 2 a code per block.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mkt {

constexpr uint32_t BGZF_RAW = 0xff00;               // uncompressed bytes per BGZF block (htslib's BGZF_BLOCK_SIZE)
constexpr uint32_t BGZF_STRIDE = 0x10000;           // room for one compressed block in the work buffer (a block is <= 64 KiB)
constexpr uint32_t kZsPiece = BGZF_RAW;             // raw bytes per piece at the most: a piece is what the deflate kernel takes as a block
constexpr uint32_t kZsStride = BGZF_STRIDE;         // room for one deflated piece in the work buffer (a piece is <= kZsPiece + 5 bytes)
constexpr uint32_t kZsFrame = 2 + 2 + 4;            // bytes of a stream that are not pieces

__device__ inline void put32(uint8_t*& o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); o += 4; }      // little-endian store (both framings, and the BAM records)
struct ZsPieces { const uint64_t* off; const uint32_t* len; uint32_t* adler; };     // per piece: where it starts in raw, its bytes; out: its Adler-32

// Adler-32 of X followed by Y (len_y bytes) from the two values
__host__ __device__ inline uint32_t zs_adler_join(uint32_t x, uint32_t y, uint64_t len_y) {
    const uint32_t M = 65521u;
    const uint32_t ax = x & 0xFFFFu, bx = x >> 16, ay = y & 0xFFFFu, by = y >> 16;
    const uint32_t a = (ax + ay + M - 1u) % M;
    const uint32_t b = (uint32_t)(((uint64_t)bx + by + (len_y % M) * (uint64_t)((ax + M - 1u) % M)) % M);
    return (b << 16) | a;
}

struct CrcTabs { uint32_t t[256]; uint32_t x2n[32]; };      // what the BGZF framing reads on the device; the caller allocates and uploads it
void crc_tables(CrcTabs* ct);
extern const unsigned char kBgzfEof[28];            // the empty block that ends a BGZF file

size_t deflate_scratch_bytes(uint64_t batch);       // scratch for `batch` blocks or pieces per launch (levels 1 and 2; none needed for level 0)
// nblocks BGZF blocks of raw[0, nraw) -> comp (BGZF_STRIDE apart), their sizes -> csize; `batch` blocks per deflate launch
hipError_t bgzf_launch(const uint8_t* raw, uint64_t nraw, uint64_t nblocks, int level, const CrcTabs* ct, uint8_t* comp, uint64_t* csize, uint32_t* scratch,
                       uint64_t batch, hipStream_t st);
// the compressed blocks, packed: block b of comp -> out[coff[b], coff[b + 1])
hipError_t bgzf_pack(const uint8_t* comp, const uint64_t* coff, uint64_t nblocks, uint8_t* out, hipStream_t st);
// npieces pieces of raw -> comp (kZsStride apart), their sizes -> csize, their Adler-32 -> zp.adler
hipError_t zs_deflate(const uint8_t* raw, ZsPieces zp, uint64_t npieces, int level, uint8_t* comp, uint64_t* csize, uint32_t* scratch, uint64_t batch, hipStream_t st);

}  // namespace mkt
