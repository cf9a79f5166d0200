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

struct CrcTabs { uint32_t t[256]; uint32_t x2n[32]; };      // what the BGZF framing reads on the device; the caller allocates and uploads it (the reader of mkt_inflate.hip too)
void crc_tables(CrcTabs* ct);
extern const unsigned char kBgzfEof[28];            // the empty block that ends a BGZF file

// ---- CRC-32 (RFC 1952) of a block: every thread takes a slice, the slices are combined as polynomials ------------------------
__device__ inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {       // a(x) * b(x) mod P(x), reflected representation (zlib's multmodp)
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1u)) == 0u) break; }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
__device__ inline uint32_t crc_x8n(uint32_t nbytes, const uint32_t* x2n /* x^(2^k) mod P, k = 0..31 */) {        // x^(8 * nbytes) mod P
    uint32_t p = 1u << 31;                                            // the polynomial 1
    uint32_t n = nbytes;
    int k = 3;                                                        // bits -> bytes
    while (n) { if (n & 1u) p = crc_mulmod(x2n[k & 31], p); n >>= 1; ++k; }
    return p;
}
__device__ inline uint32_t crc_bytes(const uint8_t* d, uint32_t n, const uint32_t* tabl) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = tabl[(c ^ d[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// block-wide CRC of n bytes at src (global or LDS): slices of ceil(n / NTH) bytes
template <int NTH>
__device__ inline uint32_t block_crc(const uint8_t* src, uint32_t n, const uint32_t* tabl, const uint32_t* x2n, uint32_t* sh /* [NTH / 64] */) {
    const uint32_t per = (n + NTH - 1) / NTH;
    const uint32_t a = threadIdx.x * per < n ? threadIdx.x * per : n, b = a + per < n ? a + per : n;
    uint32_t c = 0;
    if (b > a) { c = crc_bytes(src + a, b - a, tabl); if (n - b) c = crc_mulmod(crc_x8n(n - b, x2n), c); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) r ^= sh[w];
    __syncthreads();
    return r;
}

size_t deflate_scratch_bytes(uint64_t batch);       // scratch for `batch` blocks or pieces per launch (levels 1 and 2; none needed for level 0)
// nblocks BGZF blocks of raw[0, nraw) -> comp (BGZF_STRIDE apart), their sizes -> csize; `batch` blocks per deflate launch
hipError_t bgzf_launch(const uint8_t* raw, uint64_t nraw, uint64_t nblocks, int level, const CrcTabs* ct, uint8_t* comp, uint64_t* csize, uint32_t* scratch,
                       uint64_t batch, hipStream_t st);
// the compressed blocks, packed: block b of comp -> out[coff[b], coff[b + 1])
hipError_t bgzf_pack(const uint8_t* comp, const uint64_t* coff, uint64_t nblocks, uint8_t* out, hipStream_t st);
// npieces pieces of raw -> comp (kZsStride apart), their sizes -> csize, their Adler-32 -> zp.adler
hipError_t zs_deflate(const uint8_t* raw, ZsPieces zp, uint64_t npieces, int level, uint8_t* comp, uint64_t* csize, uint32_t* scratch, uint64_t batch, hipStream_t st);

}  // namespace mkt
