// mkt_hic.hip -- the .hic container (include/mkt.h has the definition) from the resident cells of a matrix object: regroup the cells of
// every resolution by chromosome pair and block, serialise the blocks, deflate them into zlib streams (mkt_deflate.h: the LZ77 + Huffman
// stage of mkt_deflate.hip under its zlib framing) and place them in the file image; the host writes the header, the matrix records, the
// footer and the normalisation vectors around them.  The entry points (mkt_matrix_hic, .._fetch_hic) are at the end (mkt_matrix_obj.h).
//
// Per resolution, from cells that are strictly ascending in (bin1, bin2), that is in (pair, x, y):
//  * the order (pair, blockNumber, y, x) by STABLE radix passes (launch_radix64) over  composite << ib | cell index, composite =
//    c1 | c2 | blockNumber | y mod bb.  x is not part of the key: cells that agree on the composite differ in x only and are in ascending
//    x already.  The composite is as wide as the resolution needs (no bits for one chromosome, one block column, ...); where it does not
//    fit beside the index it is sorted in chunks from the low end, the keys of the next chunk rebuilt through the index in between.
//  * k_hic_gather: the sorted cells as (pair << 32 | blockNumber, y mod bb << 16 | x mod bb, count) and the head flags of blocks and rows,
//    which one exclusive scan turns into block and row ordinals.
//  * k_hic_heads: where every block and row starts.  k_hic_blocks: a wave per block, the largest count (useShort) and the exact sum of its
//    counts by a fixed tree, and the payload size in closed form.  Two scans: payload offsets (multiples of 16) and first pieces.
//  * k_hic_serialise: one lane per record writes its record, a row head its row header, a block head the block header; 16-bit stores.
//  * zs_deflate over the piece table, k_hic_streams (stream sizes, Adler-32 of the pieces joined), and when the host has laid the file
//    out k_hic_pack: a workgroup per block copies 78 9C, the pieces, 03 00 and the Adler-32 to the block's place.
// Integers only, no atomics: the bytes depend on the multiset of pairs and the options.
#include <hip/hip_runtime.h>

#include <stdarg.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>

#include "mkt_matrix_obj.h"
#include "mkt_launch.h"
#include "mkt_segred.h"
#include "mkt_deflate.h"

namespace mkt {

constexpr int HWG = 256;

struct HicGeo {
    const uint32_t *b1, *b2, *cnt, *off, *len;       // the cells; first bin and length of a chromosome
    const uint16_t* chr;
    uint64_t n;
    uint32_t r, bb;
    int cb, bnb, ylb;                                // bits of a chromosome index, a block number, y mod bb
};
struct HicCell { uint32_t pair, bn, yl, xl; };
__device__ inline uint32_t hic_bcc(const HicGeo& g, uint32_t c1, uint32_t c2) {
    const uint32_t l1 = g.len[c1], l2 = g.len[c2];
    return (l1 > l2 ? l1 : l2) / g.r / g.bb + 1u;
}
__device__ inline HicCell hic_cell(const HicGeo& g, uint64_t i) {
    const uint32_t a = g.b1[i], b = g.b2[i];
    const uint32_t c1 = g.chr[a], c2 = g.chr[b];
    const uint32_t x = a - g.off[c1], y = b - g.off[c2];
    HicCell c;
    c.pair = (c1 << g.cb) | c2;
    c.bn = (y / g.bb) * hic_bcc(g, c1, c2) + x / g.bb;
    c.yl = y % g.bb; c.xl = x % g.bb;
    return c;
}
// bits [from, from + nb) of the composite, above the cell index
__global__ __launch_bounds__(HWG) void k_hic_keys(HicGeo g, const uint64_t* prev, int ib, int from, int nb, uint64_t* key) {
    const uint64_t j = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (j >= g.n) return;
    const uint64_t imask = (1ull << ib) - 1ull;
    const uint64_t i = prev ? (prev[j] & imask) : j;
    const HicCell c = hic_cell(g, i);
    const unsigned __int128 comp = ((unsigned __int128)c.pair << (g.bnb + g.ylb)) | ((uint64_t)c.bn << g.ylb) | (uint64_t)c.yl;
    const uint64_t f = nb ? ((uint64_t)(comp >> from) & (nb >= 64 ? ~0ull : ((1ull << nb) - 1ull))) : 0ull;
    key[j] = (ib < 64 ? (f << ib) : 0ull) | i;
}
__global__ __launch_bounds__(HWG) void k_hic_gather(HicGeo g, const uint64_t* key, int ib, uint64_t* bk, uint32_t* yx, uint32_t* c, uint64_t* flag) {
    const uint64_t j = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (j >= g.n) return;
    const uint64_t imask = (1ull << ib) - 1ull;
    const uint64_t i = key[j] & imask;
    const HicCell me = hic_cell(g, i);
    bool bh = true, rh = true;
    if (j) {
        const HicCell p = hic_cell(g, key[j - 1] & imask);
        bh = p.pair != me.pair || p.bn != me.bn;
        rh = bh || p.yl != me.yl;
    }
    bk[j] = ((uint64_t)me.pair << 32) | me.bn;
    yx[j] = (me.yl << 16) | me.xl;
    c[j] = g.cnt[i];
    flag[j] = (bh ? 1ull : 0ull) | (rh ? 1ull << 32 : 0ull);
}
struct HicOrd { uint32_t b, row; bool bh, rh; };
// ordinals of record j from the scanned flags
__device__ inline HicOrd hic_ord(const uint64_t* bk, const uint32_t* yx, const uint64_t* scan, uint64_t j) {
    HicOrd o;
    o.bh = j == 0 || bk[j] != bk[j - 1];
    o.rh = o.bh || (yx[j] >> 16) != (yx[j - 1] >> 16);
    const uint64_t s = scan[j];
    o.b = (uint32_t)s + (o.bh ? 1u : 0u) - 1u;
    o.row = (uint32_t)(s >> 32) + (o.rh ? 1u : 0u) - 1u;
    return o;
}
// bstart[nblk + 1], brow[nblk + 1], rstart[nrows + 1]; the last record also writes the three ends
__global__ __launch_bounds__(HWG) void k_hic_heads(const uint64_t* bk, const uint32_t* yx, const uint64_t* scan, uint64_t n, uint32_t* bstart, uint32_t* brow, uint64_t* bkey, uint32_t* rstart) {
    const uint64_t j = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (j >= n) return;
    const HicOrd o = hic_ord(bk, yx, scan, j);
    if (o.bh) { bstart[o.b] = (uint32_t)j; brow[o.b] = o.row; bkey[o.b] = bk[j]; }
    if (o.rh) rstart[o.row] = (uint32_t)j;
    if (j == n - 1) { bstart[o.b + 1] = (uint32_t)n; brow[o.b + 1] = o.row + 1u; rstart[o.row + 1] = (uint32_t)n; }
}
// a wave per block: largest count, sum of the counts; payload bytes, their room (a multiple of 16) and the pieces
__global__ __launch_bounds__(HWG) void k_hic_blocks(const uint32_t* c, const uint32_t* bstart, const uint32_t* brow, uint64_t nblk, uint32_t* bmax, uint64_t* bsum,
                                                    uint64_t* psize, uint64_t* poff, uint64_t* pfirst) {
    const uint64_t b = ((uint64_t)blockIdx.x * HWG + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (b >= nblk) return;                                                       // (whole waves)
    const uint32_t s = bstart[b], e = bstart[b + 1];
    uint32_t mx = 0;
    unsigned long long sum = 0;
    for (uint32_t j = s + lane; j < e; j += 64) { const uint32_t v = c[j]; mx = mx > v ? mx : v; sum += v; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = (uint32_t)__shfl_down((int)mx, d, 64);
        mx = mx > y ? mx : y;
        sum += (unsigned long long)__shfl_down((long long)sum, d, 64);
    }
    if (lane == 0) {
        const uint64_t rows = brow[b + 1] - brow[b], recs = e - s;
        const uint64_t bytes = 16 + 4 * rows + recs * (mx <= kHicCountShort ? 4 : 6);
        bmax[b] = mx; bsum[b] = sum; psize[b] = bytes;
        poff[b] = (bytes + 15) & ~15ull;
        pfirst[b] = (bytes + kZsPiece - 1) / kZsPiece;
    }
}
__global__ __launch_bounds__(HWG) void k_hic_pieces(const uint64_t* psize, const uint64_t* poff, const uint64_t* pfirst, uint64_t nblk, uint64_t* piece_off, uint32_t* piece_len) {
    const uint64_t b = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (b >= nblk) return;
    const uint64_t bytes = psize[b], p0 = pfirst[b], np = pfirst[b + 1] - p0;
    for (uint64_t k = 0; k < np; ++k) {
        piece_off[p0 + k] = poff[b] + k * kZsPiece;
        piece_len[p0 + k] = (uint32_t)(bytes - k * kZsPiece < kZsPiece ? bytes - k * kZsPiece : kZsPiece);
    }
}
__device__ inline void put16(uint8_t* p, uint32_t v) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)v; }      // (every field of a payload is on an even offset)
__device__ inline void put32h(uint8_t* p, uint32_t v) { put16(p, v); put16(p + 2, v >> 16); }
__global__ __launch_bounds__(HWG) void k_hic_serialise(HicGeo g, const uint64_t* bk, const uint32_t* yx, const uint32_t* c, const uint64_t* scan, const uint32_t* bstart, const uint32_t* brow,
                                                       const uint32_t* rstart, const uint32_t* bmax, const uint64_t* poff, uint8_t* raw) {
    const uint64_t j = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (j >= g.n) return;
    const HicOrd o = hic_ord(bk, yx, scan, j);
    const bool us = bmax[o.b] <= kHicCountShort;
    const uint64_t rs = us ? 4 : 6, k = j - bstart[o.b], rib = o.row - brow[o.b];
    uint8_t* base = raw + poff[o.b];
    const uint32_t v = yx[j], cnt = c[j];
    uint8_t* p = base + 16 + 4 * (rib + 1) + rs * k;
    put16(p, v & 0xFFFFu);
    if (us) put16(p + 2, cnt); else put32h(p + 2, __float_as_uint((float)cnt));
    if (o.rh) { uint8_t* q = p - 4; put16(q, v >> 16); put16(q + 2, rstart[o.row + 1] - (uint32_t)j); }
    if (o.bh) {
        const uint64_t key = bk[j];
        const uint32_t pair = (uint32_t)(key >> 32), bn = (uint32_t)key;
        const uint32_t bcc = hic_bcc(g, pair >> g.cb, pair & ((1u << g.cb) - 1u));
        put32h(base, bstart[o.b + 1] - bstart[o.b]);
        put32h(base + 4, (bn % bcc) * g.bb);
        put32h(base + 8, (bn / bcc) * g.bb);
        put16(base + 12, (us ? 1u : 0u) | (1u << 8));                             // useShort, matrixType 1
        put16(base + 14, brow[o.b + 1] - brow[o.b]);
    }
}
// per block: the bytes of its stream and the Adler-32 of its payload
__global__ __launch_bounds__(HWG) void k_hic_streams(const uint64_t* pfirst, const uint64_t* csize, const uint32_t* piece_len, const uint32_t* adler, uint64_t nblk, uint64_t* ssize, uint32_t* sadler) {
    const uint64_t b = (uint64_t)blockIdx.x * HWG + threadIdx.x;
    if (b >= nblk) return;
    const uint64_t p0 = pfirst[b], p1 = pfirst[b + 1];
    uint64_t bytes = kZsFrame;
    uint32_t ad = 1;                                                             // of no bytes
    for (uint64_t p = p0; p < p1; ++p) { bytes += csize[p]; ad = zs_adler_join(ad, adler[p], piece_len[p]); }
    ssize[b] = bytes; sadler[b] = ad;
}
__global__ __launch_bounds__(HWG) void k_hic_pack(const uint8_t* comp, const uint64_t* pfirst, const uint64_t* csize, const uint32_t* sadler, const uint64_t* fpos, uint8_t* image) {
    const uint64_t b = blockIdx.x;
    uint8_t* d = image + fpos[b];
    uint64_t o = 2;
    for (uint64_t p = pfirst[b]; p < pfirst[b + 1]; ++p) {
        const uint8_t* s = comp + p * kZsStride;
        const uint32_t n = (uint32_t)csize[p];
        for (uint32_t i = threadIdx.x; i < n; i += HWG) d[o + i] = s[i];
        o += n;
    }
    if (threadIdx.x == 0) {
        const uint32_t ad = sadler[b];
        d[0] = 0x78; d[1] = 0x9C;
        d[o] = 3; d[o + 1] = 0;
        d[o + 2] = (uint8_t)(ad >> 24); d[o + 3] = (uint8_t)(ad >> 16); d[o + 4] = (uint8_t)(ad >> 8); d[o + 5] = (uint8_t)ad;
    }
}

// ---------------------------------------------------------------------------------------------------------------
static int hic_fail(std::string* why, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static int hic_fail(std::string* why, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (why) *why = buf;
    return code;
}
#define HIC_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hic_fail(why, e_ == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "hic: HIP call failed: %s", hipGetErrorString(e_)); } while (0)
static int hic_bits(uint64_t n) { int b = 0; while (b < 64 && (1ull << b) < n) ++b; return b; }          // the bits that hold 0 .. n - 1

namespace {
struct HicBlk { uint64_t key; uint64_t ssize, psize, sum; uint32_t mx; };
struct HicResDev {                                   // what a resolution keeps until the file is laid out
    uint64_t nblk = 0, npieces = 0;
    DevBuf<uint8_t> comp;
    DevBuf<uint64_t> csize, pfirst, fpos;
    DevBuf<uint32_t> sadler;
    std::vector<HicBlk> blk;                         // ascending in (pair, blockNumber)
};
struct Bytes {
    std::vector<uint8_t> v;
    void raw(const void* p, size_t n) { const uint8_t* q = (const uint8_t*)p; v.insert(v.end(), q, q + n); }
    void i32(int32_t x) { raw(&x, 4); }
    void i64(int64_t x) { raw(&x, 8); }
    void f32(float x) { raw(&x, 4); }
    void str(const std::string& s) { raw(s.data(), s.size()); v.push_back(0); }
};
}  // namespace

// one resolution: its blocks serialised and deflated on the device, their table on the host
static int hic_resolution(const HicResIn& in, const std::vector<uint32_t>& lens, const uint32_t* d_len, const mkt_hic_opts& o, hipStream_t st, HicResDev& out, HicTiming& tm, std::string* why) {
    const uint64_t n = in.cells.nnz;
    if (n == 0) return MKT_OK;
    if (n >= (1ull << 32)) return hic_fail(why, MKT_E_CAPACITY, "hic: %llu cells at %u bp: fewer than 2^32 are needed (cell indices are 32-bit)", (unsigned long long)n, in.bin_size);
    const uint32_t nchr = (uint32_t)lens.size(), bb = o.block_bins;
    uint32_t maxlen = 0;
    for (uint32_t l : lens) maxlen = std::max(maxlen, l);
    const uint64_t bccmax = (uint64_t)maxlen / in.bin_size / bb + 1;
    if (bccmax * bccmax > 0x7FFFFFFFull) return hic_fail(why, MKT_E_CAPACITY, "hic: %llu block columns at %u bp and %u bins per block: block numbers do not fit 31 bits (use larger blocks)", (unsigned long long)bccmax, in.bin_size, bb);
    HicGeo g;
    g.b1 = in.cells.b1; g.b2 = in.cells.b2; g.cnt = in.cells.cnt; g.off = in.cells.off; g.len = d_len; g.chr = in.chr;
    g.n = n; g.r = in.bin_size; g.bb = bb;
    g.cb = hic_bits(nchr); g.bnb = hic_bits(bccmax * bccmax);
    g.ylb = hic_bits(std::min<uint64_t>(bb, (uint64_t)maxlen / in.bin_size + 1));
    const int ib = std::max(1, hic_bits(n)), W = 2 * g.cb + g.bnb + g.ylb, K = 64 - ib;
    DevEvents<5> ev;
    HIC_HIP(ev.create());
    const unsigned grid = grid_for(n, HWG);

    // ---- the order
    DevBuf<uint64_t> kA, kB, scan;
    DevBuf<uint32_t> radix, yx, cc;
    HIC_HIP(kA.alloc(n, 64)); HIC_HIP(kB.alloc(n, 64)); HIC_HIP(scan.alloc(n + 1)); HIC_HIP(yx.alloc(n)); HIC_HIP(cc.alloc(n));
    HIC_HIP(radix.alloc(0, radix64_count_bytes(n)));
    uint64_t *pA = kA, *pB = kB;
    HIC_HIP(hipEventRecord(ev[0], st));
    for (int from = 0, first = 1; first || from < W; first = 0) {
        const int nb = std::min(K, W - from);
        hipLaunchKernelGGL(k_hic_keys, dim3(grid), dim3(HWG), 0, st, g, first ? (const uint64_t*)nullptr : (const uint64_t*)pA, ib, from, nb, pA);
        HIC_HIP(hipGetLastError());
        if (nb) HIC_HIP(launch_radix64(pA, pB, n, ib, nb, radix, st));
        from += nb;
        if (nb == 0) break;
    }
    uint64_t* bk = pB;                                                           // (the other key buffer is free again)
    hipLaunchKernelGGL(k_hic_gather, dim3(grid), dim3(HWG), 0, st, g, (const uint64_t*)pA, ib, bk, yx.get(), cc.get(), scan.get());
    HIC_HIP(hipGetLastError());
    HIC_HIP(launch_exscan(scan, n, scan.get() + n, st));
    uint64_t tot = 0;
    HIC_HIP(hipMemcpyAsync(&tot, scan.get() + n, 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipEventRecord(ev[1], st));
    HIC_HIP(hipStreamSynchronize(st));
    const uint64_t nblk = tot & 0xFFFFFFFFull, nrows = tot >> 32;
    if (nblk == 0 || nblk > nrows || nrows > n) return hic_fail(why, MKT_E_KERNEL, "hic: %llu blocks and %llu rows from %llu cells", (unsigned long long)nblk, (unsigned long long)nrows, (unsigned long long)n);

    // ---- block and row tables, payload sizes, the piece table
    DevBuf<uint32_t> bstart, brow, rstart, bmax, piece_len, adler;
    DevBuf<uint64_t> bkey, bsum, psize, poff, piece_off, ssize;
    HIC_HIP(bstart.alloc(nblk + 1)); HIC_HIP(brow.alloc(nblk + 1)); HIC_HIP(rstart.alloc(nrows + 1)); HIC_HIP(bmax.alloc(nblk));
    HIC_HIP(bkey.alloc(nblk)); HIC_HIP(bsum.alloc(nblk)); HIC_HIP(psize.alloc(nblk)); HIC_HIP(poff.alloc(nblk + 1)); HIC_HIP(out.pfirst.alloc(nblk + 1)); HIC_HIP(ssize.alloc(nblk));
    hipLaunchKernelGGL(k_hic_heads, dim3(grid), dim3(HWG), 0, st, (const uint64_t*)bk, (const uint32_t*)yx, (const uint64_t*)scan, n, bstart.get(), brow.get(), bkey.get(), rstart.get());
    hipLaunchKernelGGL(k_hic_blocks, dim3(grid_for(nblk * 64, HWG)), dim3(HWG), 0, st, (const uint32_t*)cc, (const uint32_t*)bstart, (const uint32_t*)brow, nblk, bmax.get(), bsum.get(),
                       psize.get(), poff.get(), out.pfirst.get());
    HIC_HIP(hipGetLastError());
    HIC_HIP(launch_exscan(poff, nblk, poff.get() + nblk, st));
    HIC_HIP(launch_exscan(out.pfirst, nblk, out.pfirst.get() + nblk, st));
    uint64_t raw_room = 0, npieces = 0;
    HIC_HIP(hipMemcpyAsync(&raw_room, poff.get() + nblk, 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipMemcpyAsync(&npieces, out.pfirst.get() + nblk, 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipStreamSynchronize(st));
    if (npieces < nblk || npieces > raw_room / 16 + nblk) return hic_fail(why, MKT_E_KERNEL, "hic: %llu pieces for %llu blocks of %llu bytes", (unsigned long long)npieces, (unsigned long long)nblk, (unsigned long long)raw_room);
    DevBuf<uint8_t> raw;
    HIC_HIP(raw.alloc(raw_room, 64));
    HIC_HIP(piece_off.alloc(npieces)); HIC_HIP(piece_len.alloc(npieces)); HIC_HIP(adler.alloc(npieces));
    HIC_HIP(out.comp.alloc(npieces * (uint64_t)kZsStride, 64)); HIC_HIP(out.csize.alloc(npieces)); HIC_HIP(out.sadler.alloc(nblk));
    const uint64_t batch = std::min<uint64_t>(npieces, 1024);
    DevBuf<uint32_t> scratch;
    if (o.level > 0) HIC_HIP(scratch.alloc(0, deflate_scratch_bytes(batch)));
    HIC_HIP(hipMemsetAsync(raw, 0, raw_room + 64, st));                          // (the room between payloads: read by the 16-byte loads, never coded)
    hipLaunchKernelGGL(k_hic_pieces, dim3(grid_for(nblk, HWG)), dim3(HWG), 0, st, (const uint64_t*)psize, (const uint64_t*)poff, (const uint64_t*)out.pfirst, nblk, piece_off.get(), piece_len.get());
    hipLaunchKernelGGL(k_hic_serialise, dim3(grid), dim3(HWG), 0, st, g, (const uint64_t*)bk, (const uint32_t*)yx, (const uint32_t*)cc, (const uint64_t*)scan, (const uint32_t*)bstart,
                       (const uint32_t*)brow, (const uint32_t*)rstart, (const uint32_t*)bmax, (const uint64_t*)poff, raw.get());
    HIC_HIP(hipGetLastError());
    HIC_HIP(hipEventRecord(ev[2], st));
    const ZsPieces zp{piece_off, piece_len, adler};
    HIC_HIP(zs_deflate(raw, zp, npieces, o.level, out.comp, out.csize, scratch, batch, st));
    hipLaunchKernelGGL(k_hic_streams, dim3(grid_for(nblk, HWG)), dim3(HWG), 0, st, (const uint64_t*)out.pfirst, (const uint64_t*)out.csize, (const uint32_t*)piece_len, (const uint32_t*)adler, nblk,
                       ssize.get(), out.sadler.get());
    HIC_HIP(hipGetLastError());
    HIC_HIP(hipEventRecord(ev[3], st));
    std::vector<uint64_t> hkey(nblk), hss(nblk), hps(nblk), hsum(nblk);
    std::vector<uint32_t> hmx(nblk);
    HIC_HIP(hipMemcpyAsync(hkey.data(), bkey, nblk * 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipMemcpyAsync(hss.data(), ssize, nblk * 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipMemcpyAsync(hps.data(), psize, nblk * 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipMemcpyAsync(hsum.data(), bsum, nblk * 8, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipMemcpyAsync(hmx.data(), bmax, nblk * 4, hipMemcpyDeviceToHost, st));
    HIC_HIP(hipStreamSynchronize(st));
    float ms = 0;
    HIC_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); tm.sort_ms = ms;
    HIC_HIP(hipEventElapsedTime(&ms, ev[1], ev[2])); tm.serialise_ms = ms;
    HIC_HIP(hipEventElapsedTime(&ms, ev[2], ev[3])); tm.deflate_ms = ms;
    out.nblk = nblk; out.npieces = npieces;
    out.blk.resize(nblk);
    for (uint64_t b = 0; b < nblk; ++b) {
        out.blk[b] = HicBlk{hkey[b], hss[b], hps[b], hsum[b], hmx[b]};
        if (b && hkey[b] <= hkey[b - 1]) return hic_fail(why, MKT_E_KERNEL, "hic: the blocks at %u bp are not in ascending order", in.bin_size);
        if (hss[b] >= (1ull << 31)) return hic_fail(why, MKT_E_CAPACITY, "hic: a block at %u bp deflates to %llu bytes: fewer than 2^31 are needed (use smaller blocks)", in.bin_size, (unsigned long long)hss[b]);
    }
    return MKT_OK;
}

int hic_build(HicState& s, const std::vector<HicResIn>& res, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const mkt_hic_opts& o, hipStream_t st, std::string* why) {
    s = HicState();
    const uint32_t nchr = (uint32_t)lens.size(), nres = (uint32_t)res.size();
    for (uint32_t c = 0; c < nchr; ++c)
        if (lens[c] >= (1u << 31)) return hic_fail(why, MKT_E_CAPACITY, "hic: chromosome %s of %u bp: lengths below 2^31 are needed (int32 in the file)", names[c].c_str(), lens[c]);
    // the resolutions in descending bin size: the zoom index
    std::vector<uint32_t> zoom(nres);
    for (uint32_t k = 0; k < nres; ++k) zoom[k] = k;
    std::sort(zoom.begin(), zoom.end(), [&](uint32_t a, uint32_t b) { return res[a].bin_size > res[b].bin_size; });
    for (uint32_t z = 1; z < nres; ++z)
        if (res[zoom[z]].bin_size == res[zoom[z - 1]].bin_size) return hic_fail(why, MKT_E_ARG, "hic: the bin size %u is there twice", res[zoom[z]].bin_size);
    const std::string genome = o.genome_id ? o.genome_id : "", label = o.norm_label ? o.norm_label : "ICE";

    DevBuf<uint32_t> d_len;
    HIC_HIP(d_len.alloc(nchr));
    HIC_HIP(hipMemcpyAsync(d_len, lens.data(), (size_t)nchr * 4, hipMemcpyHostToDevice, st));
    std::vector<HicResDev> dev(nres);
    std::vector<HicTiming> timing(nres);
    for (uint32_t k = 0; k < nres; ++k)
        if (const int rc = hic_resolution(res[k], lens, d_len, o, st, dev[k], timing[k], why)) return rc;

    // ---- the layout.  Per pair and zoom index: the range of its blocks in the resolution's table
    const int cb = hic_bits(nchr);
    struct Range { uint64_t first = 0, n = 0; };
    std::map<uint32_t, std::vector<Range>> pairs;                                // c1 << cb | c2, ascending = ascending (c1, c2)
    for (uint32_t z = 0; z < nres; ++z) {
        const HicResDev& d = dev[zoom[z]];
        for (uint64_t b = 0; b < d.nblk; ++b) {
            std::vector<Range>& v = pairs[(uint32_t)(d.blk[b].key >> 32)];
            if (v.empty()) v.resize(nres);
            if (v[z].n++ == 0) v[z].first = b;
        }
    }
    Bytes head;
    head.raw("HIC\0", 4); head.i32(8); head.i64(0); head.str(genome);
    head.i32(1); head.str("software"); head.str("microcket-mi355x");
    head.i32((int32_t)nchr);
    for (uint32_t c = 0; c < nchr; ++c) { head.str(names[c]); head.i32((int32_t)lens[c]); }
    head.i32((int32_t)nres);
    for (uint32_t z = 0; z < nres; ++z) head.i32((int32_t)res[zoom[z]].bin_size);
    head.i32(0);
    // a position and a size per pair; the records themselves once the positions are known
    mkt_hic_info info;
    memset(&info, 0, sizeof info);
    std::vector<std::vector<uint64_t>> fpos(nres);
    for (uint32_t k = 0; k < nres; ++k) fpos[k].resize(dev[k].nblk);
    struct Rec { uint64_t pos; Bytes b; uint64_t total; };
    std::vector<Rec> recs;
    Bytes foot;
    foot.i32((int32_t)pairs.size());
    uint64_t pos = head.v.size();
    for (const auto& kv : pairs) {
        const uint32_t c1 = kv.first >> cb, c2 = kv.first & ((1u << cb) - 1u);
        uint64_t nb_all = 0;
        for (const Range& r : kv.second) nb_all += r.n;
        Rec rec;
        rec.pos = pos;
        uint64_t at = pos + 12 + (uint64_t)nres * 39 + nb_all * 16;              // the first block
        rec.b.i32((int32_t)c1); rec.b.i32((int32_t)c2); rec.b.i32((int32_t)nres);
        for (uint32_t z = 0; z < nres; ++z) {
            const HicResDev& d = dev[zoom[z]];
            const Range& r = kv.second[z];
            const uint32_t bs = res[zoom[z]].bin_size;
            uint64_t sum = 0;
            for (uint64_t b = r.first; b < r.first + r.n; ++b) sum += d.blk[b].sum;
            rec.b.str("BP"); rec.b.i32((int32_t)z); rec.b.f32((float)sum); rec.b.f32(0); rec.b.f32(0); rec.b.f32(0);
            rec.b.i32((int32_t)bs); rec.b.i32((int32_t)o.block_bins);
            rec.b.i32((int32_t)(std::max(lens[c1], lens[c2]) / bs / o.block_bins + 1));
            rec.b.i32((int32_t)r.n);
            for (uint64_t b = r.first; b < r.first + r.n; ++b) {
                const HicBlk& x = d.blk[b];
                rec.b.i32((int32_t)(uint32_t)x.key); rec.b.i64((int64_t)at); rec.b.i32((int32_t)x.ssize);
                fpos[zoom[z]][b] = at;
                at += x.ssize;
                info.blocks++; info.float_blocks += x.mx > kHicCountShort; info.raw_bytes += x.psize; info.deflated_bytes += x.ssize;
            }
        }
        rec.total = at - pos;
        char keyname[32];
        snprintf(keyname, sizeof keyname, "%u_%u", c1, c2);
        foot.str(keyname); foot.i64((int64_t)rec.pos); foot.i32((int32_t)rec.total);
        if (rec.total >= (1ull << 31)) return hic_fail(why, MKT_E_CAPACITY, "hic: the matrix of %s and %s takes %llu bytes: fewer than 2^31 are needed (int32 in the master index)", names[c1].c_str(), names[c2].c_str(), (unsigned long long)rec.total);
        pos = at;
        recs.push_back(std::move(rec));
    }
    info.matrices = pairs.size();
    for (const HicResDev& d : dev) info.pieces += d.npieces;
    const uint64_t footer_pos = pos;
    foot.i32(0); foot.i32(0);
    // the normalisation vectors: per balanced resolution in header order, per chromosome in table order
    std::vector<std::vector<double>> vecs;
    struct VecAt { uint32_t z, chr; uint64_t n; const double* v; };
    std::vector<VecAt> vat;
    if (o.norm) {
        for (uint32_t z = 0; z < nres; ++z) {
            const HicResIn& in = res[zoom[z]];
            if (!in.d_w) continue;
            vecs.emplace_back(in.cells.nbins);
            std::vector<double>& w = vecs.back();
            HIC_HIP(hipMemcpyAsync(w.data(), in.d_w, in.cells.nbins * 8, hipMemcpyDeviceToHost, st));
            HIC_HIP(hipStreamSynchronize(st));
            const double qnan = __builtin_nan("");
            for (double& x : w) x = x != x ? qnan : 1.0 / x;                      // .hic vectors divide; one canonical NaN
            for (uint32_t c = 0; c < nchr; ++c) {
                const uint64_t lo = (*in.off)[c], hi = c + 1 < nchr ? (*in.off)[c + 1] : in.cells.nbins;
                vat.push_back(VecAt{z, c, hi - lo, w.data() + lo});
            }
        }
    }
    foot.i32((int32_t)vat.size());
    uint64_t index_bytes = 0;
    for (const VecAt& a : vat) { (void)a; index_bytes += label.size() + 1 + 4 + 3 + 4 + 8 + 4; }
    uint64_t vpos = footer_pos + 4 + foot.v.size() + index_bytes;
    const int32_t nbytes = (int32_t)(foot.v.size() + index_bytes);
    for (const VecAt& a : vat) {
        const uint64_t bytes = 4 + a.n * 8;
        if (bytes >= (1ull << 31)) return hic_fail(why, MKT_E_CAPACITY, "hic: a normalisation vector of %llu values does not fit the int32 of its index entry", (unsigned long long)a.n);
        foot.str(label); foot.i32((int32_t)a.chr); foot.str("BP"); foot.i32((int32_t)res[zoom[a.z]].bin_size); foot.i64((int64_t)vpos); foot.i32((int32_t)bytes);
        vpos += bytes;
    }
    if (foot.v.size() >= (1ull << 31)) return hic_fail(why, MKT_E_CAPACITY, "hic: a footer of %zu bytes does not fit the int32 of nBytes", foot.v.size());
    Bytes tail;
    tail.i32(nbytes);
    tail.raw(foot.v.data(), foot.v.size());
    for (const VecAt& a : vat) { tail.i32((int32_t)a.n); tail.raw(a.v, a.n * 8); }
    const uint64_t file_bytes = footer_pos + tail.v.size();
    memcpy(head.v.data() + 8, &footer_pos, 8);

    // ---- the image
    HIC_HIP(s.image.alloc(file_bytes, 64));
    HIC_HIP(hipMemcpyAsync(s.image, head.v.data(), head.v.size(), hipMemcpyHostToDevice, st));
    for (const Rec& r : recs) HIC_HIP(hipMemcpyAsync(s.image.get() + r.pos, r.b.v.data(), r.b.v.size(), hipMemcpyHostToDevice, st));
    HIC_HIP(hipMemcpyAsync(s.image.get() + footer_pos, tail.v.data(), tail.v.size(), hipMemcpyHostToDevice, st));
    DevEvents<2> ev;
    HIC_HIP(ev.create());
    for (uint32_t k = 0; k < nres; ++k) {
        HicResDev& d = dev[k];
        if (d.nblk == 0) continue;
        HIC_HIP(d.fpos.alloc(d.nblk));
        HIC_HIP(hipMemcpyAsync(d.fpos, fpos[k].data(), d.nblk * 8, hipMemcpyHostToDevice, st));
        HIC_HIP(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(k_hic_pack, dim3((unsigned)d.nblk), dim3(HWG), 0, st, (const uint8_t*)d.comp, (const uint64_t*)d.pfirst, (const uint64_t*)d.csize, (const uint32_t*)d.sadler,
                           (const uint64_t*)d.fpos, s.image.get());
        HIC_HIP(hipGetLastError());
        HIC_HIP(hipEventRecord(ev[1], st));
        HIC_HIP(hipStreamSynchronize(st));
        float ms = 0;
        HIC_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        timing[k].pack_ms = ms;
    }
    HIC_HIP(hipStreamSynchronize(st));                                           // (the host buffers of the copies above go out of scope)
    info.file_bytes = file_bytes;
    s.info = info;
    s.timing = std::move(timing);
    s.built = true;
    return MKT_OK;
}

}  // namespace mkt

// ---- the entry points -----------------------------------------------------------------------------------------------------------
using namespace mkt;
extern "C" {

void mkt_hic_opts_default(mkt_hic_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->block_bins = 1000; o->level = 2; o->norm = 1;
}

int mkt_matrix_hic(mkt_matrix* m, const mkt_hic_opts* opts, mkt_hic_info* info) {
    if (!m) return MKT_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    const mkt_hic_opts o = mx_opts(opts, mkt_hic_opts_default);
    if (o.block_bins < 1 || o.block_bins > kHicBlockBinsMax) return mfail(m, MKT_E_ARG, "hic: block_bins %u (1 .. %u: block coordinates are int16)", o.block_bins, kHicBlockBinsMax);
    if (o.level < 0 || o.level > 2) return mfail(m, MKT_E_ARG, "hic: level %d (0 stored, 1 fixed codes, 2 dynamic codes)", o.level);
    if (o.norm != 0 && o.norm != 1) return mfail(m, MKT_E_ARG, "hic: norm %d (0 or 1)", o.norm);
    if (o.reserved != 0) return mfail(m, MKT_E_ARG, "hic: the reserved field is not 0");
    if (o.norm_label && !*o.norm_label) return mfail(m, MKT_E_ARG, "hic: an empty norm_label");
    if (!m->ran) return mfail(m, MKT_E_STATE, "hic before run");
    MCHK(m, hipSetDevice(m->device));
    std::vector<HicResIn> in(m->res.size());
    for (size_t k = 0; k < m->res.size(); ++k) {
        MxRes& r = m->res[k];
        if (r.nnz) MX(m, "hic: ", layout_chr(r.lay, mx_cells(r), m->stream));
        in[k].cells = mx_cells(r);
        in[k].chr = r.nnz ? r.lay.chr.get() : nullptr;
        in[k].off = &r.off;
        in[k].bin_size = r.r;
        in[k].d_w = r.balanced ? r.d_w.get() : nullptr;
    }
    HicState hs;                                                        // a refused or failed call leaves the previous file alone
    std::string why;
    const int rc = hic_build(hs, in, m->names, m->lens, o, m->stream, &why);
    if (rc != MKT_OK) return mfail(m, rc, "%s", why.c_str());
    m->hic = std::move(hs);
    if (info) *info = m->hic.info;
    return MKT_OK;
}

int mkt_matrix_fetch_hic(mkt_matrix* m, uint64_t off, char* out, size_t n) {
    if (!m || (n && !out)) return MKT_E_ARG;
    if (!(m->ran && m->hic.built)) return mfail(m, MKT_E_STATE, "no .hic file: hic first");
    const uint64_t fb = m->hic.info.file_bytes;
    if (off > fb || n > fb - off) return mfail(m, MKT_E_ARG, "range past the end of the .hic file");
    MCHK(m, hipSetDevice(m->device));
    if (n) MCHK(m, hipMemcpy(out, m->hic.image.get() + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

int mkt_matrix_hic_timing(const mkt_matrix* m, uint32_t res_index, double* sort_ms, double* serialise_ms, double* deflate_ms, double* pack_ms) {
    if (!m || res_index >= m->res.size()) return MKT_E_ARG;
    const bool have = m->ran && m->hic.built && res_index < m->hic.timing.size();
    const HicTiming t = have ? m->hic.timing[res_index] : HicTiming();
    mx_ms(sort_ms, have, t.sort_ms); mx_ms(serialise_ms, have, t.serialise_ms); mx_ms(deflate_ms, have, t.deflate_ms); mx_ms(pack_ms, have, t.pack_ms);
    return MKT_OK;
}

}  // extern "C"
