// mkt_deflate.hip -- the GPU deflate (RFC 1951) and its two framings (mkt_deflate.h): BGZF members for sam2bam (mkt_bam.hip) and
// pieces of zlib streams for the .hic writer (mkt_hic.hip).  One workgroup per block of at most BGZF_RAW bytes: LZ77 + Huffman codes
// (level 2: a code built per block; level 1: the fixed code; level 0: stored), the block's CRC-32 (RFC 1952) or Adler-32 (RFC 1950)
// made beside it.  The code construction is mkt_deflate_codes.h (shared with the host test driver).  Nothing here knows SAM, BAM or
// .hic.  Byte / integer work in LDS; no MFMA.
#include "mkt_deflate.h"
#include "mkt_deflate_codes.h"

namespace mkt {

constexpr int BWG = 256;

// block-wide Adler-32 (RFC 1950) of n <= 65 280 bytes at src, from the state (1, 0): slices of ceil(n / NTH) bytes; a slice [s, e) gives
// a = sum d_i and b = sum (e - i) d_i, and the whole is A = 1 + sum a, B = n + sum (b + (n - e) a), both mod 65521.  Integer sums in a
// fixed tree: the value does not depend on the order anything ran in.
template <int NTH>
__device__ inline uint32_t block_adler(const uint8_t* src, uint32_t n, uint32_t* sh /* [NTH / 64] */) {
    const uint32_t per = (n + NTH - 1) / NTH;                 // <= 256 bytes for NTH >= 256: a < 2^16, b < 2^24
    const uint32_t s = threadIdx.x * per < n ? threadIdx.x * per : n, e = s + per < n ? s + per : n;
    uint32_t a = 0, b = 0;
    for (uint32_t i = s; i < e; ++i) { a += src[i]; b += a; }
    uint32_t tb = (uint32_t)(((uint64_t)b + (uint64_t)(n - e) * a) % 65521u);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += (uint32_t)__shfl_xor((int)a, d, 64); tb += (uint32_t)__shfl_xor((int)tb, d, 64); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    uint32_t A = 1;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) A += sh[w];
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = tb;
    __syncthreads();
    uint32_t Bs = n;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) Bs += sh[w];
    __syncthreads();
    return ((Bs % 65521u) << 16) | (A % 65521u);
}
__device__ inline void bgzf_header(uint8_t* o, uint32_t bsize_minus1) {     // SAMv1 4.1
    const uint8_t h[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
    for (int i = 0; i < 16; ++i) o[i] = h[i];
    o[16] = (uint8_t)bsize_minus1; o[17] = (uint8_t)(bsize_minus1 >> 8);
}

// level 0: one stored deflate block per BGZF block
__global__ __launch_bounds__(BWG) void k_bgzf_stored(const uint8_t* raw, uint64_t nraw, const CrcTabs* ct, uint8_t* comp, uint64_t* csize) {
    __shared__ uint32_t tabl[256], x2n[32], sh[BWG / 64];
    tabl[threadIdx.x] = ct->t[threadIdx.x];
    if (threadIdx.x < 32) x2n[threadIdx.x] = ct->x2n[threadIdx.x];
    __syncthreads();
    const uint64_t b0 = (uint64_t)blockIdx.x * BGZF_RAW;
    const uint32_t n = (uint32_t)(nraw - b0 < BGZF_RAW ? nraw - b0 : BGZF_RAW);
    const uint8_t* src = raw + b0;
    uint8_t* o = comp + (uint64_t)blockIdx.x * BGZF_STRIDE;
    const uint32_t crc = block_crc<BWG>(src, n, tabl, x2n, sh);
    const uint32_t total = 18 + 5 + n + 8;
    if (threadIdx.x == 0) {
        bgzf_header(o, total - 1);
        o[18] = 1;                                         // BFINAL = 1, BTYPE = 00
        o[19] = (uint8_t)n; o[20] = (uint8_t)(n >> 8); o[21] = (uint8_t)~n; o[22] = (uint8_t)(~n >> 8);
        uint8_t* e = o + 23 + n;
        put32(e, crc); put32(e, n);
        csize[blockIdx.x] = total;
    }
    for (uint32_t i = threadIdx.x; i < n; i += BWG) o[23 + i] = src[i];
}
// the compressed blocks, packed
__global__ __launch_bounds__(BWG) void k_bgzf_pack(const uint8_t* comp, const uint64_t* coff, uint64_t nblocks, uint8_t* out) {
    const uint64_t b = blockIdx.x;
    const uint64_t o = coff[b], n = coff[b + 1] - o;
    const uint8_t* s = comp + b * BGZF_STRIDE;
    for (uint32_t i = threadIdx.x; i < n; i += BWG) out[o + i] = s[i];
}

// ---- levels 1 and 2: LZ77 + Huffman codes (RFC 1951), one workgroup per BGZF block ------------------------------------------
// Every wave parses its share of the block (an eighth by default) with its own hash table (matches stay inside the share), 64
// positions per step: a hash of four bytes names a candidate from earlier steps (distance 1 first, for runs), checked on four
// bytes in parallel; then the greedy parse of the step token by token -- literals skipped in bulk, a match's length measured
// by the whole wave at once -- and the tokens go to a list.  Level 1 codes them with the fixed tables of RFC 1951 3.2.6, level 2
// with tables built for the block (3.2.7): symbol counts gathered while parsing, code lengths by the in-place minimum-redundancy
// algorithm of Moffat and Katajainen on the sorted counts, limited to 15 (7) bits by moving codes down the Kraft sum, canonical
// codes, the code lengths themselves run-length coded as the format prescribes.  Second pass: 64 tokens per step to bits, bit
// offsets by a wave scan, ORed into the wave's stream; header, the waves' streams and the end-of-block code are then joined
// bit-exactly.  A block that does not shrink is stored.
#ifndef MKT_DZ_WAVES
#define MKT_DZ_WAVES 8
#endif
constexpr int DZ_WAVES = MKT_DZ_WAVES;                  // waves per BGZF block (4, 8 or 16); 64 KiB of hash tables in all
constexpr int DZ_THREADS = 64 * DZ_WAVES;
constexpr uint32_t DZ_Q = BGZF_RAW / DZ_WAVES;           // bytes per wave (BGZF_RAW = 2^8 * 255 divides evenly)
constexpr uint32_t DZ_HBITS = DZ_WAVES == 4 ? 12 : (DZ_WAVES == 8 ? 11 : 10);
static_assert(DZ_Q * DZ_WAVES == BGZF_RAW, "even split");
constexpr uint32_t DZ_MAXLEN = 258, DZ_MINLEN = 4;
constexpr uint32_t DZ_QWORDS = (DZ_Q * 15 / 8 + 64) / 4 + 2;      // a wave's bit stream: at most 15 bits per byte
constexpr uint32_t DZ_WAVE_SCRATCH = DZ_Q + DZ_QWORDS;            // words per wave: token list + bit stream
constexpr int DZ_STAGE = 104;                            // one step's bits of a wave: 64 tokens of <= 48 bits + the carry
constexpr int DZ_HDRW = 176;                             // dynamic block header: <= 3 + 14 + 57 + 316 * 14 bits

// len_code, dist_code, mk_lengths, huff_codes, bitrev: mkt_deflate_codes.h (shared with the host test driver)
struct BitSink {                                         // one lane appends bits to words in LDS
    uint32_t* w; uint32_t n;
    __device__ inline void put(uint32_t v, uint32_t nb) {
        if (!nb) return;
        const uint32_t i = n >> 5, s = n & 31u;
        w[i] |= v << s;
        if (s + nb > 32u) w[i + 1] |= v >> (32u - s);
        n += nb;
    }
};

// Two framings of the same parse and coder.  ZS = false: a self-contained BGZF member per block of BGZF_RAW bytes (BFINAL = 1, gzip
// header, CRC-32 and size behind it).  ZS = true: a PIECE of a zlib stream (mkt_deflate.h): block `blk` is the piece zp.off[blk],
// zp.len[blk] of raw; its deflate block has BFINAL = 0 and is followed by an empty stored block (000, padding, 00 00 FF FF), so that the
// piece ends on a byte and pieces can be joined by copying; no header, the piece's Adler-32 goes to zp.adler[blk].
template <bool DYN, bool ZS>
__global__ __launch_bounds__(DZ_THREADS) void k_bgzf_deflate(const uint8_t* raw, uint64_t nraw, uint64_t first_block, const CrcTabs* ct, uint8_t* comp, uint64_t* csize,
                                                             uint32_t* scratch /* per block of the launch: DZ_WAVES * DZ_WAVE_SCRATCH words */, ZsPieces zp) {
    __shared__ __attribute__((aligned(16))) uint32_t in32[(BGZF_RAW + 288) / 4];      // + what a length measurement reads past the end
    __shared__ uint32_t htab[DZ_WAVES][1u << DZ_HBITS];
    __shared__ uint32_t stage_[DZ_WAVES][DZ_STAGE];
    __shared__ uint32_t tabl[256], x2n[32], sh[DZ_THREADS / 64];
    __shared__ uint32_t wbits[DZ_WAVES + 2], woff[DZ_WAVES + 3], wntok[DZ_WAVES];
    __shared__ uint32_t ll_tab[288], d_tab[32];          // symbol -> reversed code | length << 16
    __shared__ uint32_t ll_hist[288], d_hist[32];
    __shared__ uint32_t skey[288], dkey[32];
    __shared__ uint16_t ssym[288], dsym[32];
    __shared__ uint32_t hdrw[DZ_HDRW];
    __shared__ uint32_t nused[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint8_t* in = reinterpret_cast<uint8_t*>(in32);
    auto word_at = [&](uint32_t off) {                   // the four bytes at any offset (two aligned reads)
        const uint32_t i = off >> 2;
        return __builtin_amdgcn_alignbyte(in32[i + 1], in32[i], off & 3u);
    };
    volatile uint32_t (*stage)[DZ_STAGE] = stage_;       // lanes of a wave hand bits to each other through it
    if (!ZS && tid < 256) tabl[tid] = ct->t[tid];
    if (tid < 32) { if (!ZS) x2n[tid] = ct->x2n[tid]; d_hist[tid] = 0; }
    if (tid < 288) ll_hist[tid] = 0;
    for (int i = tid; i < DZ_HDRW; i += DZ_THREADS) hdrw[i] = 0;
    const uint64_t blk = first_block + blockIdx.x;
    const uint64_t b0 = ZS ? zp.off[blk] : blk * BGZF_RAW;
    const uint32_t n = ZS ? zp.len[blk] : (uint32_t)(nraw - b0 < BGZF_RAW ? nraw - b0 : BGZF_RAW);
    {   // the block into LDS, 16 bytes per load (blocks start on multiples of 16; the raw buffer is readable 64 bytes past its end,
        // and what lies behind byte n is never looked at)
        const uint4* src = reinterpret_cast<const uint4*>(raw + b0);
        uint4* dst = reinterpret_cast<uint4*>(in32);
        for (uint32_t i = tid; i < (BGZF_RAW + 288) / 16; i += DZ_THREADS) dst[i] = (i << 4) < n ? src[i] : make_uint4(0, 0, 0, 0);
    }
    for (uint32_t i = lane; i < (1u << DZ_HBITS); i += 64) htab[wv][i] = 0;          // 0 = empty (positions are stored + 1)
    __syncthreads();
    const uint32_t crc = ZS ? block_adler<DZ_THREADS>(in, n, sh) : block_crc<DZ_THREADS>(in, n, tabl, x2n, sh);       // (ZS: the piece's Adler-32)
    // ---- pass 1: this wave's share -> tokens (a literal byte, or 1 << 31 | length - 3 << 16 | distance - 1)
    const uint32_t q0 = wv * DZ_Q < n ? wv * DZ_Q : n, q1 = q0 + DZ_Q < n ? q0 + DZ_Q : n;
    uint32_t* wtok = scratch + ((uint64_t)blockIdx.x * DZ_WAVES + wv) * DZ_WAVE_SCRATCH;
    uint32_t* ws = wtok + DZ_Q;
    uint32_t ntok = 0;
    uint32_t cur = q0;                                   // first position not yet covered by a token
    for (uint32_t base = q0; base < q1; base += 64) {
        const uint32_t p = base + lane;
        const bool live = p < q1;
        uint32_t mlen = 0, mdist = 0;
        uint32_t h = 0;
        const bool hashable = live && p + DZ_MINLEN <= q1;
        const bool open_step = cur < base + 64u && cur < q1;      // (uniform) false: an earlier token covers all 64 positions
        // every position's candidate, checked on its first four bytes only: distance 1 (runs) before the table's
        uint32_t cand = 0xFFFFFFFFu;
        if (hashable) {
            const uint32_t v = word_at(p);
            h = (v * 2654435761u) >> (32 - DZ_HBITS);
            const uint32_t c1 = htab[wv][h];
            if (open_step) {
                if (p > q0 && word_at(p - 1u) == v) cand = p - 1u;
                else if (c1 && word_at(c1 - 1u) == v) cand = c1 - 1u;          // < base: only earlier steps have written
            }
        }
        // (all lanes have read the table before any lane of this wave writes: one wave, program order)
        if (hashable) atomicMax(&htab[wv][h], p + 1);
        if (!open_step) continue;
        // greedy parse of the step, token by token; literals are skipped in bulk, a match's length is measured by the whole
        // wave at once (lane i compares bytes 4 i .. 4 i + 3), so the cost does not grow with the length
        uint64_t sel = 0;
        {
            const uint64_t hasm = __ballot(cand != 0xFFFFFFFFu);
            const uint32_t nlive = q1 - base < 64u ? q1 - base : 64u;
            uint32_t pos = cur - base;
            while (pos < nlive) {
                const uint64_t rem = hasm >> pos;
                const uint32_t lit = rem ? (uint32_t)__builtin_ctzll(rem) : 64u;       // literals up to the next candidate
                if (lit) {
                    const uint32_t e = pos + lit < nlive ? pos + lit : nlive;
                    sel |= (e >= 64u ? ~0ull : ((1ull << e) - 1ull)) & ~((1ull << pos) - 1ull);
                    pos = e;
                    continue;
                }
                const uint32_t c = (uint32_t)__shfl((int)cand, (int)pos, 64), pp = base + pos;
                const uint32_t lim = q1 - pp < DZ_MAXLEN ? q1 - pp : DZ_MAXLEN;
                const uint32_t x = word_at(c + 4u * (uint32_t)lane) ^ word_at(pp + 4u * (uint32_t)lane);
                const uint64_t ne = __ballot(x != 0u);
                uint32_t len;
                if (ne) {
                    const int j = (int)__builtin_ctzll(ne);
                    const uint32_t xj = (uint32_t)__shfl((int)x, j, 64);
                    len = 4u * (uint32_t)j + ((uint32_t)__builtin_ctz(xj) >> 3);
                } else {                                         // 256 equal bytes: two more decide between 256, 257, 258
                    const uint32_t y = word_at(c + 256u) ^ word_at(pp + 256u);
                    len = 256u + ((y & 0xFFu) ? 0u : ((y & 0xFF00u) ? 1u : 2u));
                }
                if (len > lim) len = lim;
                if ((uint32_t)lane == pos) { mlen = len; mdist = pp - c; }
                sel |= 1ull << pos;
                pos += len;
            }
            cur = base + pos;
        }
        if ((sel >> lane) & 1ull) {
            const uint32_t rank = (uint32_t)__popcll(sel & ((1ull << lane) - 1ull));
            wtok[ntok + rank] = mlen ? (0x80000000u | ((mlen - 3u) << 16) | (mdist - 1u)) : (uint32_t)in[p];
            if (DYN) {
                if (mlen) {
                    uint32_t sy, eb, ev;
                    len_code(mlen, sy, eb, ev);
                    atomicAdd(&ll_hist[sy], 1u);
                    dist_code(mdist, sy, eb, ev);
                    atomicAdd(&d_hist[sy], 1u);
                } else atomicAdd(&ll_hist[in[p]], 1u);
            }
        }
        ntok += (uint32_t)__popcll(sel);
    }
    if (lane == 0) wntok[wv] = ntok;
    __syncthreads();
    // ---- the code tables and the block header
    uint32_t hdr_bits = 3;
    if (!DYN) {
        for (int s = tid; s < 288; s += DZ_THREADS) {        // RFC 1951 3.2.6
            uint32_t code, nb;
            if (s < 144) { code = bitrev(0x30 + s, 8); nb = 8; }
            else if (s < 256) { code = bitrev(0x190 + (s - 144), 9); nb = 9; }
            else if (s < 280) { code = bitrev(s - 256, 7); nb = 7; }
            else { code = bitrev(0xC0 + (s - 280), 8); nb = 8; }
            ll_tab[s] = code | (nb << 16);
        }
        if (tid < 32) d_tab[tid] = bitrev((uint32_t)tid, 5) | (5u << 16);
        if (tid == 0) hdrw[0] = ZS ? 2u : 3u;                // BFINAL = 1 (ZS: 0), BTYPE = 01
        __syncthreads();
    } else {
        if (tid == 0) {
            ll_hist[256] = 1;                                // end of block
            int nz = 0;
            for (int s = 0; s < 30; ++s) nz += d_hist[s] != 0u;
            if (nz == 0) { d_hist[0] = 1; d_hist[1] = 1; }       // (as zlib: never fewer than two distance codes)
            else if (nz == 1) { if (d_hist[0]) d_hist[1] = 1; else d_hist[0] = 1; }
            int nl = 0;
            for (int s = 0; s < 286; ++s) nl += ll_hist[s] != 0u;
            if (nl < 2) { if (!ll_hist[0]) ll_hist[0] = 1; else ll_hist[1] = 1; }
        }
        __syncthreads();
        // used symbols in ascending order of their counts (rank by counting; ties by symbol)
        for (int t = tid; t < 286; t += DZ_THREADS) {
            const uint32_t f = ll_hist[t];
            if (f) {
                uint32_t r = 0;
                for (int j = 0; j < 286; ++j) { const uint32_t g = ll_hist[j]; r += (g != 0u) && (g < f || (g == f && j < t)); }
                skey[r] = f; ssym[r] = (uint16_t)t;
            }
        }
        for (int t = DZ_THREADS - 1 - tid; t < 30; t += DZ_THREADS) {           // (the last threads: they have no literal symbol to rank)
            const uint32_t f = d_hist[t];
            if (f) {
                uint32_t r = 0;
                for (int j = 0; j < 30; ++j) { const uint32_t g = d_hist[j]; r += (g != 0u) && (g < f || (g == f && j < t)); }
                dkey[r] = f; dsym[r] = (uint16_t)t;
            }
        }
        if (tid == 0) { int a = 0; for (int s = 0; s < 286; ++s) a += ll_hist[s] != 0u; nused[0] = (uint32_t)a; }
        if (tid == 64) { int a = 0; for (int s = 0; s < 30; ++s) a += d_hist[s] != 0u; nused[1] = (uint32_t)a; }
        __syncthreads();
        if (tid == 0) huff_codes(skey, ssym, (int)nused[0], 15, ll_tab, 288);
        if (tid == 64) huff_codes(dkey, dsym, (int)nused[1], 15, d_tab, 32);
        __syncthreads();
        if (tid == 0) {                                      // RFC 1951 3.2.7
            int nll = 286, nd = 30;
            while (nll > 257 && !(ll_tab[nll - 1] >> 16)) --nll;
            while (nd > 1 && !(d_tab[nd - 1] >> 16)) --nd;
            // the code lengths, run-length coded: symbols 0..15 literal lengths, 16 repeat previous 3..6, 17 zeros 3..10, 18 zeros 11..138
            uint16_t* cl = reinterpret_cast<uint16_t*>(skey);         // (the sort arrays are free again) symbol | extra value << 8
            int ncl = 0;
            uint32_t clh[19];
            for (int i = 0; i < 19; ++i) clh[i] = 0;
            const int tot = nll + nd;
            auto L = [&](int i) { return i < nll ? ll_tab[i] >> 16 : d_tab[i - nll] >> 16; };
            for (int i = 0; i < tot;) {
                const uint32_t v = L(i);
                int run = 1;
                while (i + run < tot && L(i + run) == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) { const int r = run < 138 ? run : 138; cl[ncl++] = (uint16_t)(18 | ((r - 11) << 8)); clh[18]++; run -= r; }
                    if (run >= 3) { cl[ncl++] = (uint16_t)(17 | ((run - 3) << 8)); clh[17]++; run = 0; }
                    while (run-- > 0) { cl[ncl++] = 0; clh[0]++; }
                } else {
                    cl[ncl++] = (uint16_t)v; clh[v]++; --run;
                    while (run >= 3) { const int r = run < 6 ? run : 6; cl[ncl++] = (uint16_t)(16 | ((r - 3) << 8)); clh[16]++; run -= r; }
                    while (run-- > 0) { cl[ncl++] = (uint16_t)v; clh[v]++; }
                }
            }
            // the code for those 19 symbols (<= 7 bits; never fewer than two of them)
            { int nzc = 0, only = 0; for (int s2 = 0; s2 < 19; ++s2) if (clh[s2]) { ++nzc; only = s2; } if (nzc == 1) clh[only ? 0 : 1] = 1; }
            uint32_t ck[19], ctab[19];
            uint16_t cs[19];
            int nc = 0;
            for (int s = 0; s < 19; ++s) if (clh[s]) { int k = nc++; while (k > 0 && (ck[k - 1] > clh[s])) { ck[k] = ck[k - 1]; cs[k] = cs[k - 1]; --k; } ck[k] = clh[s]; cs[k] = (uint16_t)s; }
            huff_codes(ck, cs, nc, 7, ctab, 19);
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            int nclc = 19;
            while (nclc > 4 && !(ctab[order[nclc - 1]] >> 16)) --nclc;
            BitSink B{hdrw, 0};
            B.put(ZS ? 4u : 5u, 3);                          // BFINAL = 1 (ZS: 0), BTYPE = 10
            B.put((uint32_t)(nll - 257), 5); B.put((uint32_t)(nd - 1), 5); B.put((uint32_t)(nclc - 4), 4);
            for (int i = 0; i < nclc; ++i) B.put(ctab[order[i]] >> 16, 3);
            for (int i = 0; i < ncl; ++i) {
                const uint32_t sy = cl[i] & 0xFFu, ev = cl[i] >> 8;
                B.put(ctab[sy] & 0xFFFFu, ctab[sy] >> 16);
                if (sy == 16) B.put(ev, 2); else if (sy == 17) B.put(ev, 3); else if (sy == 18) B.put(ev, 7);
            }
            nused[0] = B.n;
        }
        __syncthreads();
        hdr_bits = nused[0];
    }
    // ---- pass 2: tokens -> bits
    ntok = wntok[wv];
    uint32_t wpos = 0;                                   // whole words already flushed to ws
    uint32_t carry_bits = 0;                             // bits waiting in stage[wv][0]
    if (lane == 0) stage[wv][0] = 0;
    for (uint32_t t0 = 0; t0 < ntok; t0 += 64) {
        uint32_t a = 0, na = 0, b = 0, nbb = 0;          // literal / length part, distance part
        if (t0 + lane < ntok) {
            const uint32_t tok = wtok[t0 + lane];
            if (tok >> 31) {
                uint32_t sy, eb, ev;
                len_code(((tok >> 16) & 0xFFu) + 3u, sy, eb, ev);
                const uint32_t e = ll_tab[sy];
                a = (e & 0xFFFFu) | (ev << (e >> 16)); na = (e >> 16) + eb;
                dist_code((tok & 0xFFFFu) + 1u, sy, eb, ev);
                const uint32_t d = d_tab[sy];
                b = (d & 0xFFFFu) | (ev << (d >> 16)); nbb = (d >> 16) + eb;
            } else { const uint32_t e = ll_tab[tok]; a = e & 0xFFFFu; na = e >> 16; }
        }
        const uint32_t nb = na + nbb;
        uint32_t inc = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= d) inc += y; }
        const uint32_t tot = (uint32_t)__shfl((int)inc, 63, 64);
        const uint32_t bo = carry_bits + inc - nb;
        // stage[1..] cleared for this step (word 0 holds the carry)
        for (uint32_t i = 1 + lane; i < (uint32_t)DZ_STAGE; i += 64) stage[wv][i] = 0;
        __builtin_amdgcn_wave_barrier();
        if (na) {
            const uint32_t w = bo >> 5, s = bo & 31u;
            const uint64_t lo = (uint64_t)a << s;
            atomicOr(&stage_[wv][w], (uint32_t)lo);
            if ((uint32_t)(lo >> 32)) atomicOr(&stage_[wv][w + 1], (uint32_t)(lo >> 32));
        }
        if (nbb) {
            const uint32_t w = (bo + na) >> 5, s = (bo + na) & 31u;
            const uint64_t lo = (uint64_t)b << s;
            atomicOr(&stage_[wv][w], (uint32_t)lo);
            if ((uint32_t)(lo >> 32)) atomicOr(&stage_[wv][w + 1], (uint32_t)(lo >> 32));
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t endb = carry_bits + tot, full = endb >> 5;
        for (uint32_t i = lane; i < full; i += 64) ws[wpos + i] = stage[wv][i];
        const uint32_t rest = stage[wv][full];
        __builtin_amdgcn_wave_barrier();
        wpos += full;
        carry_bits = endb & 31u;
        if (lane == 0) stage[wv][0] = carry_bits ? rest : 0u;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) { ws[wpos] = stage[wv][0]; wbits[1 + wv] = wpos * 32u + carry_bits; }
    if (tid == 0) { wbits[0] = hdr_bits; wbits[DZ_WAVES + 1] = (ll_tab[256] >> 16) + (ZS ? 3u : 0u); }       // (ZS: + the 000 of the empty stored block)
    __threadfence_block();
    __syncthreads();
    // ---- join: header, the waves' streams in order, the end-of-block code
    if (tid == 0) { uint32_t a = 0; for (int w = 0; w < DZ_WAVES + 2; ++w) { woff[w] = a; a += wbits[w]; } woff[DZ_WAVES + 2] = a; }
    __syncthreads();
    const uint32_t total_bits = woff[DZ_WAVES + 2];
    const uint32_t cbytes = (total_bits + 7u) >> 3;
    uint8_t* o = comp + blk * BGZF_STRIDE;
    constexpr uint32_t HDR = ZS ? 0u : 18u;              // bytes in front of the deflate data
    if (ZS && cbytes + 4u >= n + 5u) {                    // did not shrink: one stored block, BFINAL = 0
        if (tid == 0) {
            o[0] = 0; o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8);
            csize[blk] = n + 5u; zp.adler[blk] = crc;
        }
        for (uint32_t i = tid; i < n; i += DZ_THREADS) o[5 + i] = in[i];
        return;
    }
    if (!ZS && cbytes >= n + 5u) {                        // did not shrink: stored
        const uint32_t total = 18 + 5 + n + 8;
        if (tid == 0) {
            bgzf_header(o, total - 1);
            o[18] = 1; o[19] = (uint8_t)n; o[20] = (uint8_t)(n >> 8); o[21] = (uint8_t)~n; o[22] = (uint8_t)(~n >> 8);
            uint8_t* e = o + 23 + n;
            put32(e, crc); put32(e, n);
            csize[blk] = total;
        }
        for (uint32_t i = tid; i < n; i += DZ_THREADS) o[23 + i] = in[i];
        return;
    }
    const uint32_t eobw = ll_tab[256] & 0xFFFFu;
    const uint32_t* s0 = scratch + ((uint64_t)blockIdx.x * DZ_WAVES) * DZ_WAVE_SCRATCH + DZ_Q;
    // output word k holds bits [32 k, 32 k + 32) of the joined stream
    const uint32_t nwords = (total_bits + 31u) >> 5;
    for (uint32_t k = tid; k < nwords; k += DZ_THREADS) {
        uint32_t word = 0;
        const uint32_t lo = k << 5, hi = lo + 32u;
        for (int s = 0; s < DZ_WAVES + 2; ++s) {
            const uint32_t so = woff[s], sn = wbits[s];
            if (sn == 0u || so >= hi || so + sn <= lo) continue;
            auto sword = [&](uint32_t w) -> uint32_t {
                if (s == 0) return hdrw[w];
                if (s == DZ_WAVES + 1) return w ? 0u : eobw;
                return s0[(uint64_t)(s - 1) * DZ_WAVE_SCRATCH + w];
            };
            // bits of stream s that land in this word: stream bit j -> joined bit so + j
            const int64_t j0 = (int64_t)lo - (int64_t)so;            // stream bit at the word's bit 0 (may be negative)
            uint32_t v;
            if (j0 >= 0) {
                const uint32_t w = (uint32_t)j0 >> 5, sft = (uint32_t)j0 & 31u;
                const uint64_t two = (uint64_t)sword(w) | ((uint64_t)(((w + 1u) << 5) < sn ? sword(w + 1) : 0u) << 32);
                v = (uint32_t)(two >> sft);
                const uint32_t avail = sn - (uint32_t)j0;             // stream bits from j0 on
                if (avail < 32u) v &= (1u << avail) - 1u;
            } else {
                const uint32_t sft = (uint32_t)(-j0);                 // 1..31
                v = sword(0) << sft;
                if (sn + sft < 32u) v &= (1u << (sn + sft)) - 1u;
            }
            word |= v;
        }
        uint8_t* d = o + HDR + 4u * k;
        const uint32_t left = cbytes - 4u * k;
        d[0] = (uint8_t)word;
        if (left > 1) d[1] = (uint8_t)(word >> 8);
        if (left > 2) d[2] = (uint8_t)(word >> 16);
        if (left > 3) d[3] = (uint8_t)(word >> 24);
    }
    if (ZS) {
        if (tid == 0) {
            uint8_t* e = o + cbytes;
            e[0] = 0; e[1] = 0; e[2] = 0xFF; e[3] = 0xFF;       // LEN = 0, NLEN of the empty stored block
            csize[blk] = cbytes + 4u; zp.adler[blk] = crc;
        }
        return;
    }
    if (tid == 0) {
        const uint32_t total = 18 + cbytes + 8;
        bgzf_header(o, total - 1);
        uint8_t* e = o + 18 + cbytes;
        put32(e, crc); put32(e, n);
        csize[blk] = total;
    }
}

// level 0: one stored deflate block (BFINAL = 0) per piece
__global__ __launch_bounds__(BWG) void k_zs_stored(const uint8_t* raw, ZsPieces zp, uint8_t* comp, uint64_t* csize) {
    __shared__ uint32_t sh[BWG / 64];
    const uint64_t p = blockIdx.x;
    const uint8_t* src = raw + zp.off[p];
    const uint32_t n = zp.len[p];
    uint8_t* o = comp + p * kZsStride;
    const uint32_t ad = block_adler<BWG>(src, n, sh);
    if (threadIdx.x == 0) {
        o[0] = 0; o[1] = (uint8_t)n; o[2] = (uint8_t)(n >> 8); o[3] = (uint8_t)~n; o[4] = (uint8_t)(~n >> 8);
        csize[p] = n + 5u; zp.adler[p] = ad;
    }
    for (uint32_t i = threadIdx.x; i < n; i += BWG) o[5 + i] = src[i];
}

void crc_tables(CrcTabs* ct) {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        ct->t[i] = c;
    }
    auto mul = [](uint32_t a, uint32_t b) {
        uint32_t m = 1u << 31, p = 0;
        for (;;) {
            if (a & m) { p ^= b; if ((a & (m - 1u)) == 0u) break; }
            m >>= 1;
            b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
        }
        return p;
    };
    uint32_t p = 1u << 30;                              // x^1
    ct->x2n[0] = p;
    for (int k = 1; k < 32; ++k) { p = mul(p, p); ct->x2n[k] = p; }
}
const unsigned char kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
static constexpr uint64_t kDzPerBlock = (uint64_t)DZ_WAVES * DZ_WAVE_SCRATCH * sizeof(uint32_t);     // deflate scratch per block of a launch
// nblocks BGZF blocks of raw[0, nraw) -> comp (BGZF_STRIDE apart), their sizes -> csize; `batch` blocks per deflate launch
hipError_t bgzf_launch(const uint8_t* raw, uint64_t nraw, uint64_t nblocks, int level, const CrcTabs* ct, uint8_t* comp, uint64_t* csize, uint32_t* scratch,
                       uint64_t batch, hipStream_t st) {
    if (level > 0) {
        for (uint64_t fb = 0; fb < nblocks; fb += batch) {
            const unsigned g = (unsigned)(nblocks - fb < batch ? nblocks - fb : batch);
            if (level >= 2) hipLaunchKernelGGL((k_bgzf_deflate<true, false>), dim3(g), dim3(DZ_THREADS), 0, st, raw, nraw, fb, ct, comp, csize, scratch, ZsPieces{});
            else hipLaunchKernelGGL((k_bgzf_deflate<false, false>), dim3(g), dim3(DZ_THREADS), 0, st, raw, nraw, fb, ct, comp, csize, scratch, ZsPieces{});
        }
    } else {
        hipLaunchKernelGGL(k_bgzf_stored, dim3((unsigned)nblocks), dim3(BWG), 0, st, raw, nraw, ct, comp, csize);
    }
    return hipGetLastError();
}
hipError_t bgzf_pack(const uint8_t* comp, const uint64_t* coff, uint64_t nblocks, uint8_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)nblocks), dim3(BWG), 0, st, comp, coff, nblocks, out);
    return hipGetLastError();
}
size_t deflate_scratch_bytes(uint64_t batch) { return (size_t)(batch * kDzPerBlock); }
hipError_t zs_deflate(const uint8_t* raw, ZsPieces zp, uint64_t npieces, int level, uint8_t* comp, uint64_t* csize, uint32_t* scratch, uint64_t batch, hipStream_t st) {
    if (npieces == 0) return hipSuccess;
    if (level <= 0) hipLaunchKernelGGL(k_zs_stored, dim3((unsigned)npieces), dim3(BWG), 0, st, raw, zp, comp, csize);
    else {
        if (!scratch || batch == 0) return hipErrorInvalidValue;
        for (uint64_t fb = 0; fb < npieces; fb += batch) {
            const unsigned g = (unsigned)(npieces - fb < batch ? npieces - fb : batch);
            if (level >= 2) hipLaunchKernelGGL((k_bgzf_deflate<true, true>), dim3(g), dim3(DZ_THREADS), 0, st, raw, (uint64_t)0, fb, (const CrcTabs*)nullptr, comp, csize, scratch, zp);
            else hipLaunchKernelGGL((k_bgzf_deflate<false, true>), dim3(g), dim3(DZ_THREADS), 0, st, raw, (uint64_t)0, fb, (const CrcTabs*)nullptr, comp, csize, scratch, zp);
        }
    }
    return hipGetLastError();
}

}  // namespace mkt
