// mkt_inflate.h -- reading BGZF (SAMv1 4.1) back: the block table of a file and the inflate of RFC 1951 (include/mkt.h has the
// definition, DESIGN.md 6g the kernel).
//
// Everything that decides whether a stream is accepted lives here as __host__ __device__ inline functions: the bit reader, the Kraft
// checks and the table build, the dynamic header (HLIT / HDIST / HCLEN, the code-length code, the repeats 16 / 17 / 18) and the decode of
// one token with all its refusals.  The kernel (mkt_inflate.hip) runs them with one wavefront per BGZF block and only adds the parallel
// expansion of a batch of tokens; inf_member_serial below runs them one token at a time on the host (tests/host/inflate_host.cpp).
// Compiled without hipcc this file includes no HIP header, like mkt_px2.h.
//
// Nothing here trusts the stream: every read is checked against the end of the member's compressed span, every write against ISIZE,
// a distance against the bytes the block has produced so far, and every loop consumes at least one bit of the span per turn.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define MKT_INF_HD __host__ __device__
#else
#define MKT_INF_HD
#endif

namespace mkt {

// why a file or a block is refused (0: it is not).  The status word of a block is one of these.
enum InfReason : uint32_t {
    INF_OK = 0,
    // the block table (host)
    INF_BAD_MAGIC, INF_PLAIN_GZIP, INF_XLEN, INF_PAST_FILE, INF_BSIZE_SMALL, INF_ISIZE_LARGE,
    // the stream
    INF_BLOCK_TYPE, INF_STORED_NLEN, INF_STORED_PAD, INF_HLIT, INF_HDIST, INF_CL_OVER, INF_CL_INCOMPLETE, INF_REPEAT_FIRST, INF_REPEAT_PAST,
    INF_NO_EOB, INF_LL_OVER, INF_LL_INCOMPLETE, INF_D_OVER, INF_D_INCOMPLETE, INF_BAD_CODE, INF_LEN_SYMBOL, INF_NO_DIST_CODE, INF_DIST_SYMBOL,
    INF_DIST_BEFORE, INF_OUT_LONG, INF_OUT_SHORT, INF_PAST_SPAN, INF_TRAILING,
    // the footer
    INF_CRC,
    INF_REASONS
};
// a short key (what the tests compare) and a sentence (what a message says)
inline const char* inf_reason_key(uint32_t r) {
    static const char* const k[INF_REASONS] = {"ok", "bad_magic", "plain_gzip", "xlen", "past_file", "bsize_small", "isize_large", "block_type_3", "stored_nlen", "stored_padding",
        "hlit", "hdist", "cl_oversubscribed", "cl_incomplete", "repeat_first", "repeat_past_last", "no_end_of_block", "ll_oversubscribed", "ll_incomplete", "d_oversubscribed",
        "d_incomplete", "bad_code", "length_symbol", "no_distance_code", "distance_symbol", "distance_before_start", "output_long", "output_short", "past_span", "trailing_bytes", "crc"};
    return r < INF_REASONS ? k[r] : "unknown";
}
inline const char* inf_reason_text(uint32_t r) {
    static const char* const t[INF_REASONS] = {"ok", "no BGZF block (bad magic bytes)", "not BGZF: a plain gzip file (a member without the extra field)",
        "not BGZF: the extra field is not the one BC subfield (XLEN 6)", "the block runs past the end of the file (truncated?)", "BSIZE is too small for a block",
        "ISIZE exceeds 65536", "deflate block type 3", "stored block: NLEN is not the complement of LEN", "stored block: the bits up to the byte boundary are not zero",
        "dynamic block: more than 286 literal/length codes", "dynamic block: more than 30 distance codes", "code-length code: over-subscribed", "code-length code: incomplete",
        "dynamic block: repeat of a previous length at the first length", "dynamic block: a repeat runs past the last code length", "dynamic block: no code for end of block",
        "literal/length code: over-subscribed", "literal/length code: incomplete", "distance code: over-subscribed", "distance code: incomplete",
        "a bit pattern that is no code", "length symbol 286 or 287", "a match in a block without distance codes", "distance symbol 30 or 31",
        "a distance reaches before the start of the block", "the output is longer than ISIZE", "the output is shorter than ISIZE", "the stream runs past its span",
        "trailing bytes after the final deflate block", "CRC-32 of the inflated block differs from the footer"};
    return r < INF_REASONS ? t[r] : "unknown";
}

constexpr uint32_t kInfMaxIsize = 65536;                 // ISIZE 0 .. 65536 inclusive
constexpr uint32_t kInfHead = 18, kInfFoot = 8;          // a member: 18 bytes of header, the deflate span, CRC-32 and ISIZE
constexpr uint32_t kInfSpanPad = 8;                      // the bit reader looks at most 4 bytes past the span; they are zeros
constexpr uint32_t kInfBatch = 64;                       // tokens per batch of the kernel: one per lane

// ---- the block table (host) ---------------------------------------------------------------------------------------------------------
struct InfBlock { uint64_t coff, toff; uint32_t bsize, isize, crc, pad; };     // file offset, text offset (exclusive sum of ISIZE), BSIZE + 1
static_assert(sizeof(InfBlock) == 32, "InfBlock is shared with the device as it is");

// Walks the members of gz[0, n).  Accepts what tests/px2def.py bgzf_blocks accepts (1f 8b 08 04, XLEN 6, the one BC subfield, BSIZE)
// and nothing else; 0, or the reason with *bad_off = the file offset of the member.  has_eof: the file ends with the empty block.
inline uint32_t inf_block_table(const uint8_t* gz, uint64_t n, std::vector<InfBlock>& out, uint64_t* bad_off, bool* has_eof) {
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    out.clear();
    uint64_t p = 0, u = 0;
    auto fail = [&](uint32_t r) { *bad_off = p; return r; };
    while (p < n) {
        const uint8_t* h = gz + p;
        const uint64_t left = n - p;
        if (left < 4 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return fail(left < 4 && left >= 1 && h[0] == 0x1f ? INF_PAST_FILE : INF_BAD_MAGIC);
        if (!(h[3] & 4)) return fail(INF_PLAIN_GZIP);
        if (h[3] != 4) return fail(INF_BAD_MAGIC);
        if (left < kInfHead) return fail(INF_PAST_FILE);
        if (h[10] != 6 || h[11] != 0 || h[12] != 'B' || h[13] != 'C' || h[14] != 2 || h[15] != 0) return fail(INF_XLEN);
        const uint32_t bsize = ((uint32_t)h[16] | (uint32_t)h[17] << 8) + 1u;
        if (bsize > left) return fail(INF_PAST_FILE);
        if (bsize < kInfHead + kInfFoot) return fail(INF_BSIZE_SMALL);
        const uint8_t* f = h + bsize - 8;
        InfBlock b;
        b.coff = p; b.toff = u; b.bsize = bsize; b.pad = 0;
        b.crc = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)f[3] << 24;
        b.isize = (uint32_t)f[4] | (uint32_t)f[5] << 8 | (uint32_t)f[6] << 16 | (uint32_t)f[7] << 24;
        if (b.isize > kInfMaxIsize) return fail(INF_ISIZE_LARGE);
        out.push_back(b);
        u += b.isize;
        p += bsize;
    }
    bool e = n >= 28;
    for (int k = 0; e && k < 28; ++k) e = gz[n - 28 + k] == eof[k];
    *has_eof = e;
    return INF_OK;
}

// ---- the bit reader -------------------------------------------------------------------------------------------------------------------
// d is readable up to 4 bytes past (end + 7) / 8 and holds zeros there.  p and end are bit offsets into d.
struct InfBits {
    const uint8_t* d; uint32_t p, end;
    MKT_INF_HD uint32_t peek(uint32_t nb) const {         // the next nb <= 16 bits, the first one in bit 0
        const uint32_t q = p >> 3;
        const uint32_t w = (uint32_t)d[q] | (uint32_t)d[q + 1] << 8 | (uint32_t)d[q + 2] << 16 | (uint32_t)d[q + 3] << 24;
        return (w >> (p & 7u)) & ((1u << nb) - 1u);
    }
    MKT_INF_HD bool skip(uint32_t nb) { if (p + nb > end) return false; p += nb; return true; }
    MKT_INF_HD int take(uint32_t nb) {                    // the bits, or -1 past the span
        const uint32_t v = peek(nb);
        return skip(nb) ? (int)v : -1;
    }
};

// ---- codes ------------------------------------------------------------------------------------------------------------------------------
// A canonical code (RFC 1951 3.2.2) as the counts per length and the symbols in the order of their codes.
// inf_build: < 0 over-subscribed, 0 complete, > 0 incomplete (the Kraft sum against 2^15); *used = symbols that have a code.
MKT_INF_HD inline int inf_build(const uint8_t* lens, uint32_t n, uint16_t* count /* [16] */, uint16_t* sym /* [n] */, uint32_t* used) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) count[lens[s] & 15u]++;
    *used = n - count[0];
    int left = 1;
    for (int l = 1; l < 16; ++l) { left <<= 1; left -= (int)count[l]; if (left < 0) return -1; }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (uint32_t s = 0; s < n; ++s) if (lens[s] & 15u) sym[offs[lens[s] & 15u]++] = (uint16_t)s;
    return left;
}
// one symbol: >= 0, or -INF_BAD_CODE (a pattern of 15 bits that is no code: the unused half of a single-code set), -INF_PAST_SPAN
MKT_INF_HD inline int inf_symbol(InfBits& b, const uint16_t* count, const uint16_t* sym) {
    uint32_t w = b.peek(15);
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len < 16; ++len) {
        code |= (int)(w & 1u);
        w >>= 1;
        const int cnt = count[len];
        if (code - cnt < first) return b.skip(len) ? (int)sym[index + (code - first)] : -(int)INF_PAST_SPAN;
        index += cnt; first += cnt;
        first <<= 1; code <<= 1;
    }
    return -(int)INF_BAD_CODE;
}

// the tables of one deflate block and the scratch of its header
struct InfTables {
    uint16_t lcount[16], lsym[288], dcount[16], dsym[32], ccount[16], csym[19];
    uint8_t lens[320];                                    // literal/length lengths, then the distance lengths
    uint32_t has_dist;
};

// the fixed code (3.2.6)
MKT_INF_HD inline void inf_fixed(InfTables& t) {
    for (uint32_t s = 0; s < 288; ++s) t.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    for (uint32_t s = 0; s < 32; ++s) t.lens[288 + s] = 5;
    uint32_t used;
    (void)inf_build(t.lens, 288, t.lcount, t.lsym, &used);
    (void)inf_build(t.lens + 288, 32, t.dcount, t.dsym, &used);
    t.has_dist = 1;
}
// the header of a dynamic block (3.2.7) behind its three type bits: 0, or the reason
MKT_INF_HD inline uint32_t inf_dynamic(InfBits& b, InfTables& t) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int h = b.take(14);
    if (h < 0) return INF_PAST_SPAN;
    const uint32_t hlit = ((uint32_t)h & 31u) + 257u, hdist = ((uint32_t)h >> 5 & 31u) + 1u, hclen = ((uint32_t)h >> 10) + 4u;
    if (hlit > 286) return INF_HLIT;
    if (hdist > 30) return INF_HDIST;
    uint8_t cl[19];
    for (int k = 0; k < 19; ++k) cl[k] = 0;
    for (uint32_t k = 0; k < hclen; ++k) {
        const int v = b.take(3);
        if (v < 0) return INF_PAST_SPAN;
        cl[order[k]] = (uint8_t)v;
    }
    uint32_t used;
    int left = inf_build(cl, 19, t.ccount, t.csym, &used);
    if (left < 0) return INF_CL_OVER;
    if (left > 0) return INF_CL_INCOMPLETE;               // (no symbol at all is incomplete too)
    const uint32_t total = hlit + hdist;
    uint32_t n = 0;
    while (n < total) {                                   // every turn takes at least one bit
        const int s = inf_symbol(b, t.ccount, t.csym);
        if (s < 0) return (uint32_t)-s;
        if (s < 16) { t.lens[n++] = (uint8_t)s; continue; }
        uint32_t rep, v = 0;
        int x;
        if (s == 16) {
            if (n == 0) return INF_REPEAT_FIRST;
            v = t.lens[n - 1];
            if ((x = b.take(2)) < 0) return INF_PAST_SPAN;
            rep = 3u + (uint32_t)x;
        } else if (s == 17) {
            if ((x = b.take(3)) < 0) return INF_PAST_SPAN;
            rep = 3u + (uint32_t)x;
        } else {
            if ((x = b.take(7)) < 0) return INF_PAST_SPAN;
            rep = 11u + (uint32_t)x;
        }
        if (n + rep > total) return INF_REPEAT_PAST;
        for (uint32_t k = 0; k < rep; ++k) t.lens[n++] = (uint8_t)v;
    }
    if (!t.lens[256]) return INF_NO_EOB;
    left = inf_build(t.lens, hlit, t.lcount, t.lsym, &used);
    if (left < 0) return INF_LL_OVER;
    if (left > 0) return INF_LL_INCOMPLETE;
    left = inf_build(t.lens + hlit, hdist, t.dcount, t.dsym, &used);
    if (left < 0) return INF_D_OVER;
    t.has_dist = used ? 1u : 0u;                          // literals only: no distance code at all
    if (left > 0 && used && !(used == 1 && t.dcount[1] == 1)) return INF_D_INCOMPLETE;       // one distance code of length 1 is allowed
    return INF_OK;
}

// A token: length << 16 | x.  Length 1: the literal byte x.  Length 3 .. 258: a match at distance x + 1 (1 .. 32768).
// 0 a token, 1 end of block, < 0 minus the reason.  outpos: bytes of the BGZF block produced so far (a distance may not reach before
// them, and outpos + length may not exceed isize).
MKT_INF_HD inline int inf_token(InfBits& b, const InfTables& t, uint32_t outpos, uint32_t isize, uint32_t* tok) {
    const int s = inf_symbol(b, t.lcount, t.lsym);
    if (s < 0) return s;
    if (s < 256) {
        if (outpos + 1u > isize) return -(int)INF_OUT_LONG;
        *tok = 1u << 16 | (uint32_t)s;
        return 0;
    }
    if (s == 256) return 1;
    if (s > 285) return -(int)INF_LEN_SYMBOL;
    const uint32_t i = (uint32_t)s - 257u;
    uint32_t len;
    if (i < 8) len = 3u + i;
    else if (i == 28) len = 258;
    else {
        const uint32_t e = (i - 4u) >> 2;
        const int x = b.take(e);
        if (x < 0) return -(int)INF_PAST_SPAN;
        len = 3u + ((4u + (i & 3u)) << e) + (uint32_t)x;
    }
    if (!t.has_dist) return -(int)INF_NO_DIST_CODE;
    const int ds = inf_symbol(b, t.dcount, t.dsym);
    if (ds < 0) return ds;
    if (ds > 29) return -(int)INF_DIST_SYMBOL;
    uint32_t dist;
    if (ds < 4) dist = (uint32_t)ds + 1u;
    else {
        const uint32_t e = ((uint32_t)ds >> 1) - 1u;
        const int x = b.take(e);
        if (x < 0) return -(int)INF_PAST_SPAN;
        dist = 1u + ((2u + ((uint32_t)ds & 1u)) << e) + (uint32_t)x;
    }
    if (dist > outpos) return -(int)INF_DIST_BEFORE;
    if (outpos + len > isize) return -(int)INF_OUT_LONG;
    *tok = len << 16 | (dist - 1u);
    return 0;
}

// the start of a deflate block: BFINAL and BTYPE; a stored block's LEN after its checks (the reader then stands on its first byte)
MKT_INF_HD inline uint32_t inf_block_head(InfBits& b, uint32_t* bfinal, uint32_t* btype) {
    const int h = b.take(3);
    if (h < 0) return INF_PAST_SPAN;
    *bfinal = (uint32_t)h & 1u;
    *btype = (uint32_t)h >> 1;
    return *btype == 3 ? INF_BLOCK_TYPE : INF_OK;
}
MKT_INF_HD inline uint32_t inf_stored_head(InfBits& b, uint32_t outpos, uint32_t isize, uint32_t* len) {
    const uint32_t pad = (8u - (b.p & 7u)) & 7u;
    const int z = b.take(pad);
    if (z < 0) return INF_PAST_SPAN;
    if (z) return INF_STORED_PAD;
    const int n = b.take(16), nn = b.take(16);
    if (n < 0 || nn < 0) return INF_PAST_SPAN;
    if (((uint32_t)n ^ (uint32_t)nn) != 0xFFFFu) return INF_STORED_NLEN;
    if (b.p + 8u * (uint32_t)n > b.end) return INF_PAST_SPAN;
    if (outpos + (uint32_t)n > isize) return INF_OUT_LONG;
    *len = (uint32_t)n;
    return INF_OK;
}
// behind the final block: zero bits up to the byte boundary, the end of the span, all of ISIZE produced
MKT_INF_HD inline uint32_t inf_member_end(InfBits& b, uint32_t outpos, uint32_t isize) {
    const uint32_t pad = (8u - (b.p & 7u)) & 7u;
    const int z = b.take(pad);
    if (z < 0) return INF_PAST_SPAN;
    if (z || b.p != b.end) return INF_TRAILING;
    return outpos == isize ? INF_OK : INF_OUT_SHORT;
}

// ---- one member, serially (the host driver; the kernel has the same loop with a batch of tokens expanded by 64 lanes) ------------------
// span: the deflate bytes, readable kInfSpanPad zero bytes past nspan.  out: isize bytes.  kinds[3]: deflate blocks by type, added to.
inline uint32_t inf_member_serial(const uint8_t* span, uint32_t nspan, uint8_t* out, uint32_t isize, uint64_t kinds[3]) {
    InfBits b = {span, 0, nspan * 8u};
    InfTables t;
    uint32_t outpos = 0;
    for (;;) {
        uint32_t bfinal = 0, btype = 0;
        if (uint32_t r = inf_block_head(b, &bfinal, &btype)) return r;
        kinds[btype]++;
        if (btype == 0) {
            uint32_t n = 0;
            if (uint32_t r = inf_stored_head(b, outpos, isize, &n)) return r;
            for (uint32_t k = 0; k < n; ++k) out[outpos + k] = span[(b.p >> 3) + k];
            b.p += 8u * n;
            outpos += n;
        } else {
            if (btype == 1) inf_fixed(t);
            else if (uint32_t r = inf_dynamic(b, t)) return r;
            for (;;) {
                uint32_t tok = 0;
                const int r = inf_token(b, t, outpos, isize, &tok);
                if (r < 0) return (uint32_t)-r;
                if (r == 1) break;
                const uint32_t len = tok >> 16;
                if (len == 1) out[outpos] = (uint8_t)tok;
                else for (uint32_t k = 0, d = (tok & 0xFFFFu) + 1u; k < len; ++k) out[outpos + k] = out[outpos + k - d];
                outpos += len;
            }
        }
        if (bfinal) break;
    }
    return inf_member_end(b, outpos, isize);
}

}  // namespace mkt
