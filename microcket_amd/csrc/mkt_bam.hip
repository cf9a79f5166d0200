// mkt_bam.hip -- SURVEY.md 8(f) N3: the .sam -> BAM tail of the pipeline, on the GPU.
//
// The driver ends with (microcket:533-540)
//     cat $samheader $sid.flash.sam $sid.unc.sam | samtools view -b | samtools sort -o $sid.valid.bam ;  samtools index $sid.valid.bam
// i.e. the filtered alignments that sam2pairs wrote, as a coordinate-sorted, BGZF-compressed BAM with its .bai.  Here: newline
// index, one key per line (reference id, position, strand), the stable LSD radix sort of mkt_sort.hip, an exclusive scan of the
// record sizes, one pass that writes the binary records in sorted order, BGZF blocks (level 2, the default: LZ77 + a Huffman
// code built per block; level 1: the fixed code; level 0: stored; CRC-32 per block) and the reductions the BAI needs (linear index, chunk starts, per-reference counts).  Byte / integer work
// bound by HBM; no MFMA.
//
// Formats: SAM / BAM / BGZF / BAI as published in "Sequence Alignment/Map Format Specification" (samtools/hts-specs, SAMv1
// sections 1.4, 4.1, 4.2, 5.2), RFC 1951 (deflate), RFC 1952 (gzip, CRC-32).  The reference ships samtools only as a prebuilt
// third-party binary (bin/samtools), which is never run here: parity with it is UNPINNED.  What is checked instead
// (tests/test_gpu_bam.py): every block inflates with Python's zlib (which verifies CRC-32 and ISIZE), an independent reader
// written from the specification (tests/bamio.py) gets the input lines back in coordinate order, and every region query
// through the .bai returns exactly the records a brute-force scan finds; the records themselves are byte for byte those of an
// encoder written from the specification (tests/bamdef.py; DESIGN.md "The records, exactly").  Conventions that the specification leaves open follow
// htslib's documented behaviour: integer tags in the smallest type that holds them (unsigned types for values >= 0), `bin`
// from [pos, end) with a length of 1 for unmapped reads or empty CIGARs, a mapped read without CIGAR marked unmapped, ties
// of the sort key (reference, position, strand) in input order, @HD SO:coordinate set in the header of a sorted file.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <errno.h>
#include <fcntl.h>
#include <unistd.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_deflate.h"
#include "mkt_devbuf.h"
#include "mkt_launch.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

enum { BE_FIELDS = 1, BE_REF = 2, BE_NUM = 4, BE_CIGAR = 8, BE_TAG = 16, BE_SEQ = 32, BE_NAME = 64 };

struct RefTab {                                       // reference names -> ids (built on the host from the @SQ lines)
    const unsigned long long* hash;                   // FNV-1a of the name, 0 = empty
    const int32_t* id;
    const uint32_t* name_off;                         // per id: [off, off + len) in names
    const uint8_t* names;
    uint32_t mask, nref;
};
struct BamIdx { int32_t tid, beg, end; uint32_t bin; };     // per record, in file order: what the index needs (bin: low half; high half: FLAG)

__device__ inline int32_t ref_lookup(const RefTab& rt, const uint8_t* t, uint64_t a, uint64_t b, uint32_t* err) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (uint64_t p = a; p < b; ++p) { h ^= t[p]; h *= 0x100000001b3ull; }
    if (!h) h = 1;
    uint32_t s = (uint32_t)(h >> 20) & rt.mask;
    for (uint32_t probe = 0; probe <= rt.mask; ++probe) {
        const unsigned long long cur = rt.hash[s];
        if (cur == 0ull) break;
        if (cur == h) {
            const int32_t id = rt.id[s];
            const uint32_t o = rt.name_off[id], l = rt.name_off[id + 1] - o;
            bool same = l == (uint32_t)(b - a);
            for (uint32_t i = 0; same && i < l; ++i) same = rt.names[o + i] == t[a + i];
            if (same) return id;
        }
        s = (s + 1u) & rt.mask;
    }
    atomicOr(err, (uint32_t)BE_REF);
    return -1;
}
__device__ inline uint32_t reg2bin(int64_t beg, int64_t end) {        // SAMv1 5.3
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}
__device__ inline void put8(uint8_t*& o, uint32_t v) { *o++ = (uint8_t)v; }
__device__ inline void put16(uint8_t*& o, uint32_t v) { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o += 2; }
// A record's bytes go out through this: single bytes up to the first 8-byte boundary, then whole aligned 8-byte words, single
// bytes for the rest (the neighbours on both sides belong to other threads' records).
struct Sink {
    uint8_t* p;            // where the next stored byte goes (8-aligned whenever k > 0)
    uint64_t acc;
    uint32_t k;            // bytes waiting in acc
    __device__ explicit Sink(uint8_t* at) : p(at), acc(0), k(0) {}
    __device__ inline void b(uint32_t v) {
        if (k == 0u && ((uintptr_t)p & 7u)) { *p++ = (uint8_t)v; return; }
        acc |= (uint64_t)(v & 0xFFu) << (8u * k);
        if (++k == 8u) { *reinterpret_cast<uint64_t*>(p) = acc; p += 8; acc = 0; k = 0; }
    }
    __device__ inline void h(uint32_t v) { b(v); b(v >> 8); }
    __device__ inline void w(uint32_t v) { b(v); b(v >> 8); b(v >> 16); b(v >> 24); }
    __device__ inline void flush() { for (uint32_t i = 0; i < k; ++i) p[i] = (uint8_t)(acc >> (8u * i)); p += k; k = 0; acc = 0; }
};

// unsigned decimal in [a, b); *ok cleared when it is not one
__device__ inline uint64_t dec_u(const uint8_t* t, uint64_t a, uint64_t b, bool* ok) {
    if (a >= b || b - a > 19) { *ok = false; return 0; }
    uint64_t v = 0;
    for (uint64_t p = a; p < b; ++p) { const uint32_t d = (uint32_t)t[p] - 48u; if (d > 9u) { *ok = false; return 0; } v = v * 10 + d; }
    return v;
}
__device__ inline int64_t dec_s(const uint8_t* t, uint64_t a, uint64_t b, bool* ok) {
    bool neg = false;
    if (a < b && (t[a] == '-' || t[a] == '+')) { neg = t[a] == '-'; ++a; }
    const uint64_t v = dec_u(t, a, b, ok);
    if (v > (1ull << 62)) { *ok = false; return 0; }
    return neg ? -(int64_t)v : (int64_t)v;
}
// decimal floating point text -> float (tags of type f and B:f).  Mantissa M of up to 19 digits, power of ten E applied in double.
// Where M < 2^53 and |E| <= 22 (which holds whatever samtools prints with %g up to %.15g at those exponents) both are exact
// doubles and one multiplication or division gives M * 10^E; that one result is rounded TO ODD (the fma gives the side the exact
// value lies on), so the rounding to float that follows is the correct rounding of the decimal, ties to even: a double rounded to
// nearest can land exactly on a float midpoint the decimal only comes close to (967498269e-19 does), and then goes the wrong way.
// The %.9g print of ANY finite float also comes back as that float (it lies within 5e-10 of it, the nearest midpoint 6e-8 away;
// the few double roundings cannot bridge that).  Everything else -- more digits, |E| > 22 -- can differ from strtof in the last bit.
__device__ inline float dec_f(const uint8_t* t, uint64_t a, uint64_t b, bool* ok) {
    bool neg = false;
    if (a < b && (t[a] == '-' || t[a] == '+')) { neg = t[a] == '-'; ++a; }
    uint64_t m = 0;
    int nd = 0, e10 = 0;
    bool any = false, dot = false;
    uint64_t p = a;
    for (; p < b; ++p) {
        const uint8_t c = t[p];
        if (c == '.' && !dot) { dot = true; continue; }
        const uint32_t d = (uint32_t)c - 48u;
        if (d > 9u) break;
        any = true;
        if (nd < 19) { m = m * 10 + d; if (m) ++nd; if (dot) --e10; }
        else if (!dot) ++e10;
    }
    if (!any) { *ok = false; return 0.f; }
    if (p < b) {
        if (t[p] != 'e' && t[p] != 'E') { *ok = false; return 0.f; }
        bool eok = true;
        const int64_t ee = dec_s(t, p + 1, b, &eok);
        if (!eok || ee > 400 || ee < -400) { *ok = false; return 0.f; }
        e10 += (int)ee;
    }
    double d = (double)m;
    const double p10[] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    int e = e10;
    if (m < (1ull << 53) && e >= -22 && e <= 22) {
        const double pw = p10[e >= 0 ? e : -e];
        double left;                                   // exact value minus d, in sign (exactly zero when d is exact)
        if (e >= 0) { const double x = d * pw; left = fma(d, pw, -x); d = x; }
        else { const double q = d / pw; left = fma(-q, pw, d); d = q; }
        long long bits = __double_as_longlong(d);      // d > 0 here (or m == 0 and left == 0): neighbours are bits +- 1
        if (left != 0.0 && !(bits & 1ll)) d = __longlong_as_double(bits + (left > 0.0 ? 1ll : -1ll));
    } else {
        while (e > 22) { d *= 1e22; e -= 22; }
        while (e < -22) { d /= 1e22; e += 22; }
        d = e >= 0 ? d * p10[e] : d / p10[-e];
    }
    const float f = (float)d;
    return neg ? -f : f;
}

__device__ inline uint32_t seq_code(uint8_t c) {      // SAMv1 4.2: "=ACMGRSVTWYHKDBN", anything else (and lower case alike) -> N
    switch (c & 0xDF) {                                // upper case
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14; default: break;
    }
    return c == '=' ? 0u : 15u;
}
__device__ inline int cigar_op(uint8_t c) {
    switch (c) { case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5;
                 case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1; }
}

// One alignment line -> its BAM record.  WRITE = false: sizes and keys only.  Returns the record's bytes (block_size + 4), 0 on error.
template <bool WRITE>
__device__ uint32_t bam_record(const uint8_t* t, uint64_t ls, uint64_t le, const RefTab& rt, uint8_t* out, BamIdx* ix, uint32_t* err) {
    uint64_t tab[11];
    int nt = 0;
    for (uint64_t p = ls; p < le && nt < 11; ++p) if (t[p] == '\t') tab[nt++] = p;
    if (nt < 10) { atomicOr(err, (uint32_t)BE_FIELDS); return 0; }
    const uint64_t qual_end = nt == 11 ? tab[10] : le;
    bool ok = true;
    const uint64_t l_qname = tab[0] - ls;
    if (l_qname == 0 || l_qname > 254) { atomicOr(err, (uint32_t)BE_NAME); return 0; }
    uint64_t flag = dec_u(t, tab[0] + 1, tab[1], &ok);
    const int64_t pos1 = dec_s(t, tab[2] + 1, tab[3], &ok);
    const uint64_t mapq = dec_u(t, tab[3] + 1, tab[4], &ok);
    const int64_t pnext1 = dec_s(t, tab[6] + 1, tab[7], &ok);
    const int64_t tlen = dec_s(t, tab[7] + 1, tab[8], &ok);
    if (!ok || flag > 65535 || mapq > 255 || pos1 < 0 || pos1 > 0x7fffffffll || pnext1 < 0 || pnext1 > 0x7fffffffll || tlen > 0x7fffffffll || tlen < -0x80000000ll) {
        atomicOr(err, (uint32_t)BE_NUM);
        return 0;
    }
    int32_t tid = -1, mtid = -1;
    {
        const uint64_t a = tab[1] + 1, b = tab[2];
        if (!(b - a == 1 && t[a] == '*')) tid = ref_lookup(rt, t, a, b, err);
        const uint64_t c = tab[5] + 1, d = tab[6];
        if (d - c == 1 && t[c] == '=') mtid = tid;
        else if (!(d - c == 1 && t[c] == '*')) mtid = ref_lookup(rt, t, c, d, err);
    }
    // CIGAR
    const uint64_t ca = tab[4] + 1, cb = tab[5];
    uint32_t n_cigar = 0;
    int64_t rlen = 0;
    const bool no_cigar = cb - ca == 1 && t[ca] == '*';
    if (!(flag & 4u) && (pos1 == 0 || tid < 0)) flag |= 4u;  // "mapped query cannot have zero coordinate; treated as unmapped" / no reference (htslib sam_parse1)
    if (no_cigar) { if (!(flag & 4u)) flag |= 4u; }          // "mapped query must have a CIGAR; treated as unmapped"
    else {
        uint64_t v = 0;
        bool digits = false;
        for (uint64_t p = ca; p < cb; ++p) {
            const uint32_t d = (uint32_t)t[p] - 48u;
            if (d <= 9u) { v = v * 10 + d; digits = true; if (v >= (1ull << 28)) { atomicOr(err, (uint32_t)BE_CIGAR); return 0; } continue; }
            const int op = cigar_op(t[p]);
            if (op < 0 || !digits) { atomicOr(err, (uint32_t)BE_CIGAR); return 0; }
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += (int64_t)v;
            ++n_cigar; v = 0; digits = false;
        }
        if (digits || n_cigar == 0 || n_cigar > 65535) { atomicOr(err, (uint32_t)BE_CIGAR); return 0; }
    }
    // SEQ / QUAL
    const uint64_t sa = tab[8] + 1, sb = tab[9], qa = tab[9] + 1, qb = qual_end;
    const uint32_t l_seq = (sb - sa == 1 && t[sa] == '*') ? 0u : (uint32_t)(sb - sa);
    const bool no_qual = qb - qa == 1 && t[qa] == '*';                     // (also for a 1-base read, as in htslib)
    if (!no_qual && (qb - qa) != l_seq) { atomicOr(err, (uint32_t)BE_SEQ); return 0; }
    const int32_t pos = (int32_t)pos1 - 1;
    int64_t span = ((flag & 4u) || rlen == 0) ? 1 : rlen;
    const int64_t end = (int64_t)pos + span;
    const uint32_t bin = reg2bin(pos, end);
    Sink o(WRITE ? out + 4 : out);                             // block_size (the first four bytes) is written at the end
    if (WRITE) {
        o.w((uint32_t)tid);
        o.w((uint32_t)pos);
        o.b((uint32_t)l_qname + 1u);
        o.b((uint32_t)mapq);
        o.h(bin);
        o.h(n_cigar);
        o.h((uint32_t)flag);
        o.w(l_seq);
        o.w((uint32_t)mtid);
        o.w((uint32_t)((int32_t)pnext1 - 1));
        o.w((uint32_t)(int32_t)tlen);
        for (uint64_t p = ls; p < tab[0]; ++p) o.b(t[p]);
        o.b(0);
        if (!no_cigar) {
            uint32_t v = 0;
            for (uint64_t p = ca; p < cb; ++p) {
                const uint32_t d = (uint32_t)t[p] - 48u;
                if (d <= 9u) { v = v * 10 + d; continue; }
                o.w((v << 4) | (uint32_t)cigar_op(t[p]));
                v = 0;
            }
        }
        for (uint32_t k = 0; k + 1 < l_seq; k += 2) o.b((seq_code(t[sa + k]) << 4) | seq_code(t[sa + k + 1]));
        if (l_seq & 1u) o.b(seq_code(t[sa + l_seq - 1]) << 4);
        if (no_qual) for (uint32_t k = 0; k < l_seq; ++k) o.b(0xFF);
        else for (uint32_t k = 0; k < l_seq; ++k) o.b(t[qa + k] - 33u);
    }
    uint32_t size = 4 + 32 + (uint32_t)l_qname + 1 + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    // optional fields  TG:T:value
    uint64_t p = nt == 11 ? tab[10] + 1 : le;
    while (p < le) {
        uint64_t q = p;
        while (q < le && t[q] != '\t') ++q;
        if (q - p < 5 || t[p + 2] != ':' || t[p + 4] != ':') { atomicOr(err, (uint32_t)BE_TAG); return 0; }
        const uint8_t ty = t[p + 3];
        const uint64_t va = p + 5, vb = q;
        if (WRITE) { o.b(t[p]); o.b(t[p + 1]); }
        size += 2;
        bool tok = true;
        if (ty == 'A' || ty == 'a' || ty == 'c' || ty == 'C') {      // (htslib reads the lower-case forms of the BAM types as A)
            if (vb - va != 1) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            if (WRITE) { o.b('A'); o.b(t[va]); }
            size += 2;
        } else if (ty == 'i' || ty == 'I') {
            const bool neg = va < vb && t[va] == '-';
            const int64_t x = dec_s(t, va, vb, &tok);
            if (!tok || x < -0x80000000ll || x > 0xffffffffll) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            char c; uint32_t w;
            if (neg) { if (x >= -128) { c = 'c'; w = 1; } else if (x >= -32768) { c = 's'; w = 2; } else { c = 'i'; w = 4; } }
            else { if (x <= 255) { c = 'C'; w = 1; } else if (x <= 65535) { c = 'S'; w = 2; } else { c = 'I'; w = 4; } }
            if (WRITE) { o.b((uint8_t)c); if (w == 1) o.b((uint32_t)x); else if (w == 2) o.h((uint32_t)x); else o.w((uint32_t)x); }
            size += 1 + w;
        } else if (ty == 'f') {
            const float f = dec_f(t, va, vb, &tok);
            if (!tok) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            if (WRITE) { o.b('f'); o.w(__float_as_uint(f)); }
            size += 5;
        } else if (ty == 'Z' || ty == 'H') {
            if (WRITE) { o.b(ty); for (uint64_t k = va; k < vb; ++k) o.b(t[k]); o.b(0); }
            size += 2 + (uint32_t)(vb - va);
        } else if (ty == 'B') {
            if (va >= vb) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            const uint8_t sub = t[va];
            uint32_t w = 0;
            switch (sub) { case 'c': case 'C': w = 1; break; case 's': case 'S': w = 2; break; case 'i': case 'I': case 'f': w = 4; break; default: break; }
            if (!w) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            uint32_t cnt = 0;
            for (uint64_t k = va + 1; k < vb; ++k) if (t[k] == ',') ++cnt;
            if (va + 1 < vb && t[va + 1] != ',') { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            if (WRITE) {
                o.b('B'); o.b(sub); o.w(cnt);
                uint64_t k = va + 2;
                for (uint32_t i = 0; i < cnt; ++i) {
                    uint64_t e = k;
                    while (e < vb && t[e] != ',') ++e;
                    if (sub == 'f') o.w(__float_as_uint(dec_f(t, k, e, &tok)));
                    else { const int64_t x = dec_s(t, k, e, &tok); if (w == 1) o.b((uint32_t)x); else if (w == 2) o.h((uint32_t)x); else o.w((uint32_t)x); }
                    k = e + 1;
                }
            } else {
                uint64_t k = va + 2;
                for (uint32_t i = 0; i < cnt; ++i) {
                    uint64_t e = k;
                    while (e < vb && t[e] != ',') ++e;
                    if (sub == 'f') (void)dec_f(t, k, e, &tok);
                    else {                                  // every element inside its subtype's range (htslib rejects the line otherwise; no silent wrap)
                        const int64_t x = dec_s(t, k, e, &tok);
                        const int64_t lo = sub == 'c' ? -128 : sub == 's' ? -32768 : sub == 'i' ? -2147483648ll : 0;
                        const int64_t hi = sub == 'c' ? 127 : sub == 'C' ? 255 : sub == 's' ? 32767 : sub == 'S' ? 65535 : sub == 'i' ? 2147483647ll : 4294967295ll;
                        if (x < lo || x > hi) tok = false;
                    }
                    k = e + 1;
                }
            }
            if (!tok) { atomicOr(err, (uint32_t)BE_TAG); return 0; }
            size += 2 + 4 + cnt * w;
        } else { atomicOr(err, (uint32_t)BE_TAG); return 0; }
        p = q + 1;
    }
    if (WRITE) { o.flush(); uint8_t* h = out; put32(h, size - 4); }
    if (ix) { ix->tid = tid; ix->beg = pos; ix->end = (int32_t)(end > 0x7fffffffll ? 0x7fffffffll : end); ix->bin = (bin & 0xFFFFu) | ((uint32_t)flag << 16); }      // (a position past 2^29 gives a bin beyond 16 bits: the host makes no index then)
    return size;
}

// pass 1: size of every line's record + its sort key ((tid, -1 last) | pos + 1 | reverse strand), idx = line
__global__ void k_bam_keys(const uint8_t* text, const uint64_t* starts, uint64_t nlines, RefTab rt, SortRec* rec, uint32_t* size, uint32_t* err) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nlines) return;
    BamIdx ix;
    ix.tid = -1; ix.beg = -1; ix.end = 0; ix.bin = 0;
    uint64_t le = starts[j + 1] - 1;
    const uint64_t ls = starts[j];
    if (le > ls && text[le - 1] == '\r') --le;
    const uint32_t sz = bam_record<false>(text, ls, le, rt, nullptr, &ix, err);
    size[j] = sz;
    SortRec r;
    const uint64_t tkey = ix.tid < 0 ? (uint64_t)rt.nref : (uint64_t)ix.tid;
    r.hi = (tkey << 33) | ((uint64_t)(uint32_t)(ix.beg + 1) << 1) | ((ix.bin >> 20) & 1u);       // FLAG 0x10: reverse strand
    r.lo = 0; r.idx = (uint32_t)j;
    rec[j] = r;
}
__global__ void k_bam_sizes(const SortRec* rec, const uint32_t* size, uint64_t n, uint64_t* off) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) off[r] = size[rec[r].idx];
}
// pass 2: the records, in file order
__global__ void k_bam_write(const uint8_t* text, const uint64_t* starts, uint64_t n, RefTab rt, const SortRec* rec, const uint64_t* off, uint8_t* raw, BamIdx* idx, uint32_t* err) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t j = rec[r].idx;
    uint64_t le = starts[j + 1] - 1;
    const uint64_t ls = starts[j];
    if (le > ls && text[le - 1] == '\r') --le;
    BamIdx ix;
    (void)bam_record<true>(text, ls, le, rt, raw + off[r], &ix, err);
    idx[r] = ix;
}

// ---- BAI reductions -------------------------------------------------------------------------------------------------------
struct BaiHead { uint32_t r; int32_t tid; uint32_t bin; uint32_t pad; uint64_t voff; };
struct BaiRef { unsigned long long n_mapped, n_unmapped, beg, end; };          // beg: min start voffset, end: max end voffset
// Where the records of one launch sit in the file: record r starts at the uncompressed offset ubase + off[r]; coff[k] is the
// compressed offset of block blk0 + k relative to cbase (the compressed bytes before block blk0).  One launch over the whole
// file: {hdr_len, 0, 0}; a window of a stream: the blocks compressed so far lie before blk0.
struct VoffMap { uint64_t ubase, blk0, cbase; };
__device__ inline uint64_t voffset(uint64_t uoff, const uint64_t* coff, const VoffMap& vm) {
    const uint64_t b = uoff / BGZF_RAW;
    return ((vm.cbase + coff[b - vm.blk0]) << 16) | (uoff - b * BGZF_RAW);
}
// prev: the record before idx[0] (the last of the previous window), or null.  no_coor: [0] records without coordinates, [1] "no
// index possible", [2] atomicMin of the virtual offsets of records without coordinates (the first of them: they sort last).
__global__ void k_bai(const BamIdx* idx, const uint64_t* off /* [n + 1] */, uint64_t n, VoffMap vm, const uint64_t* coff, const uint64_t* lin_off, uint32_t nref,
                      unsigned long long* lin, BaiRef* refs, uint64_t* head_flag /* [n]: 1 where a run of records in one bin starts */, unsigned long long* no_coor,
                      const BamIdx* prev) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) head_flag[r] = 0;
    const int lane = threadIdx.x & 63;
    BamIdx x;
    x.tid = -1; x.beg = 0; x.end = 0; x.bin = 0;
    if (r < n) x = idx[r];
    const bool placed = r < n && x.tid >= 0;
    const uint64_t nc = __ballot(r < n && x.tid < 0);
    if (nc && lane == (int)__builtin_ctzll(nc)) {
        atomicAdd(no_coor, (unsigned long long)__popcll(nc));
        atomicMin(no_coor + 2, (unsigned long long)voffset(vm.ubase + off[r], coff, vm));
    }
    const uint64_t pm = __ballot(placed);
    if (!pm) return;
    uint64_t v0 = 0, v1 = 0;
    if (placed) { v0 = voffset(vm.ubase + off[r], coff, vm); v1 = voffset(vm.ubase + off[r + 1], coff, vm); }
    const uint32_t bin = x.bin & 0xFFFFu;
    const bool unm = (x.bin >> 18) & 1u;                           // FLAG 0x4
    // per-reference counts and file range: the records are sorted, so a wave nearly always holds ONE reference -> one set of atomics
    const int first = (int)__builtin_ctzll(pm);
    const int32_t tid0 = __shfl(x.tid, first, 64);
    if (__ballot(placed && x.tid == tid0) == pm) {
        const uint32_t cu = (uint32_t)__popcll(__ballot(placed && unm)), cm = (uint32_t)__popcll(pm) - cu;
        uint64_t lo = placed ? v0 : ~0ull, hi = placed ? v1 : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t a = (uint64_t)__shfl_xor((long long)lo, d, 64), b = (uint64_t)__shfl_xor((long long)hi, d, 64);
            lo = a < lo ? a : lo; hi = b > hi ? b : hi;
        }
        if (lane == first) {
            BaiRef* R = &refs[tid0];
            if (cm) atomicAdd(&R->n_mapped, (unsigned long long)cm);
            if (cu) atomicAdd(&R->n_unmapped, (unsigned long long)cu);
            atomicMin(&R->beg, (unsigned long long)lo);
            atomicMax(&R->end, (unsigned long long)hi);
        }
    } else if (placed) {
        BaiRef* R = &refs[x.tid];
        if (unm) atomicAdd(&R->n_unmapped, 1ull); else atomicAdd(&R->n_mapped, 1ull);
        atomicMin(&R->beg, (unsigned long long)v0);
        atomicMax(&R->end, (unsigned long long)v1);
    }
    if (!placed) return;
    const uint64_t nwin = lin_off[x.tid + 1] - lin_off[x.tid];
    int64_t w0 = x.beg < 0 ? 0 : (x.beg >> 14), w1 = (x.end > 0 ? x.end - 1 : 0) >> 14;
    if (w1 < w0) w1 = w0;
    for (int64_t w = w0; w <= w1 && (uint64_t)w < nwin; ++w) atomicMin(&lin[lin_off[x.tid] + (uint64_t)w], (unsigned long long)v0);
    // a record that reaches past its reference's LN (the linear index is sized by LN) or past the 2^29 bases a BAI can address:
    // no index can describe it (no_coor[1] != 0 -> the host writes none and says why)
    if ((uint64_t)w1 >= nwin || x.end > (1 << 29) || bin > 37449u) atomicOr(no_coor + 1, 1ull);
    bool head = r == 0 && !prev;
    if (!head) { const BamIdx y = r ? idx[r - 1] : *prev; head = y.tid != x.tid || (y.bin & 0xFFFFu) != bin; }
    if (head) head_flag[r] = 1;
}
// the run starts, in file order (head_pos = exclusive scan of head_flag)
__global__ void k_bai_heads(const BamIdx* idx, const uint64_t* off, uint64_t n, VoffMap vm, const uint64_t* coff, const uint64_t* head_pos, BaiHead* heads, const BamIdx* prev) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const BamIdx x = idx[r];
    if (x.tid < 0) return;
    bool head = r == 0 && !prev;
    if (!head) { const BamIdx y = r ? idx[r - 1] : *prev; head = y.tid != x.tid || ((y.bin ^ x.bin) & 0xFFFFu) != 0u; }
    if (!head) return;
    BaiHead h;
    h.r = (uint32_t)r; h.tid = x.tid; h.bin = x.bin & 0xFFFFu; h.pad = 0; h.voff = voffset(vm.ubase + off[r], coff, vm);
    heads[head_pos[r]] = h;
}

// ---- out-of-core mode: run formation and the merge of the runs -----------------------------------------------------------------
// What a run file keeps per record besides its bytes, in the run's sorted order: the sort key, the record's size, what the index
// needs.
struct SpillRec { uint64_t hi; uint32_t size, pad; BamIdx ix; };
static_assert(sizeof(SpillRec) == 32, "run key file layout");

// position + 1 of the last (mode 0: atomicMax) or first (mode 1: atomicMin, ~0 = none) newline in text[a, b)
__global__ void k_find_nl(const uint8_t* text, uint64_t a, uint64_t b, int first, unsigned long long* out) {
    unsigned long long best = first ? ~0ull : 0ull;
    for (uint64_t p = a + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < b; p += (uint64_t)gridDim.x * blockDim.x)
        if (text[p] == '\n') { const unsigned long long v = p + 1; best = first ? (v < best ? v : best) : (v > best ? v : best); }
    if (first) { if (best != ~0ull) atomicMin(out, best); }
    else if (best) atomicMax(out, best);
}
// a run's records in sorted order -> what its key file holds
__global__ void k_spill_recs(const SortRec* rec, const uint32_t* size, const BamIdx* idx, uint64_t n, SpillRec* out) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    SpillRec x;
    x.hi = rec[r].hi; x.size = size[rec[r].idx]; x.pad = 0; x.ix = idx[r];
    out[r] = x;
}
// merge: the safe records of a round, concatenated in run order -> sort records (idx = place in the concatenation)
__global__ void k_merge_keys(const SpillRec* in, uint64_t n, SortRec* rec) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SortRec r;
    r.hi = in[i].hi; r.lo = 0; r.idx = (uint32_t)i;
    rec[i] = r;
}
__global__ void k_merge_sizes(const SortRec* rec, const SpillRec* in, uint64_t n, uint64_t* off, BamIdx* idx) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const SpillRec& x = in[rec[r].idx];
    off[r] = x.size;
    idx[r] = x.ix;
}
// the records in merged order: one wave per record, 64 consecutive bytes per step (a record is a few hundred bytes; source
// and destination offsets are arbitrary, so the lanes move single bytes -- coalesced across the wave)
constexpr int MG_WAVES = 4;
__global__ __launch_bounds__(64 * MG_WAVES) void k_merge_gather(const uint8_t* src, const uint64_t* src_off, const SortRec* rec, const SpillRec* in, uint64_t n,
                                                                const uint64_t* off, uint8_t* dst) {
    const uint64_t r = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t j = rec[r].idx;
    const uint32_t size = in[j].size;
    const uint8_t* s = src + src_off[j];
    uint8_t* d = dst + off[r];
    for (uint32_t i = lane; i < size; i += 64u) d[i] = s[i];
}

}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------
struct BamHeader {                                     // the parsed header: BAM header bytes, reference dictionary, the lookup table's host side
    std::string hdr;
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    uint32_t tcap = 64;
    std::vector<unsigned long long> th;
    std::vector<int32_t> tidv;
    std::vector<uint32_t> noff;
    std::string blob;
};
struct SpillRun { uint64_t data_off = 0, key_off = 0, nrec = 0; };      // a sorted run: its records and keys in the two temporary files
struct SpillCur {                                      // a run's window during the merge
    uint64_t next = 0, data_next = 0;                  // first record / byte not yet loaded
    std::vector<SpillRec> keys;                        // loaded, not yet emitted
    std::string bytes;
};
struct BgzfStream {                                    // BGZF output of a stream: d_win = the partial last block (carry bytes), then the current window
    LedgerBuf<uint8_t> d_win;
    uint64_t carry = 0, blk0 = 0, cbase = 0;           // blk0: file block at d_win[0]; cbase: compressed bytes before it
    LedgerBuf<uint8_t> d_comp, d_pack;                 // (these four: grow-only)
    LedgerBuf<uint64_t> d_csize;
    LedgerBuf<uint32_t> d_scratch;
};
struct BaiAcc {                                        // the index across the windows of a file (the single pass: one window): small arrays that stay resident
    bool on = false, has_prev = false;
    std::vector<uint64_t> lin_off;
    LedgerBuf<uint64_t> d_lin_off;
    LedgerBuf<unsigned long long> d_lin, d_nocoor;
    LedgerBuf<BaiRef> d_refs;
    LedgerBuf<BamIdx> d_prev;
    LedgerBuf<uint64_t> d_hflag;                       // per window (grow-only)
    LedgerBuf<BaiHead> d_heads;
    std::vector<BaiHead> heads;
    uint64_t end_voff = 0;
};
struct MergeBufs {                                     // one merge round on the device (grow-only)
    LedgerBuf<SpillRec> rec;
    LedgerBuf<uint64_t> src, off;
    LedgerBuf<uint8_t> bytes;
    LedgerBuf<SortRec> rA, rB;
    LedgerBuf<uint32_t> hist;
    LedgerBuf<BamIdx> idx;
};
struct BamTabs {                                       // what bam_setup puts on the device: the name table, the CRC tables, the error word; find_nl's word
    LedgerBuf<uint8_t> rt[4];
    LedgerBuf<CrcTabs> ct;
    LedgerBuf<uint32_t> err;
    LedgerBuf<unsigned long long> nl;
};

struct mkt_bam {
    int device = 0;
    DevStream stream;                                   // (first: it goes last)
    // device bytes held by this object: every device buffer below is a LedgerBuf charged to it.  limit = $MKT_BAM_DEVICE_LIMIT: the
    // device bytes this object may hold (as if HBM ended there)
    DevLedger led;
    LedgerBuf<uint8_t> d_text; size_t cap = 0, len = 0;
    uint64_t tstart = 0;                                // text before this offset has gone into runs (out-of-core mode)
    bool header_done = false, ran = false;
    std::string header, pending;
    LedgerBuf<uint8_t> d_bam; uint64_t bam_len = 0;
    std::string bai;
    uint64_t records = 0;
    // pinned staging for callers that move files (mkt_bam_window / _commit / _read / _pull): two slots, used alternately
    PinBuf<char> h_io[2];
    DevEvents<2> ev_io;
    bool io_busy[2] = {false, false};
    int io_slot = 0;
    std::string err, note;
    // out-of-core mode (mkt_bam_spill)
    bool spill_set = false, autob = false, spilled = false;
    uint64_t budget = 0;                                // text bytes per run; 0 = single pass
    int sp_sorted = 1, sp_level = 2;
    std::string tmp_path[2];                            // records, keys
    int tmp_fd[2] = {-1, -1};
    bool tmp_made[2] = {false, false};                  // created by this object (only those are removed)
    PinBuf<char> h_stage;                               // pinned staging of run data on its way to the temporary files
    uint64_t tmp_bytes = 0, nruns = 0, rounds = 0;
    std::vector<SpillRun> runs;
    std::vector<SpillCur> cur;
    bool hdr_ready = false;
    BamHeader H;
    RefTab rt{};
    BamTabs tb;
    BgzfStream bs;
    BaiAcc bx;
    MergeBufs mb;
    std::string outq; size_t outq_pos = 0;              // compressed bytes not yet pulled
    uint64_t out_total = 0, pull_off = 0;
    bool merging = false, done = false;
    double t_form = 0, t_merge = 0;
};
constexpr size_t kBamIoCap = (size_t)64 << 20;
static int bfail(mkt_bam* s, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (s) s->err = buf;
    return code;
}
#define BCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bfail((s), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// `bytes` for a device buffer of this object: a new allocation / only if they do not fit yet (grow-only, contents not kept)
template <typename T>
static int dev_alloc(mkt_bam* s, LedgerBuf<T>& b, size_t bytes, bool grow = false) {
    const hipError_t e = grow ? b.grow(s->led, bytes) : b.alloc(s->led, bytes);
    if (e != hipSuccess) return bfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return MKT_OK;
}
template <typename T>
static int dev_grow(mkt_bam* s, LedgerBuf<T>& b, size_t bytes) { return dev_alloc(s, b, bytes, true); }
static uint64_t device_free(mkt_bam* s) {                           // what this object may still allocate
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    if (s->led.limit) { const uint64_t l = s->led.limit > s->led.now ? s->led.limit - s->led.now : 0; if (l < fr) fr = (size_t)l; }
    return fr;
}
// the end of a conversion: what the object holds on the device besides the text and the BAM goes
static void bam_release_work(mkt_bam* s) { s->bs = BgzfStream(); s->mb = MergeBufs(); s->bx = BaiAcc(); s->tb = BamTabs(); }
struct PhaseMarks {                                    // MKT_VERBOSE: the time since the previous mark (call sites follow a stream synchronisation)
    bool on;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mkt_bam] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    }
};

// room for `need` bytes of text counted from tstart (the text before tstart is dropped)
static int bam_reserve(mkt_bam* s, size_t need) {
    if (s->tstart + need <= s->cap) return MKT_OK;
    size_t ncap = s->cap ? s->cap : ((size_t)64 << 20);
    if (!s->cap && s->budget && ncap > 2 * s->budget + ((size_t)1 << 20)) ncap = 2 * s->budget + ((size_t)1 << 20);     // runs: sized by the budget
    while (ncap < need) ncap *= 2;
    LedgerBuf<uint8_t> nb;
    // (doubling keeps old and new side by side during the copy; when that does not fit: just enough; when that does not either, the
    //  input is larger than one GPU takes -- text + records + compressed blocks are resident together, ~2.2 x the .sam: INTEGRATION.md)
    hipError_t e = nb.alloc(s->led, ncap + 64);
    if (e != hipSuccess) { ncap = need + ((size_t)64 << 20); e = nb.alloc(s->led, ncap + 64); }
    if (e != hipSuccess) { ncap = need; e = nb.alloc(s->led, ncap + 64); }
    if (e != hipSuccess) {
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        return bfail(s, MKT_E_NOMEM, "the SAM input (%.1f GB so far) does not fit this GPU (%.1f of %.1f GB free): sam2bam keeps the whole input in HBM "
                     "unless it is given a run budget (sam2bam -m, mkt_bam_spill); convert the modes' .sam files one by one", (double)need / 1e9, (double)fr / 1e9, (double)tot / 1e9);
    }
    if (s->d_text) {
        BCHK(s, hipStreamSynchronize(s->stream));
        if (s->len > s->tstart) BCHK(s, hipMemcpy(nb, s->d_text + s->tstart, s->len - s->tstart, hipMemcpyDeviceToDevice));
    }
    s->len -= s->tstart; s->tstart = 0;
    s->d_text = std::move(nb); s->cap = ncap;                   // (the old text goes here, after the copy)
    return MKT_OK;
}
static void put_le32(std::string& s, uint32_t v) { char b[4] = {(char)v, (char)(v >> 8), (char)(v >> 16), (char)(v >> 24)}; s.append(b, 4); }
static void put_le64(std::string& s, uint64_t v) { put_le32(s, (uint32_t)v); put_le32(s, (uint32_t)(v >> 32)); }

// header: text (with @HD SO:coordinate when sorting), the reference dictionary from @SQ, the BAM header bytes, the name table
static int bam_parse_header(mkt_bam* s, bool sorted, BamHeader& H) {
    std::string text = s->header;
    std::vector<std::string>& names = H.names;
    std::vector<uint32_t>& lens = H.lens;
    {
        size_t p = 0;
        while (p < text.size()) {
            size_t e = text.find('\n', p);
            if (e == std::string::npos) e = text.size();
            if (e - p >= 3 && text.compare(p, 3, "@SQ") == 0) {
                std::string sn;
                long long ln = -1;
                size_t q = p;
                while (q < e) {
                    size_t f = text.find('\t', q);
                    if (f == std::string::npos || f > e) f = e;
                    if (f - q > 3 && text.compare(q, 3, "SN:") == 0) sn = text.substr(q + 3, f - q - 3);
                    if (f - q > 3 && text.compare(q, 3, "LN:") == 0) ln = atoll(text.substr(q + 3, f - q - 3).c_str());
                    q = f + 1;
                }
                if (sn.empty() || ln < 0 || ln > 0x7fffffffll) return bfail(s, MKT_E_ARG, "bad @SQ line in the header (SN / LN)");
                names.push_back(sn); lens.push_back((uint32_t)ln);
            }
            p = e + 1;
        }
        if (sorted) {
            if (text.compare(0, 3, "@HD") == 0) {
                size_t e = text.find('\n');
                if (e == std::string::npos) e = text.size();
                std::string hd = text.substr(0, e), out;
                size_t q = 0;
                bool had = false;
                while (q <= hd.size()) {
                    size_t f = hd.find('\t', q);
                    if (f == std::string::npos) f = hd.size();
                    std::string fld = hd.substr(q, f - q);
                    if (fld.compare(0, 3, "SO:") == 0) { fld = "SO:coordinate"; had = true; }
                    if (fld.compare(0, 3, "GO:") != 0) { if (!out.empty()) out += '\t'; out += fld; }       // (a grouping claim does not survive a sort)
                    q = f + 1;
                }
                if (!had) out += "\tSO:coordinate";
                text = out + text.substr(e);
            } else text = "@HD\tVN:1.6\tSO:coordinate\n" + text;
        }
    }
    const uint32_t nref = (uint32_t)names.size();
    std::string& hdr = H.hdr;                                      // SAMv1 4.2: magic, l_text, text, n_ref, (l_name, name, l_ref)*
    hdr.append("BAM\1", 4);
    put_le32(hdr, (uint32_t)text.size());
    hdr += text;
    put_le32(hdr, nref);
    for (uint32_t i = 0; i < nref; ++i) { put_le32(hdr, (uint32_t)names[i].size() + 1); hdr += names[i]; hdr += '\0'; put_le32(hdr, lens[i]); }
    // reference table for the device
    uint32_t& tcap = H.tcap;
    tcap = 64;
    while (tcap < 4 * nref + 4) tcap <<= 1;
    H.th.assign(tcap, 0ull);
    H.tidv.assign(tcap, -1);
    H.noff.assign(nref + 1, 0);
    std::vector<unsigned long long>& th = H.th;
    std::vector<int32_t>& tidv = H.tidv;
    std::string& blob = H.blob;
    for (uint32_t i = 0; i < nref; ++i) {
        H.noff[i] = (uint32_t)blob.size(); blob += names[i];
        unsigned long long h = 0xcbf29ce484222325ull;
        for (unsigned char c : names[i]) { h ^= c; h *= 0x100000001b3ull; }
        if (!h) h = 1;
        uint32_t k = (uint32_t)(h >> 20) & (tcap - 1);
        bool dup = false;
        while (th[k]) { if (th[k] == h && names[(size_t)tidv[k]] == names[i]) { dup = true; break; } k = (k + 1) & (tcap - 1); }
        if (dup) return bfail(s, MKT_E_ARG, "reference name %s twice in the header", names[i].c_str());
        th[k] = h; tidv[k] = (int32_t)i;
    }
    H.noff[nref] = (uint32_t)blob.size();
    return MKT_OK;
}

static bool bai_possible(const BamHeader& H) {                     // the BAI format ends at 2^29 bases per reference
    for (uint32_t l : H.lens) if (l > (1u << 29)) return false;
    return true;
}
static void bai_lin_off(const BamHeader& H, std::vector<uint64_t>& lin_off) {
    const uint32_t nref = (uint32_t)H.names.size();
    lin_off.assign(nref + 1, 0);
    for (uint32_t i = 0; i < nref; ++i) lin_off[i + 1] = lin_off[i] + ((uint64_t)H.lens[i] >> 14) + 2;
}
// The .bai from what the reductions gathered: the bin-run heads in file order, per-reference counts and ranges, the linear index,
// the virtual offset where the records without coordinates start (or the data ends).
static void bai_assemble(mkt_bam* s, uint32_t nref, const std::vector<uint64_t>& lin_off, const std::vector<BaiRef>& refs, std::vector<unsigned long long>& lin,
                         const std::vector<BaiHead>& heads, unsigned long long no_coor, unsigned long long beyond, uint64_t off_end) {
    const uint64_t nheads = heads.size(), nlin = lin_off[nref];
    // per reference (the run starts come in file order = by reference): a stable counting sort by bin
    std::vector<uint32_t> bin_cnt(65536, 0), bin_at(65536, 0);      // (every 16-bit value: a record past 2^29 bases carries a bin beyond 37449; no index is kept then, see below)
    std::vector<uint32_t> order(nheads);
    std::vector<std::pair<size_t, size_t>> ref_range(nref, {0, 0});
    {
        size_t i = 0;
        for (uint32_t t = 0; t < nref && i < nheads; ++t) {
            size_t j = i;
            while (j < nheads && (uint32_t)heads[j].tid == t) ++j;
            ref_range[t] = {i, j};
            i = j;
        }
    }
    std::string& o = s->bai;                                        // SAMv1 5.2
    o.reserve(64 + (size_t)nheads * 28 + nlin * 8 + (size_t)nref * 64);
    o.append("BAI\1", 4);
    put_le32(o, nref);
    for (uint32_t t = 0; t < nref; ++t) {
        const bool any = refs[t].n_mapped + refs[t].n_unmapped > 0;
        const size_t i0 = ref_range[t].first, i1 = ref_range[t].second;
        std::vector<uint32_t> used;                                 // the bins of this reference, ascending
        for (size_t i = i0; i < i1; ++i) if (bin_cnt[heads[i].bin]++ == 0) used.push_back(heads[i].bin);
        std::sort(used.begin(), used.end());
        uint32_t at = 0;
        for (uint32_t b : used) { bin_at[b] = at; at += bin_cnt[b]; }
        for (size_t i = i0; i < i1; ++i) order[i0 + bin_at[heads[i].bin]++] = (uint32_t)i;
        put_le32(o, (uint32_t)used.size() + (any ? 1u : 0u));
        size_t k = i0;
        for (uint32_t b : used) {
            put_le32(o, b);
            put_le32(o, bin_cnt[b]);
            for (uint32_t c = 0; c < bin_cnt[b]; ++c, ++k) {
                const size_t i = order[k];
                put_le64(o, heads[i].voff);
                put_le64(o, i + 1 < nheads ? heads[i + 1].voff : off_end);
            }
            bin_cnt[b] = 0;
        }
        if (any) {                                                  // the pseudo-bin: file range of the reference, mapped / unmapped counts
            put_le32(o, 37450u); put_le32(o, 2u);
            put_le64(o, refs[t].beg); put_le64(o, refs[t].end);
            put_le64(o, refs[t].n_mapped); put_le64(o, refs[t].n_unmapped);
        }
        // linear index: up to the last window that a record touched; empty windows take the next one's offset
        const uint64_t a = lin_off[t], b = lin_off[t + 1];
        uint64_t last = a;
        for (uint64_t k = a; k < b; ++k) if (lin[k] != ~0ull) last = k + 1;
        unsigned long long nextv = 0;
        for (uint64_t k = last; k > a;) { --k; if (lin[k] == ~0ull) lin[k] = nextv; else nextv = lin[k]; }
        put_le32(o, (uint32_t)(last - a));
        for (uint64_t k = a; k < last; ++k) put_le64(o, lin[k]);
    }
    put_le64(o, no_coor);
    if (beyond) {
        s->bai.clear();
        s->note = "no index written: a record lies past its reference's LN or past the 2^29 bases a BAI index can address (samtools index would need -c)";
    }
}
static const char kNoIndexLongRef[] = "no index written: a reference is longer than the 2^29 bases a BAI index can address (samtools index would need -c)";
// ---- the steps of a conversion: the single pass and the out-of-core mode both go through these -------------------------------
// compress nblocks blocks of raw; csize becomes the blocks' compressed offsets, csize[nblocks] and (after a synchronisation)
// *ctot their total.  The buffers and the launch batch are the caller's.
static int bgzf_compress(mkt_bam* s, const uint8_t* raw, uint64_t nraw, uint64_t nblocks, int level, uint8_t* comp, uint64_t* csize, uint32_t* scratch,
                         uint64_t batch, uint64_t* ctot) {
    hipStream_t st = s->stream;
    BCHK(s, bgzf_launch(raw, nraw, nblocks, level, s->tb.ct, comp, csize, scratch, batch, st));
    BCHK(s, launch_exscan(csize, nblocks, csize + nblocks, st));
    BCHK(s, hipMemcpyAsync(ctot, csize + nblocks, sizeof *ctot, hipMemcpyDeviceToHost, st));
    return MKT_OK;
}
// the header is known (the first alignment line has arrived, or the input has ended): parse it once, put the name table, the
// CRC tables and the error word on the device
static int bam_setup(mkt_bam* s, bool sorted) {
    if (s->hdr_ready) return MKT_OK;
    int rc = bam_parse_header(s, sorted, s->H);
    if (rc) return rc;
    const BamHeader& H = s->H;
    const uint32_t nref = (uint32_t)H.names.size();
    hipStream_t st = s->stream;
    const size_t sz[4] = {H.tcap * sizeof(unsigned long long), H.tcap * sizeof(int32_t), (nref + 1) * sizeof(uint32_t), H.blob.size() + 16};
    const void* src[4] = {H.th.data(), H.tidv.data(), H.noff.data(), H.blob.data()};
    for (int k = 0; k < 4; ++k) {
        BCHK(s, s->tb.rt[k].alloc(s->led, sz[k]));
        if (k < 3 || !H.blob.empty()) BCHK(s, hipMemcpyAsync(s->tb.rt[k], src[k], k < 3 ? sz[k] : H.blob.size(), hipMemcpyHostToDevice, st));
    }
    CrcTabs ct;
    crc_tables(&ct);
    BCHK(s, s->tb.ct.alloc(s->led, sizeof(CrcTabs)));
    BCHK(s, s->tb.err.alloc(s->led, 256));
    BCHK(s, hipMemcpyAsync(s->tb.ct, &ct, sizeof ct, hipMemcpyHostToDevice, st));
    BCHK(s, hipMemsetAsync(s->tb.err, 0, 256, st));
    BCHK(s, hipStreamSynchronize(st));
    s->rt.hash = (const unsigned long long*)s->tb.rt[0].get(); s->rt.id = (const int32_t*)s->tb.rt[1].get(); s->rt.name_off = (const uint32_t*)s->tb.rt[2].get();
    s->rt.names = (const uint8_t*)s->tb.rt[3].get(); s->rt.mask = H.tcap - 1; s->rt.nref = nref;
    s->hdr_ready = true;
    return MKT_OK;
}

// the bits of the sort key: strand and position, then the reference id (one more value than references: "none" sorts last)
static int bam_key_bits(const mkt_bam* s) {
    int tbits = 1;
    while ((1ull << tbits) <= (uint64_t)s->rt.nref) ++tbits;
    return 33 + tbits;
}
// resident text (whole lines) as records: the line starts, the keys in output order, the records' sizes and their offsets in
// the output (off[nl] = total).  The buffers go with the struct, or earlier where the caller resets them.
struct BamRecs {
    LedgerBuf<uint64_t> d_starts, d_off;
    LedgerBuf<SortRec> rA, rB;                        // (rB and d_hist: the sort's other buffer and its histograms)
    LedgerBuf<uint32_t> d_size, d_hist;
    uint64_t nl = 0, total = 0;
    unsigned grid() const { return (unsigned)((nl + 255) / 256); }
};
static int bam_records(mkt_bam* s, const uint8_t* text, uint64_t len, bool sorted, PhaseMarks& mark, BamRecs* out) {
    hipStream_t st = s->stream;
    BamRecs& R = *out;
    int rc;
    if (len) {
        uint64_t* starts = nullptr;
        const hipError_t e = sort_line_index(text, len, st, &starts, &R.nl);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return bfail(s, MKT_E_NOMEM, "the line index does not fit beside the text"); }
        if (e != hipSuccess) return bfail(s, MKT_E_HIP, "sort_line_index failed: %s", hipGetErrorString(e));
        R.d_starts.adopt(s->led, starts, (R.nl + 2) * sizeof(uint64_t));
    }
    mark("header + line index");
    const uint64_t nl = R.nl;
    if (nl >= (1ull << 32) - 1) return bfail(s, MKT_E_ARG, "%llu lines: records are indexed with 32 bits", (unsigned long long)nl);
    if (!nl) return MKT_OK;
    if ((rc = dev_alloc(s, R.rA, (nl + 1) * sizeof(SortRec))) || (rc = dev_alloc(s, R.d_size, (nl + 1) * sizeof(uint32_t))) || (rc = dev_alloc(s, R.d_off, (nl + 2) * sizeof(uint64_t)))) return rc;
    hipLaunchKernelGGL(k_bam_keys, dim3(R.grid()), dim3(256), 0, st, text, (const uint64_t*)R.d_starts, nl, s->rt, R.rA, R.d_size, s->tb.err);
    if (sorted) {
        if ((rc = dev_alloc(s, R.rB, (nl + 1) * sizeof(SortRec))) || (rc = dev_alloc(s, R.d_hist, kSortHistBytes))) return rc;
        SortRec *a = R.rA, *b = R.rB;
        sort_radix_passes(a, b, nl, R.d_hist, 1, 0, bam_key_bits(s), st);
        if (a != R.rA.get()) std::swap(R.rA, R.rB);                 // (the passes leave the result in `a`: rA holds it, as before)
    }
    uint32_t herr = 0;
    BCHK(s, hipMemcpyAsync(&herr, s->tb.err, sizeof herr, hipMemcpyDeviceToHost, st));
    BCHK(s, hipStreamSynchronize(st));
    if (herr) return bfail(s, MKT_E_ARG, "not SAM alignment text (error bits 0x%x: 1 fewer than 11 fields, 2 reference name not in the header, 4 number, 8 CIGAR, 16 optional field, 32 SEQ / QUAL lengths, 64 QNAME length)", herr);
    mark(sorted ? "keys + radix sort" : "keys");
    hipLaunchKernelGGL(k_bam_sizes, dim3(R.grid()), dim3(256), 0, st, (const SortRec*)R.rA, (const uint32_t*)R.d_size, nl, R.d_off);
    BCHK(s, launch_exscan(R.d_off, nl, R.d_off + nl, st));
    BCHK(s, hipMemcpyAsync(&R.total, R.d_off + nl, sizeof R.total, hipMemcpyDeviceToHost, st));
    BCHK(s, hipStreamSynchronize(st));
    return MKT_OK;
}
// the records' bytes -> dst (at their offsets), their index fields -> d_idx
static void bam_write(mkt_bam* s, const uint8_t* text, const BamRecs& R, uint8_t* dst, BamIdx* d_idx) {
    hipLaunchKernelGGL(k_bam_write, dim3(R.grid()), dim3(256), 0, s->stream, text, (const uint64_t*)R.d_starts, R.nl, s->rt, (const SortRec*)R.rA, (const uint64_t*)R.d_off, dst, d_idx, s->tb.err);
}

// ---- the index (coordinate order only; the format ends at 2^29 bases per reference -- longer ones would need a CSI index: none
// is made then): begin, one call per window of records with the compressed offsets of the blocks they lie in, the end of the
// data, end
struct BaiWin { const BamIdx* idx; const uint64_t* off; uint64_t n; };
static int bai_begin(mkt_bam* s) {
    const BamHeader& H = s->H;
    const uint32_t nref = (uint32_t)H.names.size();
    hipStream_t st = s->stream;
    BaiAcc& x = s->bx;
    x.on = bai_possible(H);
    if (!x.on) { s->note = kNoIndexLongRef; return MKT_OK; }
    bai_lin_off(H, x.lin_off);
    const uint64_t nlin = x.lin_off[nref];
    std::vector<BaiRef> init(nref);
    for (auto& r : init) { r.n_mapped = 0; r.n_unmapped = 0; r.beg = ~0ull; r.end = 0; }
    BCHK(s, x.d_lin_off.alloc(s->led, (nref + 1) * sizeof(uint64_t)));
    BCHK(s, x.d_lin.alloc(s->led, (nlin + 1) * sizeof(unsigned long long)));
    BCHK(s, x.d_refs.alloc(s->led, (nref + 1) * sizeof(BaiRef)));
    BCHK(s, x.d_nocoor.alloc(s->led, 256));
    BCHK(s, x.d_prev.alloc(s->led, sizeof(BamIdx) + 64));
    BCHK(s, hipMemcpyAsync(x.d_lin_off, x.lin_off.data(), (nref + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    BCHK(s, hipMemsetAsync(x.d_lin, 0xFF, (nlin + 1) * sizeof(unsigned long long), st));
    if (nref) BCHK(s, hipMemcpyAsync(x.d_refs, init.data(), nref * sizeof(BaiRef), hipMemcpyHostToDevice, st));
    BCHK(s, hipMemsetAsync(x.d_nocoor, 0, 256, st));
    BCHK(s, hipMemsetAsync(x.d_nocoor + 2, 0xFF, sizeof(unsigned long long), st));
    BCHK(s, hipStreamSynchronize(st));                             // (init is a local)
    return MKT_OK;
}
static int bai_window(mkt_bam* s, const BaiWin& w, const VoffMap& vm, const uint64_t* coff) {
    BaiAcc& x = s->bx;
    if (!x.on || !w.n) return MKT_OK;
    hipStream_t st = s->stream;
    const uint64_t n = w.n;
    const unsigned grid = (unsigned)((n + 255) / 256);
    const BamIdx* prev = x.has_prev ? x.d_prev.get() : nullptr;
    int rc = dev_grow(s, x.d_hflag, (n + 2) * sizeof(uint64_t));
    if (rc) return rc;
    hipLaunchKernelGGL(k_bai, dim3(grid), dim3(256), 0, st, w.idx, w.off, n, vm, coff, (const uint64_t*)x.d_lin_off, s->rt.nref, x.d_lin, x.d_refs, x.d_hflag, x.d_nocoor, prev);
    BCHK(s, hipGetLastError());
    BCHK(s, launch_exscan(x.d_hflag, n, x.d_hflag + n, st));
    uint64_t nheads = 0;
    BCHK(s, hipMemcpyAsync(&nheads, x.d_hflag + n, sizeof nheads, hipMemcpyDeviceToHost, st));
    BCHK(s, hipStreamSynchronize(st));
    if (nheads) {
        if ((rc = dev_grow(s, x.d_heads, (nheads + 1) * sizeof(BaiHead)))) return rc;
        hipLaunchKernelGGL(k_bai_heads, dim3(grid), dim3(256), 0, st, w.idx, w.off, n, vm, coff, (const uint64_t*)x.d_hflag, x.d_heads, prev);
        BCHK(s, hipGetLastError());
        const size_t h0 = x.heads.size();
        x.heads.resize(h0 + nheads);
        BCHK(s, hipMemcpyAsync(x.heads.data() + h0, x.d_heads, nheads * sizeof(BaiHead), hipMemcpyDeviceToHost, st));
    }
    BCHK(s, hipMemcpyAsync(x.d_prev, w.idx + (n - 1), sizeof(BamIdx), hipMemcpyDeviceToDevice, st));
    x.has_prev = true;
    return MKT_OK;
}
// the data end at the uncompressed offset uo: its virtual offset (uo on a block boundary: coff[nblocks] is the scan's total)
static int bai_data_end(mkt_bam* s, uint64_t uo, const VoffMap& vm, const uint64_t* coff) {
    if (!s->bx.on) return MKT_OK;
    const uint64_t b = uo / BGZF_RAW;
    uint64_t c = 0;
    BCHK(s, hipMemcpyAsync(&c, coff + (b - vm.blk0), sizeof c, hipMemcpyDeviceToHost, s->stream));
    BCHK(s, hipStreamSynchronize(s->stream));
    s->bx.end_voff = ((vm.cbase + c) << 16) | (uo - b * BGZF_RAW);
    return MKT_OK;
}
static int bai_end(mkt_bam* s) {
    BaiAcc& x = s->bx;
    if (!x.on) return MKT_OK;
    const uint32_t nref = (uint32_t)s->H.names.size();
    std::vector<BaiRef> refs(nref);
    std::vector<unsigned long long> lin(x.lin_off[nref]);
    unsigned long long nc[3] = {0, 0, 0};
    hipStream_t st = s->stream;
    if (nref) BCHK(s, hipMemcpyAsync(refs.data(), x.d_refs, nref * sizeof(BaiRef), hipMemcpyDeviceToHost, st));
    if (!lin.empty()) BCHK(s, hipMemcpyAsync(lin.data(), x.d_lin, lin.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    BCHK(s, hipMemcpyAsync(nc, x.d_nocoor, sizeof nc, hipMemcpyDeviceToHost, st));
    BCHK(s, hipStreamSynchronize(st));
    const uint64_t off_end = nc[0] ? nc[2] : x.end_voff;            // the first record without coordinates, or the end of the data
    s->bai.clear();
    bai_assemble(s, nref, x.lin_off, refs, lin, x.heads, nc[0], nc[1], off_end);
    std::vector<BaiHead>().swap(x.heads);
    return MKT_OK;
}

// ---- out-of-core mode ------------------------------------------------------------------------------------------------------
// Built from the steps above, which the single pass uses too: bam_records and bam_write per run, bgzf_compress and bai_window per
// window of the merge.
// Run formation: the text is cut into runs of at most `budget` bytes of whole lines (a longer line is a run of its own); every run
// goes through bam_records (line index, keys, stable radix sort, size scan) and bam_write, and its sorted records are
// appended to <prefix>.runs, their keys, sizes and index fields (SpillRec) to <prefix>.keys.  The merge reads every run in
// windows; per round the records up to the smallest last-loaded record of the runs that still have records on disk, in the
// order T = (key, run, place in the run), are safe: their keys, concatenated in run order, go through the same stable radix
// sort, a scan of their sizes gives each its output offset, and k_merge_gather puts the bytes in place.  T is the order the
// stable sort of the whole input gives, so the merged file is the single-pass file byte for byte.  BGZF blocks are cut at the
// same raw offsets (the partial last block of a window is carried into the next) and the index reductions run per window.
static void spill_remove(mkt_bam* s) {
    for (int k = 0; k < 2; ++k) {
        if (s->tmp_fd[k] >= 0) { close(s->tmp_fd[k]); s->tmp_fd[k] = -1; }
        if (s->tmp_made[k]) { (void)unlink(s->tmp_path[k].c_str()); s->tmp_made[k] = false; }
    }
}
static int spill_guard(mkt_bam* s, int rc) {                       // on any error: no temporary file stays behind
    if (rc != MKT_OK && s) spill_remove(s);
    return rc;
}
static int write_all(mkt_bam* s, int k, const void* p, size_t n) {
    const char* c = (const char*)p;
    while (n) {
        const ssize_t w = write(s->tmp_fd[k], c, n);
        if (w < 0) { if (errno == EINTR) continue; return bfail(s, MKT_E_IO, "write error on the temporary file %s: %s", s->tmp_path[k].c_str(), strerror(errno)); }
        c += w; n -= (size_t)w; s->tmp_bytes += (uint64_t)w;
    }
    return MKT_OK;
}
// device bytes -> temporary file k, 64 MiB at a time through pinned memory
static int write_dev(mkt_bam* s, int k, const void* d, uint64_t n) {
    if (!s->h_stage) BCHK(s, s->h_stage.alloc(kBamIoCap));
    for (uint64_t o = 0; o < n; o += kBamIoCap) {
        const size_t m = (size_t)(n - o < kBamIoCap ? n - o : kBamIoCap);
        BCHK(s, hipMemcpyAsync(s->h_stage, (const char*)d + o, m, hipMemcpyDeviceToHost, s->stream));
        BCHK(s, hipStreamSynchronize(s->stream));
        const int rc = write_all(s, k, s->h_stage, m);
        if (rc) return rc;
    }
    return MKT_OK;
}
static int read_at(mkt_bam* s, int k, void* p, size_t n, uint64_t off) {
    char* c = (char*)p;
    while (n) {
        const ssize_t r = pread(s->tmp_fd[k], c, n, (off_t)off);
        if (r <= 0) { if (r < 0 && errno == EINTR) continue; return bfail(s, MKT_E_IO, "read error on the temporary file %s: %s", s->tmp_path[k].c_str(), r < 0 ? strerror(errno) : "short file"); }
        c += r; n -= (size_t)r; off += (uint64_t)r;
    }
    return MKT_OK;
}

// before the first run: the set-up, and the run files (sorted output only)
static int spill_begin(mkt_bam* s) {
    if (s->spilled) return MKT_OK;
    const int rc = bam_setup(s, s->sp_sorted != 0);
    if (rc) return rc;
    for (int k = 0; k < 2 && s->sp_sorted; ++k) {
        s->tmp_fd[k] = open(s->tmp_path[k].c_str(), O_RDWR | O_CREAT | O_TRUNC, 0600);
        if (s->tmp_fd[k] < 0) return bfail(s, MKT_E_IO, "cannot create the temporary file %s: %s", s->tmp_path[k].c_str(), strerror(errno));
        s->tmp_made[k] = true;
    }
    return MKT_OK;
}

// ---- the BGZF stream
static int bs_reserve(mkt_bam* s, uint64_t n) {                  // room for n more bytes after the carry
    BgzfStream& b = s->bs;
    const size_t need = b.carry + n + 64;                          // (the deflate kernel reads up to 15 bytes past a block's end)
    if (need <= b.d_win.bytes()) return MKT_OK;
    size_t ncap = b.d_win.bytes() ? b.d_win.bytes() : ((size_t)1 << 20);
    while (ncap < need) ncap *= 2;
    LedgerBuf<uint8_t> nb;
    const int rc = dev_alloc(s, nb, ncap);
    if (rc) return rc;
    if (b.carry) BCHK(s, hipMemcpyAsync(nb, b.d_win, b.carry, hipMemcpyDeviceToDevice, s->stream));
    BCHK(s, hipStreamSynchronize(s->stream));
    b.d_win = std::move(nb);                                       // (the old window goes here, after the synchronisation)
    return MKT_OK;
}
// n_new bytes have been put after the carry: compress the complete blocks (all of them when final), reduce the window's records
// (w; they start at the carry's end) into the index, queue the compressed bytes for mkt_bam_pull, keep the partial last block
static int bs_commit(mkt_bam* s, uint64_t n_new, bool final, const BaiWin* w) {
    BgzfStream& b = s->bs;
    hipStream_t st = s->stream;
    const uint64_t len = b.carry + n_new;
    const uint64_t nfull = final ? (len + BGZF_RAW - 1) / BGZF_RAW : len / BGZF_RAW;
    const uint64_t nraw = final ? len : nfull * BGZF_RAW;
    const VoffMap vm{b.blk0 * BGZF_RAW + b.carry, b.blk0, b.cbase};
    int rc = dev_grow(s, b.d_csize, (nfull + 2) * sizeof(uint64_t));
    if (rc) return rc;
    uint64_t ctot = 0;
    if (nfull) {
        rc = dev_grow(s, b.d_comp, nfull * (uint64_t)BGZF_STRIDE + 64);
        if (rc) return rc;
        uint64_t cap_b = s->budget / (4 * (uint64_t)BGZF_RAW);       // blocks per deflate launch: the scratch follows the budget
        cap_b = cap_b < 16 ? 16 : (cap_b > 2048 ? 2048 : cap_b);
        const uint64_t batch = nfull < cap_b ? nfull : cap_b;
        if (s->sp_level > 0 && (rc = dev_grow(s, b.d_scratch, deflate_scratch_bytes(batch) + 64))) return rc;
        if ((rc = bgzf_compress(s, b.d_win, nraw, nfull, s->sp_level, b.d_comp, b.d_csize, b.d_scratch, batch, &ctot))) return rc;
    } else BCHK(s, hipMemsetAsync(b.d_csize, 0, 2 * sizeof(uint64_t), st));
    if (w && (rc = bai_window(s, *w, vm, b.d_csize))) return rc;
    if (final && (rc = bai_data_end(s, b.blk0 * BGZF_RAW + len, vm, b.d_csize))) return rc;
    BCHK(s, hipStreamSynchronize(st));
    if (ctot) {
        if ((rc = dev_grow(s, b.d_pack, ctot + 64))) return rc;
        BCHK(s, bgzf_pack(b.d_comp, b.d_csize, nfull, b.d_pack, st));
        if (s->outq_pos == s->outq.size()) { s->outq.clear(); s->outq_pos = 0; }
        const size_t q0 = s->outq.size();
        s->outq.resize(q0 + ctot);
        BCHK(s, hipMemcpyAsync(&s->outq[q0], b.d_pack, ctot, hipMemcpyDeviceToHost, st));
    }
    if (!final) {
        const uint64_t rem = len - nfull * BGZF_RAW;                 // (< one block, from >= one block in: the ranges do not overlap)
        if (nfull && rem) BCHK(s, hipMemcpyAsync(b.d_win, b.d_win + nfull * BGZF_RAW, rem, hipMemcpyDeviceToDevice, st));
        b.carry = rem;
    } else {
        s->outq.append((const char*)kBgzfEof, 28);
        b.carry = 0;
    }
    BCHK(s, hipStreamSynchronize(st));
    b.blk0 += nfull; b.cbase += ctot;
    s->out_total += ctot + (final ? 28 : 0);
    return MKT_OK;
}

// ---- run formation
static int find_nl(mkt_bam* s, uint64_t a, uint64_t b, bool first, uint64_t* pos /* position + 1; 0 = none */) {
    *pos = 0;
    if (a >= b) return MKT_OK;
    if (!s->tb.nl) BCHK(s, s->tb.nl.alloc(s->led, 64));
    hipStream_t st = s->stream;
    BCHK(s, hipMemsetAsync(s->tb.nl, first ? 0xFF : 0, sizeof(unsigned long long), st));
    const uint64_t want = (b - a + 255) / 256;
    const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(k_find_nl, dim3(grid), dim3(256), 0, st, (const uint8_t*)s->d_text, a, b, first ? 1 : 0, s->tb.nl);
    BCHK(s, hipGetLastError());
    unsigned long long v = 0;
    BCHK(s, hipMemcpyAsync(&v, s->tb.nl, sizeof v, hipMemcpyDeviceToHost, st));
    BCHK(s, hipStreamSynchronize(st));
    *pos = (first && v == ~0ull) ? 0 : v;
    return MKT_OK;
}
// text[a, b) (whole lines) -> one run (sorted) or the next piece of the stream (input order)
static int spill_form(mkt_bam* s, uint64_t a, uint64_t b) {
    int rc = spill_begin(s);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = s->stream;
    const bool sorted = s->sp_sorted != 0;
    const uint8_t* text = s->d_text + a;
    PhaseMarks quiet{false};
    BamRecs R;
    if ((rc = bam_records(s, text, b - a, sorted, quiet, &R))) return rc;
    const uint64_t nl = R.nl, total = R.total;
    LedgerBuf<BamIdx> d_idx;
    LedgerBuf<uint8_t> d_raw;                                      // (these three go when the function returns)
    LedgerBuf<SpillRec> d_rec;
    if ((rc = dev_alloc(s, d_idx, (nl + 1) * sizeof(BamIdx)))) return rc;
    if (sorted) {
        if ((rc = dev_alloc(s, d_raw, total + 64)) || (rc = dev_alloc(s, d_rec, (nl + 1) * sizeof(SpillRec)))) return rc;
        bam_write(s, text, R, d_raw, d_idx);
        hipLaunchKernelGGL(k_spill_recs, dim3(R.grid()), dim3(256), 0, st, (const SortRec*)R.rA, (const uint32_t*)R.d_size, (const BamIdx*)d_idx, nl, d_rec);
        BCHK(s, hipGetLastError());
        SpillRun r;
        r.data_off = (uint64_t)lseek(s->tmp_fd[0], 0, SEEK_CUR);
        r.key_off = (uint64_t)lseek(s->tmp_fd[1], 0, SEEK_CUR);
        r.nrec = nl;
        if ((rc = write_dev(s, 0, d_raw, total)) || (rc = write_dev(s, 1, d_rec, nl * sizeof(SpillRec)))) return rc;
        s->runs.push_back(r);
    } else {
        if (!s->spilled) {                                         // the first piece: the header goes first
            if ((rc = bs_reserve(s, s->H.hdr.size()))) return rc;
            BCHK(s, hipMemcpyAsync(s->bs.d_win, s->H.hdr.data(), s->H.hdr.size(), hipMemcpyHostToDevice, st));
            s->bs.carry = s->H.hdr.size();
        }
        if ((rc = bs_reserve(s, total))) return rc;
        bam_write(s, text, R, s->bs.d_win + s->bs.carry, d_idx);
        BCHK(s, hipGetLastError());
        if ((rc = bs_commit(s, total, false, nullptr))) return rc;
    }
    s->spilled = true;
    s->records += nl;
    ++s->nruns;
    s->t_form += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MKT_OK;
}
// cut runs off the front of the resident text: the longest prefix of whole lines within the budget, or one line when the first
// line alone is longer.  final: the text is complete (and ends with a newline).
static int spill_cut(mkt_bam* s, bool final) {
    if (!s->budget || !s->header_done) return MKT_OK;
    for (;;) {
        const uint64_t a = s->tstart, avail = s->len - a;
        if (!avail) break;
        uint64_t end = 0;
        if (final && avail <= s->budget) end = s->len;
        else if (avail < s->budget) break;
        else {
            int rc = find_nl(s, a, a + s->budget, false, &end);
            if (rc) return rc;
            if (!end && (rc = find_nl(s, a + s->budget, s->len, true, &end))) return rc;
            if (!end) break;                                       // (final text ends with a newline: not reached then)
        }
        int rc = spill_form(s, a, end);
        if (rc) return rc;
        s->tstart = end;
    }
    return MKT_OK;
}
static uint64_t auto_budget(mkt_bam* s) {                          // runs for the rest of the input once the text no longer fits
    // (of what is free besides the resident text: a run needs about 1.2 x its text again while it is formed, and the text buffer
    //  of later runs up to 2 x the budget)
    const uint64_t b = device_free(s) / 4;
    return b < ((uint64_t)64 << 10) ? ((uint64_t)64 << 10) : b;
}
// room for n more bytes of text: the unconsumed tail moves to the front of the buffer when that is free; "auto": when the text no
// longer fits, what is resident becomes runs
static int text_room(mkt_bam* s, size_t n) {
    if (s->len + n + 1 <= s->cap) return MKT_OK;
    const uint64_t tail = s->len - s->tstart;
    if (s->tstart && tail <= s->tstart && tail + n + 1 <= s->cap) {
        if (tail) BCHK(s, hipMemcpyAsync(s->d_text, s->d_text + s->tstart, tail, hipMemcpyDeviceToDevice, s->stream));
        BCHK(s, hipStreamSynchronize(s->stream));
        s->len = tail; s->tstart = 0;
        return MKT_OK;
    }
    int rc = bam_reserve(s, tail + n + 1);
    if (rc == MKT_E_NOMEM && s->autob && !s->budget && s->header_done) {
        s->budget = auto_budget(s);
        s->err.clear();
        if ((rc = spill_cut(s, false))) return rc;
        return text_room(s, n);
    }
    return rc;
}

// ---- the merge
static uint64_t merge_window_bytes(const mkt_bam* s) {             // record bytes loaded across all runs at a time
    // (half the budget: a round also holds the gathered window, its compressed blocks and the deflate scratch, all about as large)
    const uint64_t lo = (uint64_t)64 << 10, hi = (uint64_t)1 << 30, w = s->budget / 2;
    return w < lo ? lo : (w > hi ? hi : w);
}
// the merge is set up: the last run is on disk, the text is gone
static int merge_begin(mkt_bam* s) {
    const BamHeader& H = s->H;
    hipStream_t st = s->stream;
    s->cur.assign(s->runs.size(), SpillCur());
    int rc = bai_begin(s);
    if (rc || (rc = bs_reserve(s, H.hdr.size()))) return rc;
    BCHK(s, hipMemcpyAsync(s->bs.d_win, H.hdr.data(), H.hdr.size(), hipMemcpyHostToDevice, st));
    BCHK(s, hipStreamSynchronize(st));
    s->bs.carry = H.hdr.size();
    s->merging = true;
    return MKT_OK;
}
static int merge_finish(mkt_bam* s) {
    const int rc = bai_end(s);
    if (rc) return rc;
    spill_remove(s);
    bam_release_work(s);
    s->merging = false;
    s->done = true;
    if (getenv("MKT_VERBOSE"))
        fprintf(stderr, "[mkt_bam] %-28s %8.2f ms\n", ("merge, " + std::to_string(s->rounds) + " rounds").c_str(), s->t_merge);
    return MKT_OK;
}
// one round: top every run's window up, emit the records that are safe
static int merge_round(mkt_bam* s) {
    const auto t0 = std::chrono::steady_clock::now();
    const size_t R = s->runs.size();
    const uint64_t wb = merge_window_bytes(s) / R + 1;
    int rc;
    for (size_t r = 0; r < R; ++r) {
        const SpillRun& run = s->runs[r];
        SpillCur& c = s->cur[r];
        while (c.next < run.nrec && c.bytes.size() < wb) {
            const uint64_t want = (wb - c.bytes.size()) / 128 + 1;
            const uint64_t k = run.nrec - c.next < want ? run.nrec - c.next : want;
            std::vector<SpillRec> kk(k);
            if ((rc = read_at(s, 1, kk.data(), k * sizeof(SpillRec), run.key_off + c.next * sizeof(SpillRec)))) return rc;
            uint64_t take = 0, bytes = 0;
            while (take < k && (c.keys.empty() && take == 0 ? true : c.bytes.size() + bytes + kk[take].size <= wb)) bytes += kk[take++].size;
            if (!take) break;
            const size_t b0 = c.bytes.size();
            c.bytes.resize(b0 + bytes);
            if ((rc = read_at(s, 0, &c.bytes[b0], bytes, run.data_off + c.data_next))) return rc;
            c.keys.insert(c.keys.end(), kk.begin(), kk.begin() + take);
            c.next += take; c.data_next += bytes;
            if (take < k) break;
        }
    }
    // the bound: the smallest last-loaded record, in T order, of the runs with records still on disk
    bool bounded = false;
    uint64_t bhi = 0;
    size_t brun = 0;
    for (size_t r = 0; r < R; ++r) {
        const SpillCur& c = s->cur[r];
        if (c.next >= s->runs[r].nrec || c.keys.empty()) continue;
        const uint64_t h = c.keys.back().hi;
        if (!bounded || h < bhi) { bounded = true; bhi = h; brun = r; }
    }
    // safe prefixes, concatenated in run order
    std::vector<SpillRec> hrec;
    std::vector<uint64_t> hsrc;
    std::vector<std::pair<size_t, uint64_t>> take;                 // per run: safe records, their bytes (uploaded straight from the run's window)
    uint64_t nb = 0;
    for (size_t r = 0; r < R; ++r) {
        SpillCur& c = s->cur[r];
        size_t cnt = c.keys.size();
        if (bounded) {
            auto le = [&](const SpillRec& k) { return k.hi < bhi || (k.hi == bhi && r <= brun); };
            cnt = (size_t)(std::partition_point(c.keys.begin(), c.keys.end(), le) - c.keys.begin());
        }
        uint64_t rb = 0;
        for (size_t i = 0; i < cnt; ++i) { hsrc.push_back(nb + rb); rb += c.keys[i].size; }
        hrec.insert(hrec.end(), c.keys.begin(), c.keys.begin() + cnt);
        take.emplace_back(cnt, rb);
        nb += rb;
    }
    bool final = true;
    for (size_t r = 0; r < R; ++r) if (s->cur[r].next < s->runs[r].nrec || s->cur[r].keys.size() > take[r].first) final = false;
    const uint64_t n = hrec.size();
    hipStream_t st = s->stream;
    MergeBufs& m = s->mb;
    if (n) {
        if ((rc = dev_grow(s, m.rec, (n + 1) * sizeof(SpillRec))) || (rc = dev_grow(s, m.src, (n + 1) * sizeof(uint64_t))) ||
            (rc = dev_grow(s, m.bytes, nb + 64)) || (rc = dev_grow(s, m.rA, (n + 1) * sizeof(SortRec))) ||
            (rc = dev_grow(s, m.rB, (n + 1) * sizeof(SortRec))) || (rc = dev_grow(s, m.hist, kSortHistBytes)) ||
            (rc = dev_grow(s, m.off, (n + 2) * sizeof(uint64_t))) || (rc = dev_grow(s, m.idx, (n + 1) * sizeof(BamIdx))) ||
            (rc = bs_reserve(s, nb)))
            return rc;
        BCHK(s, hipMemcpyAsync(m.rec, hrec.data(), n * sizeof(SpillRec), hipMemcpyHostToDevice, st));
        BCHK(s, hipMemcpyAsync(m.src, hsrc.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        uint64_t at = 0;
        for (size_t r = 0; r < R; ++r) {
            if (take[r].second) BCHK(s, hipMemcpyAsync(m.bytes + at, s->cur[r].bytes.data(), take[r].second, hipMemcpyHostToDevice, st));
            at += take[r].second;
        }
        BCHK(s, hipStreamSynchronize(st));
        const unsigned grid = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(k_merge_keys, dim3(grid), dim3(256), 0, st, (const SpillRec*)m.rec, n, m.rA);
        SortRec *rA = m.rA, *rB = m.rB;
        sort_radix_passes(rA, rB, n, m.hist, 1, 0, bam_key_bits(s), st);
        hipLaunchKernelGGL(k_merge_sizes, dim3(grid), dim3(256), 0, st, (const SortRec*)rA, (const SpillRec*)m.rec, n, m.off, m.idx);
        BCHK(s, launch_exscan(m.off, n, m.off + n, st));
        hipLaunchKernelGGL(k_merge_gather, dim3((unsigned)((n + MG_WAVES - 1) / MG_WAVES)), dim3(64 * MG_WAVES), 0, st, (const uint8_t*)m.bytes, (const uint64_t*)m.src,
                           (const SortRec*)rA, (const SpillRec*)m.rec, n, (const uint64_t*)m.off, s->bs.d_win + s->bs.carry);
        BCHK(s, hipGetLastError());
    }
    for (size_t r = 0; r < R; ++r) {
        SpillCur& c = s->cur[r];
        c.keys.erase(c.keys.begin(), c.keys.begin() + take[r].first);
        c.bytes.erase(0, take[r].second);
    }
    const BaiWin w{m.idx, m.off, n};
    if ((rc = bs_commit(s, nb, final, &w))) return rc;
    ++s->rounds;
    s->t_merge += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (final) return merge_finish(s);
    return MKT_OK;
}

extern "C" {

int mkt_bam_create(int device, mkt_bam** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_bam* s = new mkt_bam();
    s->device = device;
    if (const char* e = getenv("MKT_BAM_DEVICE_LIMIT")) s->led.limit = (size_t)strtoull(e, nullptr, 10);
    if (hipSetDevice(device) != hipSuccess || s->stream.create(hipStreamNonBlocking) != hipSuccess) { delete s; return MKT_E_HIP; }
    *out = s;
    return MKT_OK;
}
void mkt_bam_destroy(mkt_bam* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    spill_remove(s);
    delete s;                                                       // (the members release: device buffers, pinned memory, events, the stream last)
}
const char* mkt_bam_error(const mkt_bam* s) { return s ? s->err.c_str() : ""; }
const char* mkt_bam_note(const mkt_bam* s) { return s ? s->note.c_str() : ""; }

int mkt_bam_spill(mkt_bam* s, uint64_t run_bytes, const char* tmp_prefix, int sorted, int level) {
    if (!s) return MKT_E_ARG;
    if (s->ran || s->header_done || !s->header.empty() || !s->pending.empty() || s->spill_set) return bfail(s, MKT_E_STATE, "mkt_bam_spill after the first byte");
    if (run_bytes && (!tmp_prefix || !tmp_prefix[0]) && sorted) return bfail(s, MKT_E_ARG, "a run budget needs a temporary-file prefix");
    s->spill_set = true;
    s->autob = run_bytes == MKT_BAM_RUNS_AUTO;
    s->budget = s->autob ? 0 : run_bytes;
    s->sp_sorted = sorted ? 1 : 0;
    s->sp_level = level;
    if (tmp_prefix && tmp_prefix[0]) { s->tmp_path[0] = std::string(tmp_prefix) + ".runs"; s->tmp_path[1] = std::string(tmp_prefix) + ".keys"; }
    return MKT_OK;
}

// The next bytes of the SAM stream (any chunking).  Leading '@' lines are the header; everything from the first other line on
// is alignment text and goes to the device.
static int bam_add_bytes(mkt_bam* s, const char* bytes, size_t n, bool pinned_async) {
    if (s->ran) return bfail(s, MKT_E_STATE, "add after run");
    BCHK(s, hipSetDevice(s->device));
    if (!s->header_done) {
        s->pending.append(bytes, n);
        size_t p = 0;
        for (;;) {
            if (p >= s->pending.size()) break;
            if (s->pending[p] != '@') { s->header_done = true; break; }
            const size_t e = s->pending.find('\n', p);
            if (e == std::string::npos) break;              // an unfinished header line: wait for more
            s->header.append(s->pending, p, e + 1 - p);
            p = e + 1;
        }
        s->pending.erase(0, p);
        if (!s->header_done) return MKT_OK;
        std::string rest;
        rest.swap(s->pending);
        if (rest.empty()) return MKT_OK;
        int rc = text_room(s, rest.size());
        if (rc) return rc;
        BCHK(s, hipMemcpy(s->d_text + s->len, rest.data(), rest.size(), hipMemcpyHostToDevice));
        s->len += rest.size();
        return spill_cut(s, false);
    }
    int rc = text_room(s, n);
    if (rc) return rc;
    if (n) BCHK(s, hipMemcpyAsync(s->d_text + s->len, bytes, n, hipMemcpyHostToDevice, s->stream));
    if (!pinned_async) BCHK(s, hipStreamSynchronize(s->stream));       // the caller may reuse `bytes`
    s->len += n;
    return spill_cut(s, false);
}
int mkt_bam_add(mkt_bam* s, const char* bytes, size_t n) {
    if (!s || (n && !bytes)) return MKT_E_ARG;
    return spill_guard(s, bam_add_bytes(s, bytes, n, false));
}
// room for `bytes` of alignment text, so that the buffer does not grow (and get copied) while the stream comes in
int mkt_bam_reserve(mkt_bam* s, size_t bytes) {
    if (!s) return MKT_E_ARG;
    if (s->ran) return bfail(s, MKT_E_STATE, "reserve after run");
    BCHK(s, hipSetDevice(s->device));
    if (s->budget) {                                               // runs: room for two runs and a window of input at most
        const size_t most = (size_t)s->budget * 2 + kBamIoCap;
        if (bytes > most) bytes = most;
    }
    const int rc = bam_reserve(s, bytes + 1);
    if (rc == MKT_E_NOMEM && s->autob && !s->budget) {            // "auto": the input will not fit -> runs from the start
        s->budget = auto_budget(s);
        s->err.clear();
        return MKT_OK;
    }
    return rc;
}
static int bam_io_slot(mkt_bam* s, int k) {
    if (!s->h_io[k]) {
        BCHK(s, s->h_io[k].alloc(kBamIoCap));
        BCHK(s, s->ev_io.create(k, hipEventDisableTiming));
    }
    if (s->io_busy[k]) { BCHK(s, hipEventSynchronize(s->ev_io[k])); s->io_busy[k] = false; }
    return MKT_OK;
}
// A pinned host buffer for the next bytes of the SAM stream (read a file straight into it), then mkt_bam_commit: the copy to the
// GPU runs while the caller fills the other buffer.
int mkt_bam_window(mkt_bam* s, char** buf, size_t* cap) {
    if (!s || !buf || !cap) return MKT_E_ARG;
    if (s->ran) return bfail(s, MKT_E_STATE, "window after run");
    BCHK(s, hipSetDevice(s->device));
    int rc = bam_io_slot(s, s->io_slot);
    if (rc) return rc;
    *buf = s->h_io[s->io_slot]; *cap = kBamIoCap;
    return MKT_OK;
}
int mkt_bam_commit(mkt_bam* s, size_t n) {
    if (!s || n > kBamIoCap) return MKT_E_ARG;
    const int k = s->io_slot;
    if (!s->h_io[k]) return bfail(s, MKT_E_STATE, "commit without window");
    int rc = bam_add_bytes(s, s->h_io[k], n, true);
    if (rc) return spill_guard(s, rc);
    BCHK(s, hipEventRecord(s->ev_io[k], s->stream));
    s->io_busy[k] = true;
    s->io_slot = k ^ 1;
    return MKT_OK;
}
// alignment lines that are already on the device (no header lines)
int mkt_bam_add_device(mkt_bam* s, const void* d_bytes, size_t n) {
    if (!s || (n && !d_bytes)) return MKT_E_ARG;
    if (s->ran) return bfail(s, MKT_E_STATE, "add after run");
    if (!s->pending.empty()) return bfail(s, MKT_E_STATE, "device text after an unfinished header line");
    s->header_done = true;
    BCHK(s, hipSetDevice(s->device));
    int rc = text_room(s, n);
    if (rc) return spill_guard(s, rc);
    if (n) BCHK(s, hipMemcpyAsync(s->d_text + s->len, d_bytes, n, hipMemcpyDeviceToDevice, s->stream));
    BCHK(s, hipStreamSynchronize(s->stream));
    s->len += n;
    return spill_guard(s, spill_cut(s, false));
}

// the end of the input in out-of-core mode: the last runs; sorted: the merge is set up (mkt_bam_pull drives it), input order:
// the last blocks are queued
static int spill_run_end(mkt_bam* s) {
    int rc = spill_cut(s, true);
    if (rc) return rc;
    s->d_text.reset(); s->cap = s->len = 0; s->tstart = 0;
    if (getenv("MKT_VERBOSE"))
        fprintf(stderr, "[mkt_bam] %-28s %8.2f ms\n", (std::to_string(s->nruns) + (s->sp_sorted ? " runs formed" : " pieces converted")).c_str(), s->t_form);
    if (s->sp_sorted) return merge_begin(s);
    if ((rc = bs_commit(s, 0, true, nullptr))) return rc;
    bam_release_work(s);
    s->done = true;
    return MKT_OK;
}
static int bam_run(mkt_bam* s, int sorted, int level, uint64_t* records, uint64_t* bam_bytes, uint64_t* bai_bytes);
static int bam_single(mkt_bam* s, int sorted, int level, bool verbose);
int mkt_bam_run(mkt_bam* s, int sorted, int level, uint64_t* records, uint64_t* bam_bytes, uint64_t* bai_bytes) {
    if (!s) return MKT_E_ARG;
    return spill_guard(s, bam_run(s, sorted, level, records, bam_bytes, bai_bytes));
}
static int bam_run(mkt_bam* s, int sorted, int level, uint64_t* records, uint64_t* bam_bytes, uint64_t* bai_bytes) {
    if (s->ran) return bfail(s, MKT_E_STATE, "run twice");
    if (s->spill_set && ((sorted != 0) != (s->sp_sorted != 0) || level != s->sp_level)) return bfail(s, MKT_E_ARG, "sorted / level differ from those given to mkt_bam_spill");
    BCHK(s, hipSetDevice(s->device));
    if (records) *records = 0;
    if (bam_bytes) *bam_bytes = 0;
    if (bai_bytes) *bai_bytes = 0;
    s->ran = true;
    if (!s->pending.empty()) {                                     // a last header line without newline, or a file of header lines only
        if (s->pending[0] == '@') { s->header += s->pending; s->header += '\n'; s->pending.clear(); }
    }
    hipStream_t st = s->stream;
    const bool verbose = getenv("MKT_VERBOSE") != nullptr;
    BCHK(s, hipStreamSynchronize(st));                            // (copies of mkt_bam_commit may still be on their way)
    if (s->len > s->tstart) {
        char last = 0;
        BCHK(s, hipMemcpy(&last, s->d_text + s->len - 1, 1, hipMemcpyDeviceToHost));
        if (last != '\n') { const char nl = '\n'; int rc = text_room(s, 1); if (rc) return rc; BCHK(s, hipMemcpy(s->d_text + s->len, &nl, 1, hipMemcpyHostToDevice)); ++s->len; }
    }
    if (s->budget && !s->spilled && s->len > s->budget) {         // ("auto" switched before the header was complete)
        int rc = spill_cut(s, false);
        if (rc) return rc;
    }
    int rc = s->spilled ? MKT_OK : bam_single(s, sorted, level, verbose);
    if (rc == MKT_E_NOMEM && s->autob && s->d_text && s->header_done) {
        // "auto": the single pass does not fit beside the resident text -> that text becomes runs (nothing of the pass is left)
        if (verbose) fprintf(stderr, "[mkt_bam] %s: runs instead\n", s->err.c_str());
        s->err.clear();
        if (!s->budget) s->budget = auto_budget(s);
        rc = spill_cut(s, true);
        if (!rc && !s->spilled) rc = bfail(s, MKT_E_NOMEM, "no run could be formed");
    }
    if (!s->spilled) bam_release_work(s);                           // the single pass has ended: only the BAM stays
    if (rc) return rc;
    if (s->spilled) {
        if ((rc = spill_run_end(s))) return rc;
        if (records) *records = s->records;
        if (bam_bytes) *bam_bytes = s->done ? s->out_total : 0;    // (sorted: known once mkt_bam_pull has handed out the last piece)
        return MKT_OK;
    }
    if (records) *records = s->records;
    if (bam_bytes) *bam_bytes = s->bam_len;
    if (bai_bytes) *bai_bytes = s->bai.size();
    return MKT_OK;
}
// the single pass: everything resident
static int bam_single(mkt_bam* s, int sorted, int level, bool verbose) {
    hipStream_t st = s->stream;
    PhaseMarks mark{verbose};
    int rc = bam_setup(s, sorted != 0);
    if (rc) return rc;
    const uint64_t hdr_len = s->H.hdr.size();
    BamRecs R;
    if ((rc = bam_records(s, s->d_text, s->len, sorted != 0, mark, &R))) return rc;
    const uint64_t nl = R.nl, nraw = hdr_len + R.total;
    if (s->autob) {
        // "auto": does the rest of the pass fit?  Next the records and their index fields beside the text and the sort records; then,
        // with those gone, the compressed blocks, the deflate scratch, the packed BAM and the index's head flags.
        const uint64_t nblk = (nraw + BGZF_RAW - 1) / BGZF_RAW;
        uint64_t batch = ((uint64_t)8 << 30) / deflate_scratch_bytes(1);
        if (batch > nblk) batch = nblk;
        const uint64_t next = nraw + 64 + (nl + 1) * sizeof(BamIdx);
        const uint64_t freed = s->cap + 64 + (nl + 2) * sizeof(uint64_t) + (nl + 1) * (2 * sizeof(SortRec) + sizeof(uint32_t)) + kSortHistBytes;
        const uint64_t later = 2 * nblk * (uint64_t)BGZF_STRIDE + (nblk + 2) * sizeof(uint64_t) + (level > 0 ? deflate_scratch_bytes(batch) : 0) + (nl + 2) * sizeof(uint64_t);
        const uint64_t fr = device_free(s), slack = ((uint64_t)1 << 20) + (next + later) / 20;
        if (next + slack > fr || next + later + slack > fr + freed)
            return bfail(s, MKT_E_NOMEM, "the single pass does not fit this GPU (%.2f GB free beside the text)", (double)fr / 1e9);
    }
    LedgerBuf<uint8_t> d_raw;
    LedgerBuf<BamIdx> d_idx;
    if ((rc = dev_alloc(s, d_raw, nraw + 64))) return rc;
    BCHK(s, hipMemcpyAsync(d_raw, s->H.hdr.data(), hdr_len, hipMemcpyHostToDevice, st));
    if (nl) {
        if ((rc = dev_alloc(s, d_idx, (nl + 1) * sizeof(BamIdx)))) return rc;
        bam_write(s, s->d_text, R, d_raw + hdr_len, d_idx);
        BCHK(s, hipGetLastError());
        BCHK(s, hipStreamSynchronize(st));
        mark("records");
        // the text and the sort records are no longer needed
        R.rA.reset(); R.rB.reset(); R.d_size.reset(); R.d_starts.reset();
    }
    s->d_text.reset(); s->cap = s->len = 0;

    // ---- BGZF: the whole file at once, the packed bytes stay on the device (mkt_bam_fetch / _read)
    const uint64_t nblocks = (nraw + BGZF_RAW - 1) / BGZF_RAW;
    LedgerBuf<uint8_t> d_comp;
    LedgerBuf<uint64_t> d_csize;
    LedgerBuf<uint32_t> d_scratch;
    if ((rc = dev_alloc(s, d_comp, nblocks * (uint64_t)BGZF_STRIDE + 64)) || (rc = dev_alloc(s, d_csize, (nblocks + 2) * sizeof(uint64_t)))) return rc;
    // the token lists and bit streams of the blocks of one launch (levels 1, 2): at most 8 GB of scratch
    uint64_t batch = ((uint64_t)8 << 30) / deflate_scratch_bytes(1);
    if (batch > nblocks) batch = nblocks;
    if (batch < 1) batch = 1;
    if (level > 0 && (rc = dev_alloc(s, d_scratch, deflate_scratch_bytes(batch) + 64))) return rc;
    uint64_t clen = 0;
    if ((rc = bgzf_compress(s, d_raw, nraw, nblocks, level, d_comp, d_csize, d_scratch, batch, &clen))) return rc;
    BCHK(s, hipStreamSynchronize(st));
    mark(level > 0 ? "BGZF deflate" : "BGZF stored");
    d_raw.reset();
    d_scratch.reset();
    { hipError_t e_ = s->d_bam.alloc(s->led, clen + 28 + 64); if (e_ != hipSuccess) return bfail(s, MKT_E_NOMEM, "hipMalloc of the BAM failed: %s", hipGetErrorString(e_)); }
    BCHK(s, bgzf_pack(d_comp, d_csize, nblocks, s->d_bam, st));
    BCHK(s, hipMemcpyAsync(s->d_bam + clen, kBgzfEof, 28, hipMemcpyHostToDevice, st));
    BCHK(s, hipStreamSynchronize(st));
    s->bam_len = clen + 28;
    s->records = nl;
    s->nruns = nl ? 1 : 0;
    d_comp.reset();
    mark("pack");

    // ---- BAI: one window over the whole file (after the compression: the virtual offsets need d_csize)
    s->bai.clear();
    s->note.clear();
    if (sorted) {
        const VoffMap vm{hdr_len, 0, 0};
        if ((rc = bai_begin(s)) || (rc = bai_window(s, BaiWin{d_idx, R.d_off, nl}, vm, d_csize)) || (rc = bai_data_end(s, nraw, vm, d_csize)) || (rc = bai_end(s))) return rc;
        if (s->bx.on) mark("BAI");
    }
    return MKT_OK;
}

int mkt_bam_fetch(mkt_bam* s, int which, uint64_t off, char* out, size_t n) {
    if (!s || (n && !out)) return MKT_E_ARG;
    if (!s->ran) return bfail(s, MKT_E_STATE, "fetch before run");
    if (which == 1) {
        if (off + n > s->bai.size()) return bfail(s, MKT_E_ARG, "range past the end of the index");
        memcpy(out, s->bai.data() + off, n);
        return MKT_OK;
    }
    if (off + n > s->bam_len) return bfail(s, MKT_E_ARG, "range past the end of the BAM");
    BCHK(s, hipSetDevice(s->device));
    if (n) BCHK(s, hipMemcpy(out, s->d_bam + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

// Result bytes [off, off + n) (n <= 64 MiB) through the pinned buffers: *ptr stays valid until the next call but one.
int mkt_bam_read(mkt_bam* s, int which, uint64_t off, size_t n, const char** ptr) {
    if (!s || !ptr) return MKT_E_ARG;
    if (!s->ran) return bfail(s, MKT_E_STATE, "read before run");
    if (which == 1) {
        if (off + n > s->bai.size()) return bfail(s, MKT_E_ARG, "range past the end of the index");
        *ptr = s->bai.data() + off;
        return MKT_OK;
    }
    if (n > kBamIoCap || off + n > s->bam_len) return bfail(s, MKT_E_ARG, "range past the end of the BAM, or longer than 64 MiB");
    BCHK(s, hipSetDevice(s->device));
    const int k = s->io_slot;
    int rc = bam_io_slot(s, k);
    if (rc) return rc;
    if (n) BCHK(s, hipMemcpyAsync(s->h_io[k], s->d_bam + off, n, hipMemcpyDeviceToHost, s->stream));
    BCHK(s, hipStreamSynchronize(s->stream));
    *ptr = s->h_io[k];
    s->io_slot = k ^ 1;
    return MKT_OK;
}


// The BAM in order, at most 64 MiB per call, through the pinned buffers (*ptr valid until the next call but one).  *n = 0: nothing
// more now -- after mkt_bam_run that is the end of the file, and the BAI (mkt_bam_stats, mkt_bam_read / _fetch) is complete.
// Out-of-core mode, sorted: each call drives the merge until a piece is ready; input order: pieces are ready as the input arrives.
int mkt_bam_pull(mkt_bam* s, const char** ptr, size_t* n) {
    if (!s || !ptr || !n) return MKT_E_ARG;
    *ptr = nullptr; *n = 0;
    BCHK(s, hipSetDevice(s->device));
    if (!s->spilled) {
        if (!s->ran) return MKT_OK;
        const uint64_t m = s->bam_len - s->pull_off < kBamIoCap ? s->bam_len - s->pull_off : kBamIoCap;
        if (!m) return MKT_OK;
        const int rc = mkt_bam_read(s, 0, s->pull_off, (size_t)m, ptr);
        if (rc) return rc;
        s->pull_off += m; *n = (size_t)m;
        return MKT_OK;
    }
    while (s->outq_pos == s->outq.size() && s->merging) {
        const int rc = merge_round(s);
        if (rc) return spill_guard(s, rc);
    }
    const size_t avail = s->outq.size() - s->outq_pos;
    if (!avail) return MKT_OK;
    const size_t m = avail < kBamIoCap ? avail : kBamIoCap;
    const int k = s->io_slot;
    const int rc = bam_io_slot(s, k);
    if (rc) return rc;
    memcpy(s->h_io[k], s->outq.data() + s->outq_pos, m);
    s->outq_pos += m;
    if (s->outq_pos == s->outq.size()) { s->outq.clear(); s->outq_pos = 0; }
    s->io_slot = k ^ 1;
    *ptr = s->h_io[k]; *n = m;
    s->pull_off += m;
    return MKT_OK;
}
int mkt_bam_stats(const mkt_bam* s, uint64_t stats[5]) {
    if (!s || !stats) return MKT_E_ARG;
    stats[0] = s->nruns;
    stats[1] = s->tmp_bytes;
    stats[2] = s->led.peak;
    stats[3] = s->spilled ? s->out_total : s->bam_len;
    stats[4] = s->bai.size();
    return MKT_OK;
}

}  // extern "C"
