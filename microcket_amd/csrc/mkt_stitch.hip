// mkt_stitch.hip -- read stitching on the GPU: the driver's `flash -m 10 -M 150 --interleaved-input -To -c - | deal.flash.pl - PREFIX`
// (microcket:405-408, 430-438).  Interleaved FASTQ -> FLASH's tab lines, PREFIX.ext.fq, PREFIX.cut.read1.fq / .cut.read2.fq and the
// counters of PREFIX.stitch.stat, all in input order.  The definition is in include/mkt.h ("read stitching") and, executable, in
// tests/stitchdef.py; DESIGN.md 6d describes the kernels.  One wave per read pair:
//   k_st_score   stages the pair in LDS (2-bit codes + a called mask in 64-bit words, read 2 reverse-complemented; the qualities as
//                bytes), gives every lane candidate offsets -- mismatches and called positions by XOR + popcount on funnel-shifted
//                words --, reduces to the smallest mismatch density (cross-multiplied integers), breaks ties by the mismatch quality
//                sum, which is computed for tied candidates only, and writes the offset and the four record lengths
//   (scan)       the lengths become offsets (launch_exscan)
//   k_st_write   writes the four records of the pair at their offsets
// Integers only; the atomics count pairs and report the first bad pair, none of them places a byte.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "../../include/mkt.h"
#include "mkt_launch.h"
#include "mkt_sortlib.h"
#include "mkt_stitch.h"

using namespace mkt;

namespace mkt {

constexpr int ST_MAXR = MKT_STITCH_MAX_READ;
constexpr int ST_WORDS = ST_MAXR / 32 + 1;                    // 64-bit words of 32 bases, and one of zeros behind them for the funnel shift
constexpr int ST_WAVES = 4;                                   // pairs per workgroup
constexpr uint32_t ST_NONE = 0xFFFFFFFFu;
enum { ST_BAD_EMPTY = 1, ST_BAD_LONG = 2, ST_BAD_QLEN = 3, ST_BAD_QUAL = 4 };
struct StMeta { int32_t off; uint32_t tlen; };                // chosen offset into read 1 (-1: not combined, -2: bad pair), length of the tag

struct StWave {
    uint64_t a2[ST_WORDS], an[ST_WORDS], b2[ST_WORDS], bn[ST_WORDS];
    uint8_t ca[ST_MAXR], cb[ST_MAXR], qa[ST_MAXR], qb[ST_MAXR];
    uint32_t cand[ST_MAXR];                                   // per candidate: mm << 16 | sl, or ST_NONE
};

__device__ inline uint8_t st_norm(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : (uint8_t)'N';
}
__device__ inline bool st_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r' && c != '\n'); }      // what the program drops at a line's end
__device__ inline uint32_t st_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }      // (normalised)
__device__ inline uint8_t st_comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
// the lines of pair r: 0 header 1, 1 seq 1, 3 qual 1, 4 header 2, 5 seq 2, 7 qual 2
__device__ inline uint64_t st_line(const uint64_t* starts, uint64_t r, int k, uint32_t* len) {
    const uint64_t a = starts[8 * r + k];
    *len = (uint32_t)(starts[8 * r + k + 1] - 1 - a);
    return a;
}
struct StBest { uint32_t num, den, c; };                      // num / den, candidate index (ST_NONE: nothing yet)
__device__ inline bool st_less(const StBest& a, const StBest& b) {
    if (a.c == ST_NONE) return false;
    if (b.c == ST_NONE) return true;
    const uint32_t l = a.num * b.den, r = b.num * a.den;      // < 2^16 * 2^8
    return l < r || (l == r && a.c < b.c);
}
__device__ inline StBest st_wave_min(StBest v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        StBest o;
        o.num = (uint32_t)__shfl_xor((int)v.num, d, 64); o.den = (uint32_t)__shfl_xor((int)v.den, d, 64); o.c = (uint32_t)__shfl_xor((int)v.c, d, 64);
        if (st_less(o, v)) v = o;
    }
    return v;
}
__device__ inline uint32_t st_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
__device__ inline int st_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
__device__ inline uint64_t st_funnel(const uint64_t* w, uint32_t bitpos) {
    const uint32_t k = bitpos >> 6, s = bitpos & 63u;
    return s ? (w[k] >> s) | (w[k + 1] << (64u - s)) : w[k];
}

__global__ __launch_bounds__(ST_WAVES * 64) void k_st_score(const uint8_t* text, const uint64_t* starts, uint64_t pair0, uint64_t npairs, uint64_t ord0, StParams P,
                                                            const uint16_t* thr, StMeta* meta, uint64_t* len_tab, uint64_t* len_ext, uint64_t* len_c1, uint64_t* len_c2,
                                                            unsigned long long* counts /* combined, uncombined, pass */, unsigned long long* err) {
    __shared__ StWave sh[ST_WAVES];
    __shared__ uint32_t scnt[3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    StWave& W = sh[wv];
    const uint64_t q = (uint64_t)blockIdx.x * ST_WAVES + wv;  // pair of the segment
    const bool have = q < npairs;
    const uint64_t r = pair0 + q;
    if (threadIdx.x < 3) scnt[threadIdx.x] = 0;
    uint32_t hl = 0, n1 = 0, n2 = 0, lq1 = 0, lq2 = 0;
    uint64_t h0 = 0, s1 = 0, q1 = 0, s2 = 0, q2 = 0;
    uint32_t bad = 0;
    if (have) {
        h0 = st_line(starts, r, 0, &hl); s1 = st_line(starts, r, 1, &n1); q1 = st_line(starts, r, 3, &lq1);
        s2 = st_line(starts, r, 5, &n2); q2 = st_line(starts, r, 7, &lq2);
        if (n1 == 0 || n2 == 0) bad = ST_BAD_EMPTY;
        else if (n1 > (uint32_t)ST_MAXR || n2 > (uint32_t)ST_MAXR) bad = ST_BAD_LONG;
        else if (n1 != lq1 || n2 != lq2) bad = ST_BAD_QLEN;
    }
    const bool live = have && !bad;                           // (the same in every lane of the wave)
    // ---- stage: codes and qualities, read 2 reverse-complemented
    uint32_t badq = 0;
    if (live) {
        for (uint32_t j = lane; j < n1; j += 64) {
            W.ca[j] = (uint8_t)st_code(st_norm(text[s1 + j]));
            const uint32_t v = (uint32_t)text[q1 + j] - P.phred;      // (wraps for a byte below the offset)
            if (v > 93u) badq = 1;
            W.qa[j] = (uint8_t)v;
        }
        for (uint32_t j = lane; j < n2; j += 64) {
            const uint32_t c = st_code(st_norm(text[s2 + (n2 - 1 - j)]));
            W.cb[j] = (uint8_t)(c < 4u ? 3u - c : 4u);
            const uint32_t v = (uint32_t)text[q2 + (n2 - 1 - j)] - P.phred;
            if (v > 93u) badq = 1;
            W.qb[j] = (uint8_t)v;
        }
    }
    __syncthreads();
    const bool anybadq = __ballot(badq) != 0ull;
    // ---- pack: lanes 0 .. 16 the words of read 1, lanes 32 .. 48 those of read 2
    if (live) {
        const int w = lane & 31;
        if (w < ST_WORDS) {
            const bool second = lane >= 32;
            const uint8_t* c = second ? W.cb : W.ca;
            const uint32_t n = second ? n2 : n1;
            uint64_t bits = 0, mask = 0;
            for (uint32_t b = 0; b < 32u; ++b) {
                const uint32_t j = 32u * (uint32_t)w + b;
                if (j < n && c[j] < 4u) { bits |= (uint64_t)c[j] << (2u * b); mask |= 1ull << (2u * b); }
            }
            (second ? W.b2 : W.a2)[w] = bits;
            (second ? W.bn : W.an)[w] = mask;
        }
    }
    __syncthreads();
    // ---- every candidate's called positions and mismatches
    const uint32_t lim = n1 < n2 ? n1 : n2;
    const uint32_t ncand = (live && !anybadq && lim >= P.m) ? lim - P.m + 1u : 0u;
    const uint32_t imin = n1 > n2 ? n1 - n2 : 0u;
    StBest best = {0u, 1u, ST_NONE};
    for (uint32_t c = lane; c < ncand; c += 64) {
        const uint32_t i = imin + c, L = n1 - i;              // L <= n2
        uint32_t eff = 0, mm = 0;
        for (uint32_t k = 0; 32u * k < L; ++k) {
            const uint32_t rem = L - 32u * k;
            const uint64_t lm = rem >= 32u ? ~0ull : ((1ull << (2u * rem)) - 1ull);
            const uint64_t called = st_funnel(W.an, 2u * i + 64u * k) & W.bn[k] & lm;
            const uint64_t x = st_funnel(W.a2, 2u * i + 64u * k) ^ W.b2[k];
            eff += (uint32_t)__popcll(called);
            mm += (uint32_t)__popcll((x | (x >> 1)) & called);
        }
        if (eff >= P.m) {
            const uint32_t sl = eff < P.M ? eff : P.M;
            W.cand[c] = (mm << 16) | sl;
            const StBest me = {mm, sl, c};
            if (st_less(me, best)) best = me;
        } else W.cand[c] = ST_NONE;
    }
    best = st_wave_min(best);                                 // the smallest density, the first candidate that has it
    bool combined = best.c != ST_NONE && best.num <= (uint32_t)thr[best.den];
    // ---- ties in the density: the smaller mismatch quality sum per scored position wins, then the earlier candidate
    if (combined) {
        uint32_t ties = 0;
        for (uint32_t c = lane; c < ncand; c += 64) {
            const uint32_t v = W.cand[c];
            if (v != ST_NONE && (v >> 16) * best.den == best.num * (v & 0xFFFFu)) ++ties;
        }
        if (st_wave_sum(ties) > 1u) {
            StBest qb = {0u, 1u, ST_NONE};
            for (uint32_t c = lane; c < ncand; c += 64) {
                const uint32_t v = W.cand[c];
                if (v == ST_NONE || (v >> 16) * best.den != best.num * (v & 0xFFFFu)) continue;
                const uint32_t i = imin + c, L = n1 - i;
                uint32_t mq = 0;
                for (uint32_t j = 0; j < L; ++j) {
                    const uint32_t c1 = W.ca[i + j], c2 = W.cb[j];
                    if (c1 < 4u && c2 < 4u && c1 != c2) mq += W.qa[i + j] < W.qb[j] ? W.qa[i + j] : W.qb[j];
                }
                const StBest me = {mq, v & 0xFFFFu, c};       // mq <= 93 * 512 < 2^16
                if (st_less(me, qb)) qb = me;
            }
            best = st_wave_min(qb);
        }
    }
    // ---- the tag: the header without '@' and the white space at its end; a combined pair's is cut at its last '/', an uncombined
    // pair's only loses a closing "/1" or "/2" (`combined` is the same in every lane)
    uint32_t t0 = 0, tlen = 0;
    if (have) {
        t0 = (hl && text[h0] == '@') ? 1u : 0u;
        uint32_t he = hl;
        while (he > t0 && st_space(text[h0 + he - 1])) --he;
        tlen = he - t0;
        if (combined) {
            int last = -1;
            for (uint32_t j = t0 + lane; j < he; j += 64) if (text[h0 + j] == '/') last = (int)j;
            last = st_wave_max(last);
            if (last >= 0) tlen = (uint32_t)last - t0;
        } else if (tlen >= 2u && text[h0 + he - 2] == '/' && (text[h0 + he - 1] == '1' || text[h0 + he - 1] == '2')) tlen -= 2u;
    }
    if (have && lane == 0) {
        uint64_t lt = 0, le = 0, l1 = 0, l2 = 0;
        int32_t off = -2;
        if (bad || anybadq) atomicMin(err, ((unsigned long long)(ord0 + q) << 8) | (bad ? bad : (uint32_t)ST_BAD_QUAL));
        else if (combined) {
            off = (int32_t)(imin + best.c);
            const uint64_t S = (uint64_t)off + n2;
            lt = tlen + 2 * S + 3; le = tlen + 2 * S + 6;
            atomicAdd(&scnt[0], 1u);
        } else {
            off = -1;
            lt = tlen + 2ull * n1 + 2ull * n2 + 5;
            atomicAdd(&scnt[1], 1u);
            if (n1 >= P.min_size + P.cut_tail) {
                l1 = tlen + 2ull * (n1 - P.cut_tail) + 6; l2 = tlen + 2ull * stitch_kept(n2, P.cut_tail) + 6;
                atomicAdd(&scnt[2], 1u);
            }
        }
        meta[q].off = off; meta[q].tlen = tlen;
        len_tab[q] = lt; len_ext[q] = le; len_c1[q] = l1; len_c2[q] = l2;
    }
    __syncthreads();
    if (threadIdx.x < 3 && scnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

__device__ inline void st_copy(uint8_t* d, const uint8_t* s, uint32_t n, int lane, bool norm) {
    for (uint32_t j = lane; j < n; j += 64) d[j] = norm ? st_norm(s[j]) : s[j];
}
// "@tag \n seq[:k] \n + \n qual[:k] \n"
__device__ inline void st_fastq(uint8_t* d, const uint8_t* tag, uint32_t tlen, const uint8_t* seq, const uint8_t* qual, uint32_t k, int lane) {
    if (lane == 0) { d[0] = '@'; d[1 + tlen] = '\n'; d[2 + tlen + k] = '\n'; d[3 + tlen + k] = '+'; d[4 + tlen + k] = '\n'; d[5 + tlen + 2 * k] = '\n'; }
    st_copy(d + 1, tag, tlen, lane, false);
    st_copy(d + 2 + tlen, seq, k, lane, true);
    st_copy(d + 5 + tlen + k, qual, k, lane, false);
}
// offsets: exclusive scans of the lengths (relative to the segment's first byte in each stream).  lim: the scans' totals = the room the
// host made; a record that would not lie inside it is not written and reported (offsets that are not what the host thinks: an error,
// never a write outside the buffers)
struct StTotals { uint64_t tab, ext, c1, c2; };
__global__ __launch_bounds__(ST_WAVES * 64) void k_st_write(const uint8_t* text, const uint64_t* starts, uint64_t pair0, uint64_t npairs, StParams P, const StMeta* meta,
                                                            const uint64_t* o_tab, const uint64_t* o_ext, const uint64_t* o_c1, const uint64_t* o_c2,
                                                            uint8_t* tab, uint8_t* ext, uint8_t* c1, uint8_t* c2, StTotals lim, unsigned long long* err) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * ST_WAVES + wv;
    if (q >= npairs) return;
    const uint64_t r = pair0 + q;
    const int32_t off = meta[q].off;
    if (off < -1) return;
    const uint32_t tlen = meta[q].tlen;
    uint32_t hl, n1, n2, lq;
    const uint64_t h0 = st_line(starts, r, 0, &hl), s1 = st_line(starts, r, 1, &n1), q1 = st_line(starts, r, 3, &lq);
    const uint64_t s2 = st_line(starts, r, 5, &n2), q2 = st_line(starts, r, 7, &lq);
    const uint8_t* tag = text + h0 + ((hl && text[h0] == '@') ? 1 : 0);
    {
        const bool pass = off < 0 && n1 >= P.min_size + P.cut_tail;
        const uint64_t S = (uint64_t)(off < 0 ? 0 : off) + n2;
        const uint64_t lt = off < 0 ? tlen + 2ull * n1 + 2ull * n2 + 5 : tlen + 2 * S + 3, le = off < 0 ? 0 : tlen + 2 * S + 6;
        const uint64_t l1 = pass ? tlen + 2ull * (n1 - P.cut_tail) + 6 : 0, l2 = pass ? tlen + 2ull * stitch_kept(n2, P.cut_tail) + 6 : 0;
        if (o_tab[q] + lt > lim.tab || o_ext[q] + le > lim.ext || o_c1[q] + l1 > lim.c1 || o_c2[q] + l2 > lim.c2 || n1 > (uint32_t)ST_MAXR || n2 > (uint32_t)ST_MAXR ||
            tlen > hl) {
            if (lane == 0) atomicMin(err, (unsigned long long)q);
            return;
        }
    }
    uint8_t* t = tab + o_tab[q];
    st_copy(t, tag, tlen, lane, false);
    if (off < 0) {                                            // tag \t seq1 \t qual1 \t seq2 \t qual2 \n, read 2 as it came in
        if (lane == 0) { t[tlen] = '\t'; t[tlen + 1 + n1] = '\t'; t[tlen + 2 + 2 * n1] = '\t'; t[tlen + 3 + 2 * n1 + n2] = '\t'; t[tlen + 4 + 2 * n1 + 2 * n2] = '\n'; }
        st_copy(t + tlen + 1, text + s1, n1, lane, true);
        st_copy(t + tlen + 2 + n1, text + q1, n1, lane, false);
        st_copy(t + tlen + 3 + 2 * n1, text + s2, n2, lane, true);
        st_copy(t + tlen + 4 + 2 * n1 + n2, text + q2, n2, lane, false);
        if (n1 >= P.min_size + P.cut_tail) {
            st_fastq(c1 + o_c1[q], tag, tlen, text + s1, text + q1, n1 - P.cut_tail, lane);
            st_fastq(c2 + o_c2[q], tag, tlen, text + s2, text + q2, stitch_kept(n2, P.cut_tail), lane);
        }
        return;
    }
    const uint32_t i = (uint32_t)off, S = i + n2;
    uint8_t* e = ext + o_ext[q];
    if (lane == 0) {
        t[tlen] = '\t'; t[tlen + 1 + S] = '\t'; t[tlen + 2 + 2 * S] = '\n';
        e[0] = '@'; e[1 + tlen] = '\n'; e[2 + tlen + S] = '\n'; e[3 + tlen + S] = '+'; e[4 + tlen + S] = '\n'; e[5 + tlen + 2 * S] = '\n';
    }
    st_copy(e + 1, tag, tlen, lane, false);
    for (uint32_t p = lane; p < S; p += 64) {
        uint8_t base, qual;
        if (p < i) { base = st_norm(text[s1 + p]); qual = text[q1 + p]; }
        else {
            const uint32_t j = p - i;                         // position in the reverse-complemented read 2
            const uint8_t b2 = st_comp(st_norm(text[s2 + (n2 - 1 - j)])), p2 = text[q2 + (n2 - 1 - j)];
            if (p >= n1) { base = b2; qual = p2; }
            else {
                const uint8_t b1 = st_norm(text[s1 + p]), p1 = text[q1 + p];
                if (b1 == b2) { base = b1; qual = p1 > p2 ? p1 : p2; }
                else {
                    const uint32_t d = p1 > p2 ? (uint32_t)(p1 - p2) : (uint32_t)(p2 - p1);
                    qual = (uint8_t)((d > 2u ? d : 2u) + P.phred);
                    base = p1 > p2 ? b1 : (p2 > p1 ? b2 : (b2 == 'N' ? b1 : b2));
                }
            }
        }
        t[tlen + 1 + p] = base; t[tlen + 2 + S + p] = qual;
        e[2 + tlen + p] = base; e[5 + tlen + S + p] = qual;
    }
}

}  // namespace mkt

struct mkt_stitch {
    int device = 0;
    mkt::DevStream stream;                                   // declared first: destroyed after every buffer
    mkt::DevLedger ledger;
    mkt::LedgerBuf<uint8_t> text; size_t text_cap = 0, len = 0;      // the FASTQ bytes not worked on yet (64 bytes of slack behind text_cap)
    uint64_t nl_buffered = 0;                                // newlines in them (counted on the way in: when a segment is due)
    mkt::LedgerBuf<uint8_t> out[4]; size_t out_cap[4] = {0, 0, 0, 0}; uint64_t out_len[4] = {0, 0, 0, 0};
    mkt::LedgerBuf<uint16_t> d_thr;
    mkt::LedgerBuf<unsigned long long> d_counts;             // combined, uncombined, pass | the first bad pair
    mkt::LedgerBuf<mkt::StMeta> d_meta; mkt::LedgerBuf<uint64_t> d_lens;      // per pair of a segment (4 length arrays, one total each behind them)
    uint64_t seg_pairs = 1ull << 20;
    bool begun = false, done = false;
    mkt::StParams P = {10, 150, 33, 10, 36, 0.25f};
    uint64_t pairs_done = 0, stats[3] = {0, 0, 0};
    double ms[4] = {0, 0, 0, 0};
    mkt::DevEvents<5> ev;
    std::string err;
};
static int sfail(mkt_stitch* s, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (s) s->err = buf;
    return code;
}
#define SCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return sfail((s), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
template <typename T>
static int salloc(mkt_stitch* s, mkt::LedgerBuf<T>& b, size_t bytes) {
    const hipError_t e = b.grow(s->ledger, bytes);
    return e == hipSuccess ? MKT_OK : sfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
}
// room for `need` bytes in a byte buffer whose first `keep` bytes stay (nothing queued on it)
static int sgrow_keep(mkt_stitch* s, mkt::LedgerBuf<uint8_t>& b, size_t& cap, size_t need, size_t keep, size_t floor_cap) {
    if (need <= cap && b.get()) return MKT_OK;
    size_t ncap = cap ? cap : floor_cap;
    while (ncap < need) ncap *= 2;
    mkt::LedgerBuf<uint8_t> nb;
    hipError_t e = nb.alloc(s->ledger, ncap + 64);
    if (e != hipSuccess) { ncap = need; e = nb.alloc(s->ledger, ncap + 64); }
    if (e != hipSuccess) return sfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", ncap + 64, hipGetErrorString(e));
    if (keep) SCHK(s, hipMemcpy(nb.get(), b.get(), keep, hipMemcpyDeviceToDevice));
    b = std::move(nb);
    cap = ncap;
    return MKT_OK;
}

static const char* const kStBad[] = {"", "an empty read", "a read longer than MKT_STITCH_MAX_READ (512) bases", "sequence and quality differ in length",
                                     "a quality byte outside phred_offset .. phred_offset + 93"};

// Work off the whole pairs that are buffered (final: everything), seg_pairs at a time; the streams of all segments of this call follow
// each other in out[].
static int stitch_run(mkt_stitch* s, bool final, uint64_t out_bytes[4]) {
    using namespace mkt;
    for (int k = 0; k < 4; ++k) { out_bytes[k] = 0; s->out_len[k] = 0; }
    if (s->len == 0) return MKT_OK;
    hipStream_t st = s->stream;
    if (final) {      // a missing final newline ends the last line all the same
        char last = 0;
        SCHK(s, hipMemcpy(&last, s->text + s->len - 1, 1, hipMemcpyDeviceToHost));
        if (last != '\n') {
            if (int rc = sgrow_keep(s, s->text, s->text_cap, s->len + 1, s->len, (size_t)1 << 20)) return rc;
            const char nlc = '\n';
            SCHK(s, hipMemcpy(s->text + s->len, &nlc, 1, hipMemcpyHostToDevice));
            ++s->len; ++s->nl_buffered;
        }
    }
    const uint64_t n = s->len;
    const uint8_t* text = s->text;
    SCHK(s, hipEventRecord(s->ev[0], st));
    LineIndex ix;
    { const hipError_t e = ix.count(text, n, st); if (e == hipErrorOutOfMemory) return sfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed", ix.asked); SCHK(s, e); }
    if (ix.nlines != s->nl_buffered) return sfail(s, MKT_E_KERNEL, "the line index counts %llu lines, the host %llu", (unsigned long long)ix.nlines, (unsigned long long)s->nl_buffered);
    if (final && ix.nlines % 8) return sfail(s, MKT_E_ARG, "%llu lines at the end of the input: not whole read pairs (8 lines each)", (unsigned long long)(s->pairs_done * 8 + ix.nlines));
    const uint64_t avail = ix.nlines / 8;
    const uint64_t todo = final ? avail : avail / s->seg_pairs * s->seg_pairs;
    if (todo == 0) { if (final) s->len = 0; return MKT_OK; }
    { const hipError_t e = ix.fill(text, n, st); if (e == hipErrorOutOfMemory) return sfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed", ix.asked); SCHK(s, e); }
    const uint64_t* d_starts = ix.starts;
    SCHK(s, hipEventRecord(s->ev[1], st));
    SCHK(s, hipStreamSynchronize(st));
    { float t = 0; SCHK(s, hipEventElapsedTime(&t, s->ev[0], s->ev[1])); s->ms[0] += t; }
    const uint64_t segp = todo < s->seg_pairs ? todo : s->seg_pairs;
    if (int rc = salloc(s, s->d_meta, (size_t)segp * sizeof(StMeta))) return rc;
    if (int rc = salloc(s, s->d_lens, (size_t)(4 * segp + 4) * sizeof(uint64_t))) return rc;
    uint64_t* L[4]; uint64_t* T = s->d_lens.get() + 4 * segp;
    for (int k = 0; k < 4; ++k) L[k] = s->d_lens.get() + (size_t)k * segp;
    for (uint64_t p0 = 0; p0 < todo; p0 += segp) {
        const uint64_t np = todo - p0 < segp ? todo - p0 : segp;
        const unsigned grid = (unsigned)((np + ST_WAVES - 1) / ST_WAVES);
        SCHK(s, hipMemsetAsync(s->d_counts, 0, 3 * sizeof(unsigned long long), st));
        SCHK(s, hipMemsetAsync(s->d_counts + 3, 0xFF, sizeof(unsigned long long), st));
        SCHK(s, hipEventRecord(s->ev[1], st));
        hipLaunchKernelGGL(k_st_score, dim3(grid), dim3(ST_WAVES * 64), 0, st, text, d_starts, p0, np, s->pairs_done, s->P, (const uint16_t*)s->d_thr.get(), s->d_meta.get(),
                           L[0], L[1], L[2], L[3], s->d_counts.get(), s->d_counts.get() + 3);
        SCHK(s, hipGetLastError());
        SCHK(s, hipEventRecord(s->ev[2], st));
        for (int k = 0; k < 4; ++k) SCHK(s, launch_exscan(L[k], np, T + k, st));
        unsigned long long hc[4];
        uint64_t tot[4];
        SCHK(s, hipMemcpyAsync(hc, s->d_counts, sizeof hc, hipMemcpyDeviceToHost, st));
        SCHK(s, hipMemcpyAsync(tot, T, sizeof tot, hipMemcpyDeviceToHost, st));
        SCHK(s, hipEventRecord(s->ev[3], st));
        SCHK(s, hipStreamSynchronize(st));
        if (hc[3] != ~0ull) {
            const unsigned code = (unsigned)(hc[3] & 0xFFu);
            return sfail(s, MKT_E_ARG, "read pair %llu (counted from 0): %s", hc[3] >> 8, code < 5 ? kStBad[code] : "bad");
        }
        if (hc[0] + hc[1] != np) return sfail(s, MKT_E_KERNEL, "%llu pairs scored, %llu counted", (unsigned long long)np, hc[0] + hc[1]);
        for (int k = 0; k < 4; ++k)
            if (int rc = sgrow_keep(s, s->out[k], s->out_cap[k], s->out_len[k] + tot[k], s->out_len[k], (size_t)1 << 20)) return rc;
        hipLaunchKernelGGL(k_st_write, dim3(grid), dim3(ST_WAVES * 64), 0, st, text, d_starts, p0, np, s->P, (const StMeta*)s->d_meta.get(), (const uint64_t*)L[0],
                           (const uint64_t*)L[1], (const uint64_t*)L[2], (const uint64_t*)L[3], s->out[0].get() + s->out_len[0], s->out[1].get() + s->out_len[1],
                           s->out[2].get() + s->out_len[2], s->out[3].get() + s->out_len[3], StTotals{tot[0], tot[1], tot[2], tot[3]}, s->d_counts.get() + 3);
        SCHK(s, hipGetLastError());
        unsigned long long werr = 0;
        SCHK(s, hipMemcpyAsync(&werr, s->d_counts + 3, sizeof werr, hipMemcpyDeviceToHost, st));
        SCHK(s, hipEventRecord(s->ev[4], st));
        SCHK(s, hipStreamSynchronize(st));
        if (werr != ~0ull) return sfail(s, MKT_E_KERNEL, "the record of pair %llu of the segment does not lie inside the scanned sizes", werr);
        float t = 0;
        SCHK(s, hipEventElapsedTime(&t, s->ev[1], s->ev[2])); s->ms[1] += t;
        SCHK(s, hipEventElapsedTime(&t, s->ev[2], s->ev[3])); s->ms[2] += t;
        SCHK(s, hipEventElapsedTime(&t, s->ev[3], s->ev[4])); s->ms[3] += t;
        for (int k = 0; k < 4; ++k) s->out_len[k] += tot[k];
        s->stats[0] += hc[0]; s->stats[1] += hc[1]; s->stats[2] += hc[2];
        s->pairs_done += np;
    }
    for (int k = 0; k < 4; ++k) out_bytes[k] = s->out_len[k];
    // what is left (pairs short of a segment, a record that is not complete yet) moves to the front
    uint64_t text_end = n;
    if (!final) SCHK(s, hipMemcpy(&text_end, d_starts + 8 * todo, sizeof text_end, hipMemcpyDeviceToHost));
    const uint64_t rest = n - text_end;
    if (rest) {
        LedgerBuf<uint8_t> tmp;
        if (rest <= text_end) SCHK(s, hipMemcpyAsync(s->text, text + text_end, rest, hipMemcpyDeviceToDevice, st));      // (no overlap)
        else {
            if (int rc = salloc(s, tmp, rest + 64)) return rc;
            SCHK(s, hipMemcpyAsync(tmp, text + text_end, rest, hipMemcpyDeviceToDevice, st));
            SCHK(s, hipMemcpyAsync(s->text, tmp, rest, hipMemcpyDeviceToDevice, st));
        }
        SCHK(s, hipStreamSynchronize(st));
    }
    s->len = rest;
    s->nl_buffered -= 8 * todo;
    return MKT_OK;
}

extern "C" {

int mkt_stitch_check(uint32_t min_overlap, uint32_t max_overlap, double max_mismatch_density, uint32_t phred_offset, uint32_t cut_tail, uint32_t min_size, char* msg, size_t msg_cap) {
    return mkt::stitch_check_args(min_overlap, max_overlap, max_mismatch_density, phred_offset, cut_tail, min_size, msg, msg_cap);
}
int mkt_stitch_create(int device, mkt_stitch** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_stitch* s = new mkt_stitch();
    s->device = device;
    if (hipSetDevice(device) != hipSuccess || s->stream.create(hipStreamNonBlocking) != hipSuccess || s->ev.create() != hipSuccess ||
        s->d_thr.alloc(s->ledger, (MKT_STITCH_MAX_M + 1) * sizeof(uint16_t)) != hipSuccess || s->d_counts.alloc(s->ledger, 4 * sizeof(unsigned long long)) != hipSuccess) {
        mkt_stitch_destroy(s);
        return MKT_E_HIP;
    }
    { const char* e = getenv("MKT_STITCH_SEGMENT_PAIRS"); if (e && atoll(e) > 0) s->seg_pairs = (uint64_t)atoll(e); }
    *out = s;
    return MKT_OK;
}
void mkt_stitch_destroy(mkt_stitch* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;                                                // the buffers, then the stream
}
const char* mkt_stitch_error(const mkt_stitch* s) { return s ? s->err.c_str() : ""; }
int mkt_stitch_segment_pairs(mkt_stitch* s, uint64_t pairs) {
    if (!s) return MKT_E_ARG;
    if (s->begun) return sfail(s, MKT_E_STATE, "the segment size is set before begin");
    if (pairs < 1 || pairs > (1ull << 28)) return sfail(s, MKT_E_ARG, "segment of %llu pairs: need 1 .. 2^28", (unsigned long long)pairs);
    s->seg_pairs = pairs;
    return MKT_OK;
}
int mkt_stitch_begin(mkt_stitch* s, uint32_t min_overlap, uint32_t max_overlap, double max_mismatch_density, uint32_t phred_offset, uint32_t cut_tail, uint32_t min_size) {
    if (!s) return MKT_E_ARG;
    if (s->begun || s->done) return sfail(s, MKT_E_STATE, "one run per object");
    char msg[256];
    if (int rc = mkt::stitch_check_args(min_overlap, max_overlap, max_mismatch_density, phred_offset, cut_tail, min_size, msg, sizeof msg)) return sfail(s, rc, "%s", msg);
    s->P.m = min_overlap; s->P.M = max_overlap; s->P.x = (float)max_mismatch_density; s->P.phred = phred_offset; s->P.cut_tail = cut_tail; s->P.min_size = min_size;
    uint16_t thr[MKT_STITCH_MAX_M + 1];
    mkt::stitch_thresholds(max_overlap, s->P.x, thr);
    SCHK(s, hipSetDevice(s->device));
    SCHK(s, hipMemcpy(s->d_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    s->begun = true;
    return MKT_OK;
}
int mkt_stitch_push(mkt_stitch* s, const char* bytes, size_t n, int final, uint64_t out_bytes[4]) {
    if (!s || !out_bytes || (n && !bytes)) return MKT_E_ARG;
    for (int k = 0; k < 4; ++k) out_bytes[k] = 0;
    if (!s->begun) return sfail(s, MKT_E_STATE, "push before begin");
    if (s->done) return sfail(s, MKT_E_STATE, "push after the end of the run");
    SCHK(s, hipSetDevice(s->device));
    if (n) {
        if (int rc = sgrow_keep(s, s->text, s->text_cap, s->len + n + 1, s->len, (size_t)16 << 20)) return rc;
        SCHK(s, hipMemcpyAsync(s->text + s->len, bytes, n, hipMemcpyHostToDevice, s->stream));
        SCHK(s, hipStreamSynchronize(s->stream));
        s->len += n;
        for (const char *p = bytes, *e = bytes + n; (p = (const char*)memchr(p, '\n', (size_t)(e - p))) != nullptr; ++p) ++s->nl_buffered;
    }
    if (!final && s->nl_buffered / 8 < s->seg_pairs) { for (int k = 0; k < 4; ++k) s->out_len[k] = 0; return MKT_OK; }
    const int rc = stitch_run(s, final != 0, out_bytes);
    if (final && rc == MKT_OK) s->done = true;
    return rc;
}
int mkt_stitch_fetch(mkt_stitch* s, int which, uint64_t off, char* out, size_t n) {
    if (!s || which < 0 || which > 3 || (n && !out)) return MKT_E_ARG;
    if (!s->begun) return sfail(s, MKT_E_STATE, "fetch before begin");
    if (off + n > s->out_len[which]) return sfail(s, MKT_E_ARG, "range past the end of the output");
    SCHK(s, hipSetDevice(s->device));
    if (n) SCHK(s, hipMemcpy(out, s->out[which] + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_stitch_stats(const mkt_stitch* s, uint64_t* total, uint64_t* combined, uint64_t* uncombined, uint64_t* pass) {
    if (!s) return MKT_E_ARG;
    if (total) *total = s->stats[0] + s->stats[1];
    if (combined) *combined = s->stats[0];
    if (uncombined) *uncombined = s->stats[1];
    if (pass) *pass = s->stats[2];
    return MKT_OK;
}
int mkt_stitch_timing(const mkt_stitch* s, double* index_ms, double* score_ms, double* scan_ms, double* write_ms) {
    if (!s) return MKT_E_ARG;
    if (index_ms) *index_ms = s->ms[0];
    if (score_ms) *score_ms = s->ms[1];
    if (scan_ms) *scan_ms = s->ms[2];
    if (write_ms) *write_ms = s->ms[3];
    return MKT_OK;
}

}  // extern "C"
