// mkt_trim.hip -- adapter and quality trimming on the GPU: the driver's `ktrim -k KIT -o PREFIX -1 R1 -2 R2 -c` (microcket:371, 405, 413,
// 430, 444).  Two FASTQ streams -> the interleaved FASTQ of the pairs kept, PREFIX.read1.fq / PREFIX.read2.fq and the counters of
// PREFIX.trim.log, all in input order.  The definition is in include/mkt.h ("adapter and quality trimming") and, executable, in
// tests/ktrimdef.py; DESIGN.md 6j describes the kernels.  One wave per read pair:
//   k_tr_decide  checks the two records, stages the common cycles of both reads in LDS, ballots the cycles that pass in both reads
//                into 64-bit words, finds the last cycle that ends a passing window (every lane looks up the last failing cycle at or
//                before its own: one clz per word), ballots the seed positions, verifies them in ascending order (lanes over the
//                adapter's letters, popcount of the mismatch ballot against the host's limit table), applies the tail rule, and
//                writes the kept length, the class and the two record lengths
//   (scan)       the lengths become offsets (launch_exscan)
//   k_tr_write   writes the two records of the pair to the split streams and to the interleaved one
// Integers only; the atomics count pairs and report the first bad pair, none of them places a byte.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_launch.h"
#include "mkt_sortlib.h"
#include "mkt_trim.h"

using namespace mkt;

namespace mkt {

constexpr int TR_ROW = 512;                                   // bytes of a staged read (>= MKT_TRIM_MAX_READ)
constexpr int TR_WORDS = TR_ROW / 64;
constexpr int TR_WAVES = 4;                                   // pairs per workgroup
static_assert(MKT_TRIM_MAX_READ <= TR_ROW && MKT_TRIM_MAX_ADAPTER <= 64, "a read fits its row, an adapter one wave");
struct TrMeta { uint16_t kept; uint8_t cls, emit; };
struct TrWave { uint8_t r1[TR_ROW], r2[TR_ROW]; };

// line k (0 header, 1 sequence, 2 '+', 3 quality) of record r of a stream
__device__ inline uint64_t tr_line(const uint64_t* starts, uint64_t r, int k, uint32_t* len) {
    const uint64_t a = starts[4 * r + k], d = starts[4 * r + k + 1] - 1 - a;
    *len = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
    return a;
}
__device__ inline int tr_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}
__device__ inline uint32_t tr_record_len(uint32_t hl, uint32_t kept) { return hl + 2u * kept + 5u; }      // header \n seq \n + \n qual \n

__global__ __launch_bounds__(TR_WAVES * 64) void k_tr_decide(const uint8_t* text1, const uint64_t* starts1, const uint8_t* text2, const uint64_t* starts2, uint64_t pair0,
                                                             uint64_t npairs, uint64_t ord0, TrParams P, TrMeta* meta, uint64_t* len1, uint64_t* len2,
                                                             unsigned long long* counts /* dropped, adapter, tailhit, dimer, pass */, unsigned long long* err) {
    __shared__ TrWave sh[TR_WAVES];
    __shared__ uint32_t scnt[5];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    TrWave& W = sh[wv];
    const uint64_t q = (uint64_t)blockIdx.x * TR_WAVES + wv;  // pair of the segment
    const bool have = q < npairs;
    const uint64_t r = pair0 + q;
    if (threadIdx.x < 5) scnt[threadIdx.x] = 0;
    uint32_t hl1 = 0, n1 = 0, pl1 = 0, lq1 = 0, hl2 = 0, n2 = 0, pl2 = 0, lq2 = 0, bad = 0;
    uint64_t h1 = 0, s1 = 0, p1 = 0, q1 = 0, h2 = 0, s2 = 0, p2 = 0, q2 = 0;
    if (have) {
        h1 = tr_line(starts1, r, 0, &hl1); s1 = tr_line(starts1, r, 1, &n1); p1 = tr_line(starts1, r, 2, &pl1); q1 = tr_line(starts1, r, 3, &lq1);
        h2 = tr_line(starts2, r, 0, &hl2); s2 = tr_line(starts2, r, 1, &n2); p2 = tr_line(starts2, r, 2, &pl2); q2 = tr_line(starts2, r, 3, &lq2);
        bad = trim_record_shape(hl1 ? text1[h1] : (uint8_t)0, hl1, pl1 ? text1[p1] : (uint8_t)0, n1, lq1);
        if (!bad) bad = trim_record_shape(hl2 ? text2[h2] : (uint8_t)0, hl2, pl2 ? text2[p2] : (uint8_t)0, n2, lq2);
    }
    const bool live = have && !bad;                           // (the same in every lane of the wave)
    const uint32_t n = n1 < n2 ? n1 : n2;                     // the common length: <= MKT_TRIM_MAX_READ when live
    // ---- stage the common cycles; every quality byte of both reads is checked
    uint32_t badq = 0;
    if (live) {
        for (uint32_t j = lane; j < n; j += 64) { W.r1[j] = text1[s1 + j]; W.r2[j] = text2[s2 + j]; }
        for (uint32_t j = lane; j < n1; j += 64) if (!trim_qual_ok(text1[q1 + j], P.phred)) badq = 1;
        for (uint32_t j = lane; j < n2; j += 64) if (!trim_qual_ok(text2[q2 + j], P.phred)) badq = 1;
    }
    __syncthreads();
    const bool anybadq = __ballot(badq) != 0ull;
    // ---- the cycles that pass in both reads, 64 per word; the last cycle that ends a window of passing cycles
    uint64_t pw[TR_WORDS];
#pragma unroll
    for (int wi = 0; wi < TR_WORDS; ++wi) {
        const uint32_t j = 64u * wi + lane;
        const bool ok = live && j < n && text1[q1 + j] >= P.thr && text2[q2 + j] >= P.thr;
        pw[wi] = __ballot(ok);
    }
    int kept = 0;
    if (live && !anybadq && n >= P.min_size) {
#pragma unroll
        for (int wi = 0; wi < TR_WORDS; ++wi) {
            const int j = 64 * wi + lane;
            const uint64_t own = ~pw[wi] & ((2ull << lane) - 1ull);      // failing cycles of this word at or before this lane's
            int lastbad = -1;
            if (own) lastbad = 64 * wi + 63 - __clzll((long long)own);
            else {
#pragma unroll
                for (int v = wi - 1; v >= 0; --v)
                    if (lastbad < 0 && ~pw[v]) lastbad = 64 * v + 63 - __clzll((long long)~pw[v]);
            }
            if (j < (int)n && j + 1 >= (int)P.min_size && j - lastbad >= (int)P.window && j + 1 > kept) kept = j + 1;
        }
        kept = tr_wave_max(kept);
    }
    // ---- seeds, verified in ascending order; then the tail rule
    uint32_t cls = TR_DROP_QUALITY, dimer = 0;
    if (kept > 0) {                                           // (kept >= min_size >= 10)
        const uint32_t k = (uint32_t)kept;
        int found = -1;
#pragma unroll
        for (int wi = 0; wi < TR_WORDS; ++wi) {
            const uint32_t j = 64u * wi + lane;
            bool sd = false;
            if (j + TR_SEED <= k)
                sd = (W.r1[j] == P.a1[0] && W.r1[j + 1] == P.a1[1] && W.r1[j + 2] == P.a1[2]) || (W.r2[j] == P.a2[0] && W.r2[j + 1] == P.a2[1] && W.r2[j + 2] == P.a2[2]);
            uint64_t m = __ballot(sd);
            while (m && found < 0) {
                const uint32_t p = 64u * wi + (uint32_t)__builtin_ctzll(m);      // p + TR_SEED <= k
                m &= m - 1ull;
                const uint32_t L = k - p < P.alen ? k - p : P.alen;              // <= 64
                const bool in = (uint32_t)lane < L;
                const uint32_t c1 = (uint32_t)__popcll(__ballot(in && W.r1[in ? p + lane : 0] != P.a1[lane]));
                const uint32_t c2 = (uint32_t)__popcll(__ballot(in && W.r2[in ? p + lane : 0] != P.a2[lane]));
                if (c1 <= P.limit[L] && c2 <= P.limit[L]) found = (int)p;
            }
        }
        if (found >= 0) { cls = TR_ADAPTER; kept = found; dimer = (uint32_t)found <= TR_DIMER ? 1u : 0u; }
        else {
            const uint32_t k2 = trim_tail(W.r1, W.r2, k, P.a1, P.a2);
            cls = k2 != k ? (uint32_t)TR_TAILHIT : (uint32_t)TR_PASS;
            kept = (int)k2;
        }
    }
    if (have && lane == 0) {
        uint64_t l1 = 0, l2 = 0;
        TrMeta m = {0, (uint8_t)cls, 0};
        if (bad || anybadq) atomicMin(err, ((unsigned long long)(ord0 + q) << 8) | (bad ? bad : (uint32_t)TR_BAD_QUAL));
        else {
            const bool emit = cls != TR_DROP_QUALITY && (uint32_t)kept >= P.min_size;
            if (cls == TR_ADAPTER) atomicAdd(&scnt[1], 1u);
            if (cls == TR_TAILHIT) atomicAdd(&scnt[2], 1u);
            if (dimer) atomicAdd(&scnt[3], 1u);
            atomicAdd(&scnt[emit ? 4 : 0], 1u);
            if (emit) { m.kept = (uint16_t)kept; m.emit = 1; l1 = tr_record_len(hl1, (uint32_t)kept); l2 = tr_record_len(hl2, (uint32_t)kept); }
        }
        meta[q] = m; len1[q] = l1; len2[q] = l2;
    }
    __syncthreads();
    if (threadIdx.x < 5 && scnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// header \n seq[:k] \n + \n qual[:k] \n to two places
__device__ inline void tr_record(uint8_t* d, uint8_t* e, const uint8_t* h, uint32_t hl, const uint8_t* seq, const uint8_t* qual, uint32_t k, int lane) {
    if (lane == 0) {
        d[hl] = e[hl] = '\n'; d[hl + 1 + k] = e[hl + 1 + k] = '\n'; d[hl + 2 + k] = e[hl + 2 + k] = '+'; d[hl + 3 + k] = e[hl + 3 + k] = '\n';
        d[hl + 4 + 2 * k] = e[hl + 4 + 2 * k] = '\n';
    }
    for (uint32_t j = lane; j < hl; j += 64) d[j] = e[j] = h[j];
    for (uint32_t j = lane; j < k; j += 64) { d[hl + 1 + j] = e[hl + 1 + j] = seq[j]; d[hl + 4 + k + j] = e[hl + 4 + k + j] = qual[j]; }
}
// o1 / o2: exclusive scans of the record lengths (relative to the segment's first byte in each split stream); the interleaved stream
// holds both, so a pair's place in it is o1 + o2.  lim1 / lim2: the scans' totals = the room the host made; a record that would not
// lie inside it is not written and reported (offsets that are not what the host thinks: an error, never a write outside the buffers)
__global__ __launch_bounds__(TR_WAVES * 64) void k_tr_write(const uint8_t* text1, const uint64_t* starts1, const uint8_t* text2, const uint64_t* starts2, uint64_t pair0,
                                                            uint64_t npairs, const TrMeta* meta, const uint64_t* o1, const uint64_t* o2, uint8_t* il, uint8_t* out1, uint8_t* out2,
                                                            uint64_t lim1, uint64_t lim2, unsigned long long* err) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * TR_WAVES + wv;
    if (q >= npairs) return;
    const TrMeta m = meta[q];
    if (!m.emit) return;
    const uint64_t r = pair0 + q;
    const uint32_t k = m.kept;
    uint32_t hl1, n1, hl2, n2, lq1, lq2;
    const uint64_t h1 = tr_line(starts1, r, 0, &hl1), s1 = tr_line(starts1, r, 1, &n1), q1 = tr_line(starts1, r, 3, &lq1);
    const uint64_t h2 = tr_line(starts2, r, 0, &hl2), s2 = tr_line(starts2, r, 1, &n2), q2 = tr_line(starts2, r, 3, &lq2);
    const uint64_t l1 = tr_record_len(hl1, k), l2 = tr_record_len(hl2, k);
    if (o1[q] + l1 > lim1 || o2[q] + l2 > lim2 || k > n1 || k > n2 || k > lq1 || k > lq2 || hl1 > MKT_TRIM_MAX_HEADER || hl2 > MKT_TRIM_MAX_HEADER) {
        if (lane == 0) atomicMin(err, (unsigned long long)q);
        return;
    }
    uint8_t* e = il + o1[q] + o2[q];
    tr_record(out1 + o1[q], e, text1 + h1, hl1, text1 + s1, text1 + q1, k, lane);
    tr_record(out2 + o2[q], e + l1, text2 + h2, hl2, text2 + s2, text2 + q2, k, lane);
}

}  // namespace mkt

struct TrStream {                                             // one FASTQ stream on the device
    mkt::LedgerBuf<uint8_t> text; size_t cap = 0, len = 0;    // the bytes not worked on yet (64 bytes of slack behind cap)
    uint64_t nl = 0;                                          // newlines in them (counted on the way in: when a segment is due)
};
struct mkt_trim {
    int device = 0;
    mkt::DevStream stream;                                   // declared first: destroyed after every buffer
    mkt::DevLedger ledger;
    TrStream in[2];
    mkt::LedgerBuf<uint8_t> out[3]; size_t out_cap[3] = {0, 0, 0}; uint64_t out_len[3] = {0, 0, 0};
    mkt::LedgerBuf<unsigned long long> d_counts;             // dropped, adapter, tailhit, dimer, pass | the first bad pair
    mkt::LedgerBuf<mkt::TrMeta> d_meta; mkt::LedgerBuf<uint64_t> d_lens;      // per pair of a segment (2 length arrays, one total each behind them)
    uint64_t seg_pairs = 1ull << 20;
    bool begun = false, done = false, interleaved = false;
    uint64_t il_line = 0;                                    // interleaved input: lines seen so far (which stream the next byte goes to)
    std::vector<char> split[2];
    mkt::TrParams P;
    uint64_t pairs_done = 0, stats[5] = {0, 0, 0, 0, 0};
    double ms[4] = {0, 0, 0, 0};
    mkt::DevEvents<5> ev;
    std::string err;
};
static int tfail(mkt_trim* s, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (s) s->err = buf;
    return code;
}
#define TCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return tfail((s), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
template <typename T>
static int talloc(mkt_trim* s, mkt::LedgerBuf<T>& b, size_t bytes) {
    const hipError_t e = b.grow(s->ledger, bytes);
    return e == hipSuccess ? MKT_OK : tfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
}
// room for `need` bytes in a byte buffer whose first `keep` bytes stay (nothing queued on it)
static int tgrow_keep(mkt_trim* s, mkt::LedgerBuf<uint8_t>& b, size_t& cap, size_t need, size_t keep, size_t floor_cap) {
    if (need <= cap && b.get()) return MKT_OK;
    size_t ncap = cap ? cap : floor_cap;
    while (ncap < need) ncap *= 2;
    mkt::LedgerBuf<uint8_t> nb;
    hipError_t e = nb.alloc(s->ledger, ncap + 64);
    if (e != hipSuccess) { ncap = need; e = nb.alloc(s->ledger, ncap + 64); }
    if (e != hipSuccess) return tfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", ncap + 64, hipGetErrorString(e));
    if (keep) TCHK(s, hipMemcpy(nb.get(), b.get(), keep, hipMemcpyDeviceToDevice));
    b = std::move(nb);
    cap = ncap;
    return MKT_OK;
}

// Work off the whole pairs that both streams hold (final: everything), seg_pairs at a time; the output of all segments of this call
// follows each other in out[].
static int trim_run(mkt_trim* s, bool final, uint64_t out_bytes[3]) {
    using namespace mkt;
    for (int k = 0; k < 3; ++k) { out_bytes[k] = 0; s->out_len[k] = 0; }
    hipStream_t st = s->stream;
    if (final)      // a missing final newline ends the last line all the same
        for (TrStream& t : s->in) {
            if (!t.len) continue;
            char last = 0;
            TCHK(s, hipMemcpy(&last, t.text + t.len - 1, 1, hipMemcpyDeviceToHost));
            if (last != '\n') {
                if (int rc = tgrow_keep(s, t.text, t.cap, t.len + 1, t.len, (size_t)1 << 20)) return rc;
                const char nlc = '\n';
                TCHK(s, hipMemcpy(t.text + t.len, &nlc, 1, hipMemcpyHostToDevice));
                ++t.len; ++t.nl;
            }
        }
    if (final) {
        const uint64_t done_lines = s->pairs_done * 4;
        for (int k = 0; k < 2; ++k)
            if (s->in[k].nl % 4) return tfail(s, MKT_E_ARG, "%llu lines in stream %d: not whole records (4 lines each)", (unsigned long long)(done_lines + s->in[k].nl), k + 1);
        if (s->in[0].nl != s->in[1].nl)
            return tfail(s, MKT_E_ARG, "%llu read pairs in stream 1, %llu in stream 2", (unsigned long long)(s->pairs_done + s->in[0].nl / 4), (unsigned long long)(s->pairs_done + s->in[1].nl / 4));
    }
    const uint64_t avail = (s->in[0].nl < s->in[1].nl ? s->in[0].nl : s->in[1].nl) / 4;
    const uint64_t todo = final ? avail : avail / s->seg_pairs * s->seg_pairs;
    if (todo == 0) { if (final) s->in[0].len = s->in[1].len = 0; return MKT_OK; }
    TCHK(s, hipEventRecord(s->ev[0], st));
    LineIndex ix[2];
    for (int k = 0; k < 2; ++k) {
        TrStream& t = s->in[k];
        hipError_t e = ix[k].count(t.text, t.len, st);
        if (e == hipErrorOutOfMemory) return tfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed", ix[k].asked);
        TCHK(s, e);
        if (ix[k].nlines != t.nl) return tfail(s, MKT_E_KERNEL, "the line index counts %llu lines, the host %llu", (unsigned long long)ix[k].nlines, (unsigned long long)t.nl);
        e = ix[k].fill(t.text, t.len, st);
        if (e == hipErrorOutOfMemory) return tfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed", ix[k].asked);
        TCHK(s, e);
    }
    const uint8_t *text1 = s->in[0].text, *text2 = s->in[1].text;
    const uint64_t *st1 = ix[0].starts, *st2 = ix[1].starts;
    TCHK(s, hipEventRecord(s->ev[1], st));
    TCHK(s, hipStreamSynchronize(st));
    { float t = 0; TCHK(s, hipEventElapsedTime(&t, s->ev[0], s->ev[1])); s->ms[0] += t; }
    const uint64_t segp = todo < s->seg_pairs ? todo : s->seg_pairs;
    if (int rc = talloc(s, s->d_meta, (size_t)segp * sizeof(TrMeta))) return rc;
    if (int rc = talloc(s, s->d_lens, (size_t)(2 * segp + 2) * sizeof(uint64_t))) return rc;
    uint64_t* L[2] = {s->d_lens.get(), s->d_lens.get() + segp};
    uint64_t* T = s->d_lens.get() + 2 * segp;
    for (uint64_t p0 = 0; p0 < todo; p0 += segp) {
        const uint64_t np = todo - p0 < segp ? todo - p0 : segp;
        const unsigned grid = (unsigned)((np + TR_WAVES - 1) / TR_WAVES);
        TCHK(s, hipMemsetAsync(s->d_counts, 0, 5 * sizeof(unsigned long long), st));
        TCHK(s, hipMemsetAsync(s->d_counts + 5, 0xFF, sizeof(unsigned long long), st));
        TCHK(s, hipEventRecord(s->ev[1], st));
        hipLaunchKernelGGL(k_tr_decide, dim3(grid), dim3(TR_WAVES * 64), 0, st, text1, st1, text2, st2, p0, np, s->pairs_done, s->P, s->d_meta.get(), L[0], L[1],
                           s->d_counts.get(), s->d_counts.get() + 5);
        TCHK(s, hipGetLastError());
        TCHK(s, hipEventRecord(s->ev[2], st));
        for (int k = 0; k < 2; ++k) TCHK(s, launch_exscan(L[k], np, T + k, st));
        unsigned long long hc[6];
        uint64_t tot[2];
        TCHK(s, hipMemcpyAsync(hc, s->d_counts, sizeof hc, hipMemcpyDeviceToHost, st));
        TCHK(s, hipMemcpyAsync(tot, T, sizeof tot, hipMemcpyDeviceToHost, st));
        TCHK(s, hipEventRecord(s->ev[3], st));
        TCHK(s, hipStreamSynchronize(st));
        if (hc[5] != ~0ull) {
            const unsigned code = (unsigned)(hc[5] & 0xFFu);
            return tfail(s, MKT_E_ARG, "read pair %llu (counted from 0): %s", hc[5] >> 8, code < 7 ? kTrBad[code] : "bad");
        }
        if (hc[0] + hc[4] != np) return tfail(s, MKT_E_KERNEL, "%llu pairs decided, %llu counted", (unsigned long long)np, hc[0] + hc[4]);
        const uint64_t grow[3] = {tot[0] + tot[1], tot[0], tot[1]};
        for (int k = 0; k < 3; ++k)
            if (int rc = tgrow_keep(s, s->out[k], s->out_cap[k], s->out_len[k] + grow[k], s->out_len[k], (size_t)1 << 20)) return rc;
        hipLaunchKernelGGL(k_tr_write, dim3(grid), dim3(TR_WAVES * 64), 0, st, text1, st1, text2, st2, p0, np, (const TrMeta*)s->d_meta.get(), (const uint64_t*)L[0],
                           (const uint64_t*)L[1], s->out[0].get() + s->out_len[0], s->out[1].get() + s->out_len[1], s->out[2].get() + s->out_len[2], tot[0], tot[1],
                           s->d_counts.get() + 5);
        TCHK(s, hipGetLastError());
        unsigned long long werr = 0;
        TCHK(s, hipMemcpyAsync(&werr, s->d_counts + 5, sizeof werr, hipMemcpyDeviceToHost, st));
        TCHK(s, hipEventRecord(s->ev[4], st));
        TCHK(s, hipStreamSynchronize(st));
        if (werr != ~0ull) return tfail(s, MKT_E_KERNEL, "the records of pair %llu of the segment do not lie inside the scanned sizes", werr);
        float t = 0;
        TCHK(s, hipEventElapsedTime(&t, s->ev[1], s->ev[2])); s->ms[1] += t;
        TCHK(s, hipEventElapsedTime(&t, s->ev[2], s->ev[3])); s->ms[2] += t;
        TCHK(s, hipEventElapsedTime(&t, s->ev[3], s->ev[4])); s->ms[3] += t;
        for (int k = 0; k < 3; ++k) s->out_len[k] += grow[k];
        for (int k = 0; k < 5; ++k) s->stats[k] += hc[k];
        s->pairs_done += np;
    }
    for (int k = 0; k < 3; ++k) out_bytes[k] = s->out_len[k];
    // what is left of each stream (pairs short of a segment, a record that is not complete yet) moves to the front
    for (int k = 0; k < 2; ++k) {
        TrStream& t = s->in[k];
        uint64_t text_end = t.len;
        if (!final) TCHK(s, hipMemcpy(&text_end, (k ? st2 : st1) + 4 * todo, sizeof text_end, hipMemcpyDeviceToHost));
        const uint64_t rest = t.len - text_end;
        if (rest) {
            LedgerBuf<uint8_t> tmp;
            if (rest <= text_end) TCHK(s, hipMemcpyAsync(t.text, t.text + text_end, rest, hipMemcpyDeviceToDevice, st));      // (no overlap)
            else {
                if (int rc = talloc(s, tmp, rest + 64)) return rc;
                TCHK(s, hipMemcpyAsync(tmp, t.text + text_end, rest, hipMemcpyDeviceToDevice, st));
                TCHK(s, hipMemcpyAsync(t.text, tmp, rest, hipMemcpyDeviceToDevice, st));
            }
            TCHK(s, hipStreamSynchronize(st));
        }
        t.len = rest;
        t.nl -= 4 * todo;
    }
    return MKT_OK;
}

static int trim_append(mkt_trim* s, TrStream& t, const char* bytes, size_t n) {
    if (!n) return MKT_OK;
    if (int rc = tgrow_keep(s, t.text, t.cap, t.len + n + 1, t.len, (size_t)16 << 20)) return rc;
    TCHK(s, hipMemcpyAsync(t.text + t.len, bytes, n, hipMemcpyHostToDevice, s->stream));
    TCHK(s, hipStreamSynchronize(s->stream));
    t.len += n;
    for (const char *p = bytes, *e = bytes + n; (p = (const char*)memchr(p, '\n', (size_t)(e - p))) != nullptr; ++p) ++t.nl;
    return MKT_OK;
}

extern "C" {

void mkt_trim_default_opts(mkt_trim_opts* o) {
    if (!o) return;
    o->adapter1 = o->adapter2 = o->kit = nullptr;
    o->min_size = 36; o->phred = 33; o->min_qual = 20; o->window = 5; o->mismatch = 0.125; o->interleaved_input = 0;
}
int mkt_trim_check(const mkt_trim_opts* o, char* msg, size_t msg_cap) { return mkt::trim_resolve(o, nullptr, msg, msg_cap); }
int mkt_trim_create(int device, mkt_trim** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_trim* s = new mkt_trim();
    s->device = device;
    if (hipSetDevice(device) != hipSuccess || s->stream.create(hipStreamNonBlocking) != hipSuccess || s->ev.create() != hipSuccess ||
        s->d_counts.alloc(s->ledger, 6 * sizeof(unsigned long long)) != hipSuccess) {
        mkt_trim_destroy(s);
        return MKT_E_HIP;
    }
    { const char* e = getenv("MKT_TRIM_SEGMENT_PAIRS"); if (e && atoll(e) > 0) s->seg_pairs = (uint64_t)atoll(e); }
    *out = s;
    return MKT_OK;
}
void mkt_trim_destroy(mkt_trim* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;                                                // the buffers, then the stream
}
const char* mkt_trim_error(const mkt_trim* s) { return s ? s->err.c_str() : ""; }
int mkt_trim_segment_pairs(mkt_trim* s, uint64_t pairs) {
    if (!s) return MKT_E_ARG;
    if (s->begun) return tfail(s, MKT_E_STATE, "the segment size is set before begin");
    if (pairs < 1 || pairs > (1ull << 28)) return tfail(s, MKT_E_ARG, "segment of %llu pairs: need 1 .. 2^28", (unsigned long long)pairs);
    s->seg_pairs = pairs;
    return MKT_OK;
}
int mkt_trim_begin(mkt_trim* s, const mkt_trim_opts* o) {
    if (!s || !o) return MKT_E_ARG;
    char msg[256];
    if (int rc = mkt::trim_resolve(o, &s->P, msg, sizeof msg)) return tfail(s, rc, "%s", msg);
    s->interleaved = o->interleaved_input != 0;
    s->il_line = 0; s->pairs_done = 0;
    for (TrStream& t : s->in) { t.len = 0; t.nl = 0; }
    for (int k = 0; k < 3; ++k) s->out_len[k] = 0;
    for (int k = 0; k < 5; ++k) s->stats[k] = 0;
    for (int k = 0; k < 4; ++k) s->ms[k] = 0;
    s->begun = true; s->done = false;
    return MKT_OK;
}
int mkt_trim_push(mkt_trim* s, const char* bytes1, size_t n1, const char* bytes2, size_t n2, int final, uint64_t out_bytes[3]) {
    if (!s || !out_bytes || (n1 && !bytes1) || (n2 && !bytes2)) return MKT_E_ARG;
    for (int k = 0; k < 3; ++k) out_bytes[k] = 0;
    if (!s->begun) return tfail(s, MKT_E_STATE, "push before begin");
    if (s->done) return tfail(s, MKT_E_STATE, "push after the end of the run");
    TCHK(s, hipSetDevice(s->device));
    if (s->interleaved) {      // lines 0 .. 3 of every 8 go to stream 1, lines 4 .. 7 to stream 2
        if (n2) return tfail(s, MKT_E_ARG, "interleaved input comes in bytes1 alone");
        s->split[0].clear(); s->split[1].clear();
        for (size_t a = 0; a < n1;) {
            const char* nlp = (const char*)memchr(bytes1 + a, '\n', n1 - a);
            const size_t b = nlp ? (size_t)(nlp - bytes1) + 1 : n1;
            std::vector<char>& d = s->split[(s->il_line >> 2) & 1];
            d.insert(d.end(), bytes1 + a, bytes1 + b);
            if (nlp) ++s->il_line;
            a = b;
        }
        for (int k = 0; k < 2; ++k) if (int rc = trim_append(s, s->in[k], s->split[k].data(), s->split[k].size())) return rc;
    } else {
        if (int rc = trim_append(s, s->in[0], bytes1, n1)) return rc;
        if (int rc = trim_append(s, s->in[1], bytes2, n2)) return rc;
    }
    const uint64_t avail = (s->in[0].nl < s->in[1].nl ? s->in[0].nl : s->in[1].nl) / 4;
    if (!final && avail < s->seg_pairs) { for (int k = 0; k < 3; ++k) s->out_len[k] = 0; return MKT_OK; }
    const int rc = trim_run(s, final != 0, out_bytes);
    if (final && rc == MKT_OK) s->done = true;
    return rc;
}
int mkt_trim_fetch(mkt_trim* s, int which, uint64_t off, char* out, size_t n) {
    if (!s || which < 0 || which > 2 || (n && !out)) return MKT_E_ARG;
    if (!s->begun) return tfail(s, MKT_E_STATE, "fetch before begin");
    if (off + n > s->out_len[which]) return tfail(s, MKT_E_ARG, "range past the end of the output");
    TCHK(s, hipSetDevice(s->device));
    if (n) TCHK(s, hipMemcpy(out, s->out[which] + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_trim_stats(const mkt_trim* s, uint64_t* total, uint64_t* dropped, uint64_t* adapter, uint64_t* tailhit, uint64_t* dimer, uint64_t* pass) {
    if (!s) return MKT_E_ARG;
    if (total) *total = s->stats[0] + s->stats[4];
    if (dropped) *dropped = s->stats[0];
    if (adapter) *adapter = s->stats[1];
    if (tailhit) *tailhit = s->stats[2];
    if (dimer) *dimer = s->stats[3];
    if (pass) *pass = s->stats[4];
    return MKT_OK;
}
int mkt_trim_timing(const mkt_trim* s, double* index_ms, double* decide_ms, double* scan_ms, double* write_ms) {
    if (!s) return MKT_E_ARG;
    if (index_ms) *index_ms = s->ms[0];
    if (decide_ms) *decide_ms = s->ms[1];
    if (scan_ms) *scan_ms = s->ms[2];
    if (write_ms) *write_ms = s->ms[3];
    return MKT_OK;
}

}  // extern "C"
