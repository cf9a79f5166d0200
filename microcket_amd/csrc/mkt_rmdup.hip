// mkt_rmdup.hip -- SURVEY.md 8(f) N2: the reference's duplicate removal, krmdup / krmdup.pipe (src/preprocess/krmdup.cpp:88-227), on the GPU.
// Interleaved paired-end FASTQ (8 lines per pair) -> the pairs whose 64-bit key (2 bits per base over seq1[hskip1, epos1)
// and seq2[hskip2, epos2), C=0 A=1 T=2 G=3) was not seen before, in the reference's output order, plus its four counters.
// The newline index is the sorter's (LineIndex, mkt_sortlib.h); "first seen wins" is an open-addressing set of pair ordinals
// that keeps the smaller ordinal.  All device memory sits in the owners of mkt_devbuf.h.  Bit-exact against the compiled
// reference (tests/test_gpu_krmdup.py, golden vectors made by oracle/_ref/krmdup.ref).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_blockscan.h"
#include "mkt_launch.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

struct RmParams { uint32_t hskip1, epos1, hskip2, epos2; };
constexpr uint32_t RM_BATCH = 1u << 16;                      // krmdup.cpp:19

// per pair: its key and its bucket (0 A, 1 C, 2 G, 3 everything else; 4 = discarded).  ord0 = ordinal of the segment's first pair
// in the whole input: keys are kept by ordinal for as long as the run lasts (the hash table below refers to them)
__global__ void k_rm_keys(const uint8_t* text, const uint64_t* starts, uint64_t npairs, RmParams P, uint64_t ord0, uint64_t* keys, uint8_t* bucket /* both by ordinal */) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npairs) return;
    const uint64_t s1 = starts[8 * r + 1], l1 = starts[8 * r + 2] - 1 - s1;      // seq1 without its newline
    const uint64_t s2 = starts[8 * r + 5], l2 = starts[8 * r + 6] - 1 - s2;
    uint64_t okey = 0;
    uint8_t ob = 4;
    uint8_t first = 'N';
    if (l1 >= P.epos1) first = text[s1 + P.hskip1];                              // krmdup.cpp:105-108
    if (first != 'N' && l2 >= P.epos2) {                                         // :110 / :157
        uint64_t key = 0;
        bool bad = false;
        auto code = [&](uint8_t c) -> uint32_t {                                 // :171-176
            if (c == 'A' || c == 'a') return 1u;
            if (c == 'T' || c == 't') return 2u;
            if (c == 'C' || c == 'c') return 0u;
            if (c == 'G' || c == 'g') return 3u;
            bad = true;
            return 0u;
        };
        for (uint32_t i = P.hskip1; i != P.epos1; ++i) key = (key << 2) | code(text[s1 + i]);
        for (uint32_t i = P.hskip2; i != P.epos2; ++i) key = (key << 2) | code(text[s2 + i]);
        if (!bad) { okey = key; ob = first == 'A' ? 0u : (first == 'C' ? 1u : (first == 'G' ? 2u : 3u)); }
    }
    keys[ord0 + r] = okey;
    bucket[ord0 + r] = ob;
}
// The set of keys seen so far (krmdup.cpp:325 keeps one std::unordered_set per bucket; the bucket is a function of the key's first
// base unless that base is lower case or not one of ACGT -- so the set here is over (bucket, key)): an open-addressing table of pair
// ORDINALS, the keys themselves stay in keys[].  A slot is claimed with one compare-and-swap; a pair that finds its own (bucket, key)
// in a slot leaves the SMALLER ordinal there (atomicMin), so "the first one seen wins" whatever order the lanes run in, and pairs of
// earlier segments (smaller ordinals) always win against later ones.  Load <= 1/2: a probe sequence always ends.
constexpr uint32_t RM_EMPTY = 0xFFFFFFFFu;
__device__ inline uint64_t rm_mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }
// what identifies a set member: the key and the bucket (two bits above any 64-bit key's hash input are not available: compare both)
__device__ inline bool rm_same(const uint64_t* keys, const uint8_t* bkt_all, uint32_t o, uint64_t key, uint8_t b) { return keys[o] == key && bkt_all[o] == b; }
constexpr uint32_t RM_MAX_PROBES = 1u << 22;                  // (a probe sequence that long means the table is not what the host thinks: an error, never a hang)
__global__ void k_rm_insert(const uint64_t* keys, const uint8_t* bkt_all, uint64_t ord0, uint64_t npairs, uint32_t* table, uint64_t mask, unsigned long long* err) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= npairs) return;
    const uint32_t me = (uint32_t)(ord0 + r);
    const uint8_t b = bkt_all[me];
    if (b >= 4u) return;
    const uint64_t key = keys[me];
    uint64_t h = rm_mix(key + b) & mask;
    for (uint32_t step = 0; step < RM_MAX_PROBES; ++step) {
        uint32_t cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == RM_EMPTY) {
            cur = atomicCAS(&table[h], RM_EMPTY, me);
            if (cur == RM_EMPTY) return;
        }
        if (rm_same(keys, bkt_all, cur, key, b)) { atomicMin(&table[h], me); return; }
        h = (h + 1) & mask;
    }
    atomicAdd(err, 1ull);
}
// state[pair of the segment]: 0 discarded, 1 duplicate, 2 + bucket kept
__global__ void k_rm_mark(const uint64_t* keys, const uint8_t* bkt_all, uint64_t ord0, uint64_t npairs, const uint32_t* table, uint64_t mask, uint8_t* state,
                          unsigned long long* counts /* uniq, dup, discard */) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t u = 0, d = 0, x = 0;
    if (r < npairs) {
        const uint32_t me = (uint32_t)(ord0 + r);
        const uint8_t b = bkt_all[me];
        if (b >= 4u) { state[r] = 0; x = 1; }
        else {
            const uint64_t key = keys[me];
            uint64_t h = rm_mix(key + b) & mask;
            uint32_t cur = RM_EMPTY;
            for (uint32_t step = 0; step < RM_MAX_PROBES; ++step) {
                cur = table[h];
                if (cur == RM_EMPTY || rm_same(keys, bkt_all, cur, key, b)) break;        // (EMPTY cannot happen: the pair was inserted)
                h = (h + 1) & mask;
                cur = RM_EMPTY;
            }
            if (cur == RM_EMPTY) atomicAdd(&counts[3], 1ull);                               // (reported as an error by the host)
            if (cur == me) { state[r] = (uint8_t)(2u + b); u = 1; } else { state[r] = 1; d = 1; }
        }
    }
    const uint64_t bu = __ballot(u), bd = __ballot(d), bx = __ballot(x);
    if ((threadIdx.x & 63) == 0) {
        if (bu) atomicAdd(&counts[0], (unsigned long long)__popcll(bu));
        if (bd) atomicAdd(&counts[1], (unsigned long long)__popcll(bd));
        if (bx) atomicAdd(&counts[2], (unsigned long long)__popcll(bx));
    }
}
// a bigger table: every ordinal of the old one goes in again (no two of them are the same set member)
__global__ void k_rm_rehash(const uint32_t* old_table, uint64_t old_slots, const uint64_t* keys, const uint8_t* bkt_all, uint32_t* table, uint64_t mask, unsigned long long* err) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= old_slots) return;
    const uint32_t o = old_table[j];
    if (o == RM_EMPTY) return;
    uint64_t h = rm_mix(keys[o] + bkt_all[o]) & mask;
    for (uint32_t step = 0; step < RM_MAX_PROBES; ++step) {
        if (table[h] == RM_EMPTY && atomicCAS(&table[h], RM_EMPTY, o) == RM_EMPTY) return;
        h = (h + 1) & mask;
    }
    atomicAdd(err, 1ull);
}
// output order (krmdup.cpp:215-226): batch after batch of 2^16 input pairs; inside a batch bucket A's survivors, then C's, G's, T's,
// each in input order.  One workgroup per batch: kept pairs per bucket (pass 0), then their slots (pass 1, base[] from the host scan).
__global__ __launch_bounds__(SWG) void k_rm_order(const uint8_t* state, uint64_t npairs, const uint64_t* base /* [nbatch][4], pass 1 */, uint32_t* cnt /* [nbatch][4], pass 0 */,
                                                  uint32_t* order, int pass) {
    __shared__ uint32_t sh[SWG / 64];
    const uint64_t b0 = (uint64_t)blockIdx.x * RM_BATCH, b1 = b0 + RM_BATCH < npairs ? b0 + RM_BATCH : npairs;
    for (uint32_t bucket = 0; bucket < 4u; ++bucket) {
        uint64_t run = pass ? base[(uint64_t)blockIdx.x * 4 + bucket] : 0;
        uint32_t total = 0;
        for (uint64_t r0 = b0; r0 < b1; r0 += SWG) {
            const uint64_t r = r0 + threadIdx.x;
            const uint32_t f = (r < b1 && state[r] == 2u + bucket) ? 1u : 0u;
            uint32_t tot;
            const uint32_t ex = blk_exscan(f, &tot, sh);
            if (pass && f) order[run + ex] = (uint32_t)r;
            run += tot; total += tot;
        }
        if (!pass && threadIdx.x == 0) cnt[(uint64_t)blockIdx.x * 4 + bucket] = total;
    }
}
// record lengths in output order: "id\nseq\n+\nqual\n" = len(id) + len(seq) + len(qual) + 5   (krmdup.cpp:206-209)
__device__ inline uint64_t rm_reclen(const uint64_t* starts, uint64_t r, int mate) {
    const uint64_t l = 8 * r + 4 * (uint64_t)mate;
    return (starts[l + 1] - 1 - starts[l]) + (starts[l + 2] - 1 - starts[l + 1]) + (starts[l + 4] - 1 - starts[l + 3]) + 5u;
}
constexpr uint32_t RPW = 1024;                                // records per workgroup in the gather
// which: 0 read 1, 1 read 2, 2 both interleaved (krmdup.pipe.cpp:197-199)
__global__ __launch_bounds__(SWG) void k_rm_sums(const uint32_t* order, uint64_t nkept, const uint64_t* starts, int which, uint64_t* wsum) {
    __shared__ unsigned long long s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * RPW, e = b + RPW < nkept ? b + RPW : nkept;
    unsigned long long mine = 0;
    for (uint64_t j = b + threadIdx.x; j < e; j += SWG) {
        const uint64_t r = order[j];
        mine += which == 2 ? rm_reclen(starts, r, 0) + rm_reclen(starts, r, 1) : rm_reclen(starts, r, which);
    }
    atomicAdd(&s, mine);
    __syncthreads();
    if (threadIdx.x == 0) wsum[blockIdx.x] = s;
}
__device__ inline void rm_copy_rec(const uint8_t* text, const uint64_t* starts, uint64_t r, int mate, uint8_t* d, int sub, int nsub) {
    const uint64_t l = 8 * r + 4 * (uint64_t)mate;
    const uint64_t a0 = starts[l], a1 = starts[l + 1], a3 = starts[l + 3];
    const uint64_t n0 = starts[l + 1] - a0, n1 = starts[l + 2] - a1, n3 = starts[l + 4] - a3;       // with their newlines
    for (uint64_t k = sub; k < n0; k += nsub) d[k] = text[a0 + k];
    for (uint64_t k = sub; k < n1; k += nsub) d[n0 + k] = text[a1 + k];
    if (sub == 0) { d[n0 + n1] = '+'; d[n0 + n1 + 1] = '\n'; }                                       // the third line becomes a bare "+"
    for (uint64_t k = sub; k < n3; k += nsub) d[n0 + n1 + 2 + k] = text[a3 + k];
}
__global__ __launch_bounds__(SWG) void k_rm_copy(const uint32_t* order, uint64_t nkept, const uint8_t* text, const uint64_t* starts, int which, const uint64_t* woff, uint8_t* out) {
    __shared__ uint32_t sh[SWG / 64];
    __shared__ uint32_t loff[RPW];
    const uint64_t b = (uint64_t)blockIdx.x * RPW, e = b + RPW < nkept ? b + RPW : nkept;
    uint32_t carry = 0;
    for (uint64_t j0 = b; j0 < e; j0 += SWG) {
        const uint64_t j = j0 + threadIdx.x;
        uint32_t len = 0;
        if (j < e) { const uint64_t r = order[j]; len = (uint32_t)(which == 2 ? rm_reclen(starts, r, 0) + rm_reclen(starts, r, 1) : rm_reclen(starts, r, which)); }
        uint32_t tot;
        const uint32_t ex = blk_exscan(len, &tot, sh);
        if (j < e) loff[j - b] = carry + ex;
        carry += tot;
    }
    __syncthreads();
    const uint64_t o0 = woff[blockIdx.x];
    const int sub = threadIdx.x & 31, grp = threadIdx.x >> 5;              // 32 lanes per record
    for (uint64_t j = b + grp; j < e; j += SWG / 32) {
        const uint64_t r = order[j];
        uint8_t* d = out + o0 + loff[j - b];
        if (which == 2) { rm_copy_rec(text, starts, r, 0, d, sub, 32); rm_copy_rec(text, starts, r, 1, d + rm_reclen(starts, r, 0), sub, 32); }
        else rm_copy_rec(text, starts, r, which, d, sub, 32);
    }
}

}  // namespace mkt

struct mkt_rmdup {
    int device = 0;
    mkt::DevStream stream;                                   // declared first: destroyed after every buffer
    mkt::GrowBuf<uint8_t> text; size_t len = 0;              // the FASTQ bytes not worked on yet; cap() counts the 64 bytes of slack
    mkt::GrowBuf<uint8_t> out[3]; uint64_t out_len[3] = {0, 0, 0};
    bool done = false;
    // the run (mkt_rmdup_begin .. the push with final != 0): the input goes through in SEGMENTS of whole 2^16-pair batches
    bool begun = false;
    mkt::RmParams P = {0, 0, 0, 0};
    int interleaved = 0;
    size_t seg_bytes = (size_t)256 << 20;                     // work off what is buffered once it is this much (MKT_RMDUP_SEGMENT_MB)
    uint64_t pairs_done = 0;                                 // ordinal of the next pair
    uint64_t stats[4] = {0, 0, 0, 0};
    mkt::GrowBuf<uint64_t> keys; mkt::GrowBuf<uint8_t> bkt;  // key and bucket of every pair so far, by ordinal (bkt grows last: its cap() is the room)
    mkt::GrowBuf<uint32_t> table;                            // the set: ordinals, open addressing, load <= 1/2; cap() slots
    mkt::DevBuf<unsigned long long> d_err;                   // probe sequences that did not end (none, ever: checked after every segment)
    std::string err;
};
static int rfail(mkt_rmdup* s, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (s) s->err = buf;
    return code;
}
#define RCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return rfail((s), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
static int rnomem(mkt_rmdup* s, size_t bytes, hipError_t e) { return rfail(s, MKT_E_NOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e)); }
template <typename T>
static int ralloc(mkt_rmdup* s, mkt::DevBuf<T>& b, size_t n, size_t pad = 0) {
    const hipError_t e = b.alloc(n, pad);
    return e == hipSuccess ? MKT_OK : rnomem(s, n * sizeof(T) + pad, e);
}

// room for `need` bytes of FASTQ text that wait for their segment.  Growing doubles the buffer -- old and new coexist during the
// copy -- and falls back to just enough when the doubled size does not fit.
static int rmdup_room(mkt_rmdup* s, size_t need) {
    if (s->text.fits(need + 64)) return MKT_OK;
    size_t ncap = s->text.cap() ? s->text.cap() - 64 : ((size_t)256 << 20);
    while (ncap < need) ncap *= 2;
    hipError_t e = s->text.regrow_keep(ncap + 64, s->len);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); e = s->text.regrow_keep(need + ((size_t)64 << 20) + 64, s->len); }
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        size_t fr = 0, tot = 0;
        (void)hipMemGetInfo(&fr, &tot);
        return rfail(s, MKT_E_NOMEM, "no room for %.1f GB of FASTQ text on this GPU (%.1f of %.1f GB free): with mkt_rmdup_push the input is worked off "
                     "in segments; mkt_rmdup_add + mkt_rmdup_run keep all of it", (double)need / 1e9, (double)fr / 1e9, (double)tot / 1e9);
    }
    RCHK(s, e);
    return MKT_OK;
}
// keys / buckets for ordinals < need; the table for that many members at load <= 1/2
static int rmdup_set_room(mkt_rmdup* s, uint64_t need) {
    hipStream_t st = s->stream;
    if (!s->bkt.fits(need)) {
        size_t ncap = s->bkt.cap() ? s->bkt.cap() : ((size_t)1 << 17);      // (small: the growth paths run on every input of a few batches)
        while (ncap < need) ncap *= 2;
        RCHK(s, hipStreamSynchronize(st));
        hipError_t e = s->keys.regrow_keep(ncap, s->pairs_done);
        if (e == hipSuccess) e = s->bkt.regrow_keep(ncap, s->pairs_done);
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return rfail(s, MKT_E_NOMEM, "no room for the keys of %llu read pairs", (unsigned long long)need); }
        RCHK(s, e);
    }
    if (!s->table.fits(need * 2)) {
        uint64_t ns = s->table.cap() ? s->table.cap() : ((uint64_t)1 << 18);
        while (ns < need * 2) ns *= 2;
        mkt::GrowBuf<uint32_t> nt;
        if (nt.regrow(ns) != hipSuccess) { (void)hipGetLastError(); return rfail(s, MKT_E_NOMEM, "no room for a key set of %llu slots", (unsigned long long)ns); }
        RCHK(s, hipMemsetAsync(nt, 0xFF, ns * sizeof(uint32_t), st));
        if (s->table.get()) {
            hipLaunchKernelGGL(mkt::k_rm_rehash, dim3((unsigned)((s->table.cap() + 255) / 256)), dim3(256), 0, st, (const uint32_t*)s->table.get(), (uint64_t)s->table.cap(), (const uint64_t*)s->keys.get(),
                               (const uint8_t*)s->bkt.get(), nt.get(), ns - 1, s->d_err.get());
            RCHK(s, hipGetLastError());
            RCHK(s, hipStreamSynchronize(st));
        }
        s->table = std::move(nt);                            // (the old table goes here, behind the synchronisation)
    }
    return MKT_OK;
}

// Work off what is buffered: every whole 2^16-pair batch (final: everything).  Outputs of the segment -> out[], sizes -> out_bytes.
static int rmdup_segment(mkt_rmdup* s, bool final, uint64_t out_bytes[2]) {
    using namespace mkt;
    out_bytes[0] = out_bytes[1] = 0;
    s->out_len[0] = s->out_len[1] = 0;
    if (s->len == 0) return MKT_OK;
    hipStream_t st = s->stream;
    if (final) {   // getline semantics: a missing final newline ends the last line all the same
        char last = 0;
        RCHK(s, hipMemcpy(&last, s->text + s->len - 1, 1, hipMemcpyDeviceToHost));
        if (last != '\n') { { const int rc = rmdup_room(s, s->len + 2); if (rc) return rc; } const char nlc = '\n'; RCHK(s, hipMemcpy(s->text + s->len, &nlc, 1, hipMemcpyHostToDevice)); ++s->len; }
    }
    const uint64_t n = s->len;
    const uint8_t* text = s->text;
    LineIndex ix;
    { const hipError_t e = ix.count(text, n, st); if (e == hipErrorOutOfMemory) return rnomem(s, ix.asked, e); RCHK(s, e); }
    const uint64_t nl = ix.nlines;
    const uint64_t avail = nl / 8;                           // (a truncated last record is ignored: undefined in the reference)
    const uint64_t npairs = final ? avail : avail / RM_BATCH * RM_BATCH;
    if (npairs == 0) { if (final) s->len = 0; return MKT_OK; }
    if (s->pairs_done + npairs >= (1ull << 32) - 1) return rfail(s, MKT_E_ARG, "%llu pairs: ordinals have 32 bits", (unsigned long long)(s->pairs_done + npairs));
    { const int rc = rmdup_set_room(s, s->pairs_done + npairs); if (rc) return rc; }
    DevBuf<uint8_t> d_state;
    DevBuf<uint32_t> d_bcnt, d_order;
    DevBuf<unsigned long long> d_counts;
    DevBuf<uint64_t> d_base;
    const uint32_t nbatch = (uint32_t)((npairs + RM_BATCH - 1) / RM_BATCH);
    if (int rc = ralloc(s, d_state, npairs, 64)) return rc;
    if (int rc = ralloc(s, d_bcnt, (size_t)nbatch * 4)) return rc;
    if (int rc = ralloc(s, d_base, (size_t)nbatch * 4)) return rc;
    if (int rc = ralloc(s, d_order, npairs + 1)) return rc;
    if (int rc = ralloc(s, d_counts, 8)) return rc;
    RCHK(s, hipMemsetAsync(d_counts, 0, 64, st));
    { const hipError_t e = ix.fill(text, n, st); if (e == hipErrorOutOfMemory) return rnomem(s, ix.asked, e); RCHK(s, e); }
    const uint64_t* d_starts = ix.starts;
    const unsigned pgrid = (unsigned)((npairs + 255) / 256);
    const uint64_t ord0 = s->pairs_done, mask = s->table.cap() - 1;
    hipLaunchKernelGGL(k_rm_keys, dim3(pgrid), dim3(256), 0, st, text, d_starts, npairs, s->P, ord0, s->keys.get(), s->bkt.get());
    hipLaunchKernelGGL(k_rm_insert, dim3(pgrid), dim3(256), 0, st, (const uint64_t*)s->keys.get(), (const uint8_t*)s->bkt.get(), ord0, npairs, s->table.get(), mask, s->d_err.get());
    hipLaunchKernelGGL(k_rm_mark, dim3(pgrid), dim3(256), 0, st, (const uint64_t*)s->keys.get(), (const uint8_t*)s->bkt.get(), ord0, npairs, (const uint32_t*)s->table.get(), mask, d_state.get(), d_counts.get());
    hipLaunchKernelGGL(k_rm_order, dim3(nbatch), dim3(SWG), 0, st, (const uint8_t*)d_state.get(), npairs, (const uint64_t*)d_base.get(), d_bcnt.get(), d_order.get(), 0);
    std::vector<uint32_t> bc((size_t)nbatch * 4);
    unsigned long long hc[4] = {0, 0, 0, 0}, herr = 0;
    uint64_t text_end = 0;
    RCHK(s, hipMemcpyAsync(bc.data(), d_bcnt, bc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RCHK(s, hipMemcpyAsync(hc, d_counts, sizeof hc, hipMemcpyDeviceToHost, st));
    RCHK(s, hipMemcpyAsync(&text_end, d_starts + 8 * npairs, sizeof text_end, hipMemcpyDeviceToHost, st));
    RCHK(s, hipMemcpyAsync(&herr, s->d_err, sizeof herr, hipMemcpyDeviceToHost, st));
    RCHK(s, hipStreamSynchronize(st));
    if (herr | hc[3]) return rfail(s, MKT_E_KERNEL, "the key set's probe sequences did not end (%llu inserts, %llu lookups)", herr, hc[3]);
    std::vector<uint64_t> base(bc.size());
    uint64_t nkept = 0;
    for (size_t k = 0; k < bc.size(); ++k) { base[k] = nkept; nkept += bc[k]; }
    s->stats[1] += hc[0]; s->stats[2] += hc[1]; s->stats[3] += hc[2]; s->stats[0] += hc[0] + hc[1] + hc[2];
    if (nkept != hc[0]) return rfail(s, MKT_E_KERNEL, "kept %llu pairs but counted %llu unique ones", (unsigned long long)nkept, hc[0]);
    DevBuf<uint64_t> d_wsum;
    if (nkept) {
        RCHK(s, hipMemcpyAsync(d_base, base.data(), base.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rm_order, dim3(nbatch), dim3(SWG), 0, st, (const uint8_t*)d_state.get(), npairs, (const uint64_t*)d_base.get(), d_bcnt.get(), d_order.get(), 1);
        const uint32_t wg = (uint32_t)((nkept + RPW - 1) / RPW);
        if (int rc = ralloc(s, d_wsum, (size_t)wg + 2)) return rc;
        for (int which = s->interleaved ? 2 : 0; which < (s->interleaved ? 3 : 2); ++which) {
            hipLaunchKernelGGL(k_rm_sums, dim3(wg), dim3(SWG), 0, st, (const uint32_t*)d_order.get(), nkept, d_starts, which, d_wsum.get());
            RCHK(s, launch_exscan(d_wsum, wg, d_wsum + wg, st));
            uint64_t total = 0;
            RCHK(s, hipMemcpyAsync(&total, d_wsum + wg, sizeof total, hipMemcpyDeviceToHost, st));
            RCHK(s, hipStreamSynchronize(st));
            const int slot = s->interleaved ? 0 : which;
            if (!s->out[slot].fits(total + 64)) {            // (free, then allocate: the old output is not carried)
                const hipError_t e_ = s->out[slot].regrow((size_t)total + total / 8 + 64);
                if (e_ != hipSuccess) return rfail(s, MKT_E_NOMEM, "hipMalloc of the output failed: %s", hipGetErrorString(e_));
            }
            hipLaunchKernelGGL(k_rm_copy, dim3(wg), dim3(SWG), 0, st, (const uint32_t*)d_order.get(), nkept, text, d_starts, which, (const uint64_t*)d_wsum.get(), s->out[slot].get());
            RCHK(s, hipGetLastError());
            RCHK(s, hipStreamSynchronize(st));
            s->out_len[slot] = total;
            out_bytes[slot] = total;
        }
    }
    s->pairs_done += npairs;
    // what is left (pairs of a batch that is not complete yet, a record that is not complete yet) moves to the front
    const uint64_t rest = final ? 0 : n - text_end;
    DevBuf<uint8_t> tmp;
    if (rest) {
        if (rest <= text_end) RCHK(s, hipMemcpyAsync(s->text, text + text_end, rest, hipMemcpyDeviceToDevice, st));      // (no overlap)
        else {
            if (int rc = ralloc(s, tmp, rest, 64)) return rc;
            RCHK(s, hipMemcpyAsync(tmp, text + text_end, rest, hipMemcpyDeviceToDevice, st));
            RCHK(s, hipMemcpyAsync(s->text, tmp, rest, hipMemcpyDeviceToDevice, st));
        }
        RCHK(s, hipStreamSynchronize(st));
    }
    s->len = rest;
    return MKT_OK;
}

extern "C" {

int mkt_rmdup_create(int device, mkt_rmdup** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_rmdup* s = new mkt_rmdup();
    s->device = device;
    if (hipSetDevice(device) != hipSuccess || s->stream.create(hipStreamNonBlocking) != hipSuccess) { mkt_rmdup_destroy(s); return MKT_E_HIP; }
    { const char* e = getenv("MKT_RMDUP_SEGMENT_MB"); if (e && atol(e) > 0) s->seg_bytes = (size_t)atol(e) << 20; }
    if (s->d_err.alloc(1) != hipSuccess || hipMemset(s->d_err, 0, sizeof(unsigned long long)) != hipSuccess) { mkt_rmdup_destroy(s); return MKT_E_HIP; }
    *out = s;
    return MKT_OK;
}
void mkt_rmdup_destroy(mkt_rmdup* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;                                                // the buffers, then the stream
}
const char* mkt_rmdup_error(const mkt_rmdup* s) { return s ? s->err.c_str() : ""; }

int mkt_rmdup_reserve(mkt_rmdup* s, size_t bytes) {
    if (!s) return MKT_E_ARG;
    if (s->done) return rfail(s, MKT_E_STATE, "reserve after the end of the run");
    RCHK(s, hipSetDevice(s->device));
    return rmdup_room(s, bytes + 1);
}
int mkt_rmdup_add(mkt_rmdup* s, const char* bytes, size_t n) {
    if (!s || (n && !bytes)) return MKT_E_ARG;
    if (s->done) return rfail(s, MKT_E_STATE, "add after the end of the run");
    RCHK(s, hipSetDevice(s->device));
    { const int rc = rmdup_room(s, s->len + n + 2); if (rc) return rc; }
    if (n) RCHK(s, hipMemcpyAsync(s->text + s->len, bytes, n, hipMemcpyHostToDevice, s->stream));
    RCHK(s, hipStreamSynchronize(s->stream));
    s->len += n;
    return MKT_OK;
}

/* hskip / keylen as krmdup's -k -K -s -S (krmdup.cpp:229-262).  interleaved != 0: ONE output (read 1 and read 2 records alternating,
 * krmdup.pipe), else two. */
int mkt_rmdup_begin(mkt_rmdup* s, uint32_t hskip1, uint32_t keylen1, uint32_t hskip2, uint32_t keylen2, int interleaved) {
    if (!s) return MKT_E_ARG;
    if (s->begun || s->done) return rfail(s, MKT_E_STATE, "one run per object");
    if (keylen1 + keylen2 > 32 || keylen1 + keylen2 < 16) return rfail(s, MKT_E_ARG, "invalid key sizes (krmdup.cpp:258)");
    s->P.hskip1 = hskip1; s->P.epos1 = hskip1 + keylen1; s->P.hskip2 = hskip2; s->P.epos2 = hskip2 + keylen2;
    s->interleaved = interleaved ? 1 : 0;
    s->begun = true;
    return MKT_OK;
}
/* the next bytes of the stream (may be none).  Whenever a segment's worth is buffered -- and at the end, final != 0 -- the whole
 * 2^16-pair batches in the buffer are worked off: out_bytes = what that left in the outputs (fetch it before the next push), else 0, 0 */
int mkt_rmdup_push(mkt_rmdup* s, const char* bytes, size_t n, int final, uint64_t out_bytes[2]) {
    if (!s || !out_bytes || (n && !bytes)) return MKT_E_ARG;
    out_bytes[0] = out_bytes[1] = 0;
    if (!s->begun) return rfail(s, MKT_E_STATE, "push before begin");
    if (s->done) return rfail(s, MKT_E_STATE, "push after the end of the run");
    if (n) { const int rc = mkt_rmdup_add(s, bytes, n); if (rc) return rc; }
    RCHK(s, hipSetDevice(s->device));
    if (!final && s->len < s->seg_bytes) { s->out_len[0] = s->out_len[1] = 0; return MKT_OK; }
    const int rc = rmdup_segment(s, final != 0, out_bytes);
    if (final && rc == MKT_OK) s->done = true;
    return rc;
}
/* total, uniq, dup, discard so far (krmdup.cpp:377-390) */
int mkt_rmdup_stats(const mkt_rmdup* s, uint64_t stats[4]) {
    if (!s || !stats) return MKT_E_ARG;
    for (int k = 0; k < 4; ++k) stats[k] = s->stats[k];
    return MKT_OK;
}
/* everything added so far as ONE segment (the whole input resident: for inputs that fit; the streaming form is begin / push) */
int mkt_rmdup_run(mkt_rmdup* s, uint32_t hskip1, uint32_t keylen1, uint32_t hskip2, uint32_t keylen2, int interleaved, uint64_t stats[4], uint64_t out_bytes[2]) {
    if (!s || !stats || !out_bytes) return MKT_E_ARG;
    int rc = mkt_rmdup_begin(s, hskip1, keylen1, hskip2, keylen2, interleaved);
    if (rc) return rc;
    RCHK(s, hipSetDevice(s->device));
    rc = rmdup_segment(s, true, out_bytes);
    s->done = true;
    for (int k = 0; k < 4; ++k) stats[k] = s->stats[k];
    return rc;
}

/* output `which` (0: read 1 or the interleaved stream, 1: read 2), bytes [off, off + n) */
int mkt_rmdup_fetch(mkt_rmdup* s, int which, uint64_t off, char* out, size_t n) {
    if (!s || which < 0 || which > 1 || (n && !out)) return MKT_E_ARG;
    if (!s->begun) return rfail(s, MKT_E_STATE, "fetch before run");
    if (off + n > s->out_len[which]) return rfail(s, MKT_E_ARG, "range past the end of the output");
    RCHK(s, hipSetDevice(s->device));
    if (n) RCHK(s, hipMemcpy(out, s->out[which] + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

}  // extern "C"
