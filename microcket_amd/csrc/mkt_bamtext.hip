// mkt_bamtext.hip -- BAM records to SAM text on the GPU: what `samtools view [-h | -H]` prints for the inflated stream of a BAM, and the
// reader object of include/mkt.h (mkt_bamtext_*).  DESIGN.md 6i has the record index, the carry, the float route and the bounds;
// mkt_bamtext.h the functions that decide what is accepted and write the line (shared with tests/host/bamtext_host.cpp).
//
// One run: [carry of the run before | the pieces added since] lies in one device buffer.  The record region is cut into segments; a
// workgroup per segment guesses the first record start in it and walks the chain (k_bt_guess); one lane puts the segments in order and
// walks again where a guess was wrong (k_bt_resolve); the counts are scanned and the record offsets filled; a thread per record
// validates it and measures its line (k_bt_len); the lengths are scanned (k_bt_sums, k_bt_bases); eight lanes per record write the
// line (k_bt_emit).  No atomics: every array is the same on every call.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_devbuf.h"
#include "mkt_blockscan.h"
#include "mkt_bamtext.h"

using namespace mkt;

namespace mkt {

constexpr uint32_t kBtGroup = 8;                         // lanes that write one line
constexpr uint32_t kBtPerWg = SWG / kBtGroup;

struct BtSums { uint64_t text_bytes, floats, float_records, first_bad; uint32_t reason, pad; };

// exclusive scan over one workgroup of values below 2^44 (two scans of 32-bit halves that cannot overflow)
__device__ inline uint64_t blk_exscan64(uint64_t v, uint64_t* total, uint32_t* sh) {
    uint32_t th, tl;
    const uint32_t eh = blk_exscan((uint32_t)(v >> 20), &th, sh), el = blk_exscan((uint32_t)(v & 0xFFFFFu), &tl, sh);
    *total = ((uint64_t)th << 20) + tl;
    return ((uint64_t)eh << 20) + el;
}

// Segment k is [start + k S, start + (k + 1) S).  Segment 0 begins at `start`, which is a record start; every other workgroup takes the
// lowest offset of its segment that passes bt_plausible, 256 candidates a round, and lane 0 walks the chain from it.
__global__ __launch_bounds__(SWG) void k_bt_guess(const uint8_t* __restrict__ s, uint64_t n, uint64_t start, uint64_t seg_bytes, int32_t n_ref, uint32_t max_record, BtSeg* __restrict__ seg) {
    __shared__ uint32_t sh[SWG / 64];
    const uint64_t k = blockIdx.x, lo = start + k * seg_bytes, hi = lo + seg_bytes;
    uint64_t entry = k ? kBtNone : start;
    for (uint64_t base = 0; k && base < seg_bytes && lo + base < n; base += SWG) {      // (the same turns for every thread)
        const uint64_t c = lo + base + threadIdx.x;
        const bool ok = c < hi && c < n && bt_plausible(s, n, c, n_ref, max_record);
        const uint64_t m = __ballot(ok);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m ? (uint32_t)(__ffsll((unsigned long long)m) - 1) : 64u;
        __syncthreads();
        uint32_t first = SWG;
        for (int w = SWG / 64 - 1; w >= 0; --w) if (sh[w] < 64u) first = (uint32_t)w * 64u + sh[w];
        __syncthreads();
        if (first < (uint32_t)SWG) { entry = lo + base + first; break; }
    }
    if (threadIdx.x == 0) {
        BtSeg g;
        if (entry != kBtNone && entry < n) g = bt_walk(s, n, entry, hi, max_record);
        else { g.entry = entry; g.exit = entry; g.count = 0; g.status = entry == kBtNone ? 0u : 1u; }
        seg[k] = g;
    }
}
__global__ void k_bt_resolve(const uint8_t* __restrict__ s, uint64_t n, uint64_t start, uint64_t seg_bytes, uint64_t nseg, uint32_t max_record, BtSeg* __restrict__ seg, BtIndex* __restrict__ X) {
    if (blockIdx.x == 0 && threadIdx.x == 0) bt_resolve(s, n, start, seg_bytes, nseg, max_record, seg, X);
}
// exclusive sums of the counts of the segments: base[0 .. nseg]
__global__ __launch_bounds__(SWG) void k_bt_scan_counts(const BtSeg* __restrict__ seg, uint64_t nseg, uint64_t* __restrict__ base) {
    __shared__ uint32_t sh[SWG / 64];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nseg; b += SWG) {
        const uint64_t i = b + threadIdx.x;
        uint32_t tot;
        const uint32_t ex = blk_exscan(i < nseg ? seg[i].count : 0u, &tot, sh);
        if (i < nseg) base[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) base[nseg] = carry;
}
// the record offsets of one segment: the walk of the resolve step again, bounded by its count
__global__ __launch_bounds__(SWG) void k_bt_fill(const uint8_t* __restrict__ s, const BtSeg* __restrict__ seg, uint64_t nseg, const uint64_t* __restrict__ base, uint64_t nrec, uint64_t* __restrict__ rec_off) {
    const uint64_t k = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (k >= nseg) return;
    const BtSeg g = seg[k];
    uint64_t off = g.entry, at = base[k];
    for (uint32_t i = 0; i < g.count && at < nrec; ++i, ++at) {      // (every record counted lies below n: bt_walk)
        rec_off[at] = off;
        off += 4ull + bt_u32(s, off);
    }
}
__global__ __launch_bounds__(SWG) void k_bt_len(const uint8_t* __restrict__ s, uint64_t nrec, const uint64_t* __restrict__ rec_off, BtRefs R, BtFloats F, const uint64_t* __restrict__ fblk,
                                                const uint32_t* __restrict__ foff, uint32_t* __restrict__ len, uint32_t* __restrict__ seq_at, uint32_t* __restrict__ nf, uint32_t* __restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (i >= nrec) return;
    BtLine L;
    const uint32_t r = bt_record_len(s, rec_off[i], R, F, F.len ? fblk[blockIdx.x] + foff[i] : 0ull, &L);
    len[i] = (uint32_t)L.len;                            // below 2^32: at most five characters for every byte of a record of at most 16 MiB
    seq_at[i] = L.seq_at; nf[i] = L.floats; st[i] = r;
}
// per block of SWG records: where each line begins in the block's text, its first float in the block's floats, and the block's sums
__global__ __launch_bounds__(SWG) void k_bt_sums(uint64_t nrec, const uint32_t* __restrict__ len, const uint32_t* __restrict__ nf, const uint32_t* __restrict__ st, uint64_t* __restrict__ line_off,
                                                 uint32_t* __restrict__ foff, uint64_t* __restrict__ blk_len, uint32_t* __restrict__ blk_nf, uint32_t* __restrict__ blk_frec, uint32_t* __restrict__ blk_bad) {
    __shared__ uint32_t sh[SWG / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    const bool in = i < nrec;
    const uint32_t f = in ? nf[i] : 0u, bad = in && st[i] ? 1u : 0u;
    uint64_t tl;
    uint32_t tf, tr, tb;
    const uint64_t el = blk_exscan64(in ? len[i] : 0u, &tl, sh);
    const uint32_t ef = blk_exscan(f, &tf, sh);           // a record holds fewer than 2^22 floats
    (void)blk_exscan(f ? 1u : 0u, &tr, sh);
    const uint32_t eb = blk_exscan(bad, &tb, sh);
    if (in) { line_off[i] = el; foff[i] = ef; }
    if (bad && eb == 0) blk_bad[blockIdx.x] = threadIdx.x;
    if (threadIdx.x == 0) { blk_len[blockIdx.x] = tl; blk_nf[blockIdx.x] = tf; blk_frec[blockIdx.x] = tr; if (!tb) blk_bad[blockIdx.x] = 0xFFFFFFFFu; }
}
__global__ __launch_bounds__(SWG) void k_bt_bases(uint64_t nblk, const uint64_t* __restrict__ blk_len, const uint32_t* __restrict__ blk_nf, const uint32_t* __restrict__ blk_frec, const uint32_t* __restrict__ blk_bad,
                                                  const uint32_t* __restrict__ st, uint64_t* __restrict__ tbase, uint64_t* __restrict__ fbase, BtSums* __restrict__ S) {
    __shared__ uint32_t sh[SWG / 64];
    __shared__ uint64_t first_bad;
    if (threadIdx.x == 0) first_bad = kBtNone;
    __syncthreads();
    uint64_t cl = 0, cf = 0, cr = 0;
    for (uint64_t b = 0; b < nblk; b += SWG) {
        const uint64_t i = b + threadIdx.x;
        uint64_t tl, tf;
        uint32_t tr, tb;
        const uint64_t el = blk_exscan64(i < nblk ? blk_len[i] : 0ull, &tl, sh), ef = blk_exscan64(i < nblk ? blk_nf[i] : 0ull, &tf, sh);
        (void)blk_exscan(i < nblk ? blk_frec[i] : 0u, &tr, sh);
        const bool bad = i < nblk && blk_bad[i] != 0xFFFFFFFFu;
        const uint32_t eb = blk_exscan(bad ? 1u : 0u, &tb, sh);
        if (i < nblk) { tbase[i] = cl + el; fbase[i] = cf + ef; }
        if (bad && eb == 0 && first_bad == kBtNone) first_bad = i * SWG + blk_bad[i];      // (one thread per turn; read back after the barriers of the next scan or below)
        cl += tl; cf += tf; cr += tr;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tbase[nblk] = cl; fbase[nblk] = cf;
        S->text_bytes = cl; S->floats = cf; S->float_records = cr; S->first_bad = first_bad;
        S->reason = first_bad != kBtNone ? st[first_bad] : 0u; S->pad = 0;
    }
}
__global__ __launch_bounds__(SWG) void k_bt_floats(const uint8_t* __restrict__ s, uint64_t nrec, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ nf, const uint64_t* __restrict__ fblk,
                                                   const uint32_t* __restrict__ foff, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (i < nrec && nf[i]) bt_record_floats(s, rec_off[i], out + fblk[blockIdx.x] + foff[i]);
}
// kBtGroup lanes per record.  All of them write SEQ and QUAL, a chunk of 8 characters per lane and turn; the group's first lane then writes
// what stands in front (QNAME to TLEN) and behind (the tags, the newline).  Every write lies inside the record's own line, whose length
// bt_record_len measured from the same bytes; a line that would pass the counted size of the text is not written.
__global__ __launch_bounds__(SWG) void k_bt_emit(const uint8_t* __restrict__ s, uint64_t nrec, const uint64_t* __restrict__ rec_off, BtRefs R, BtFloats F, const uint64_t* __restrict__ fblk,
                                                 const uint32_t* __restrict__ foff, const uint32_t* __restrict__ len, const uint32_t* __restrict__ seq_at, const uint64_t* __restrict__ tbase,
                                                 const uint64_t* __restrict__ line_off, uint8_t* __restrict__ text, uint64_t text_len) {
    const uint32_t g = threadIdx.x / kBtGroup, l = threadIdx.x % kBtGroup;
    const uint64_t i = (uint64_t)blockIdx.x * kBtPerWg + g;
    if (i >= nrec) return;
    const uint64_t at = tbase[i / SWG] + line_off[i];
    if (at + len[i] > text_len) return;
    uint8_t* d = text + at;
    const uint64_t off = rec_off[i];
    const BtBody B = bt_body(s, off);
    const uint32_t sa = seq_at[i], nch = (B.l_seq + 7u) >> 3;
    uint8_t* dq = d + sa + (B.l_seq ? B.l_seq : 1u) + 1u;
    for (uint32_t j = l; j < nch; j += kBtGroup) bt_emit_seq_chunk(s, B.seq, B.l_seq, j, d + sa);
    if (B.has_qual) for (uint32_t j = l; j < nch; j += kBtGroup) bt_emit_qual_chunk(s, B.qual, B.l_seq, j, dq);
    if (l == 0) {
        (void)bt_emit_head(s, off, R, d);
        if (!B.l_seq) d[sa] = '*';
        d[sa + (B.l_seq ? B.l_seq : 1u)] = '\t';
        if (!B.has_qual) dq[0] = '*';
        (void)bt_emit_tags(s, B, F, F.len ? fblk[i / SWG] + foff[i] : 0ull, dq + (B.has_qual ? B.l_seq : 1u));
    }
}
}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------------
struct mkt_bamtext {
    int device = 0;
    DevStream stream;                                   // declared first: destroyed after every buffer
    GrowBuf<uint8_t> buf;                               // the carry of the run before, then what was added since
    uint64_t held = 0, consumed = 0, records_before = 0;    // bytes in buf; stream offset of buf[0]; records of the runs before
    bool hdr_done = false, ran = false;
    BtHeader hdr;
    std::string hdr_out;
    DevBuf<uint8_t> dnames; DevBuf<uint32_t> dnoff;
    GrowBuf<uint8_t> text; uint64_t text_len = 0;
    // the arrays of a run: they only grow and live as long as the reader, so that a run of many (bam2sam's batches) allocates nothing
    GrowBuf<BtSeg> seg; GrowBuf<BtIndex> dX; GrowBuf<BtSums> dS;
    GrowBuf<uint64_t> sbase, rec_off, line_off, blk_len, tbase, fbase;
    GrowBuf<uint32_t> r32, b32, fbits;
    GrowBuf<uint8_t> fstr, flen, tmp;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    std::string err;
};
static int tfail(mkt_bamtext* p, int code, const char* fmt, ...) {
    char buf[640];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf;
    return code;
}
#define TCHK(p, call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return tfail((p), MKT_E_NOMEM, "%s: the device memory does not suffice (feed smaller pieces)", #call); } \
                           if (e_ != hipSuccess) return tfail((p), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// room for n elements in a buffer that only grows (a quarter more than asked for, so that batches of about one size settle)
template <typename T>
static hipError_t bt_need(GrowBuf<T>& b, size_t n) {
    if (b.get() && b.fits(n)) return hipSuccess;
    return b.regrow(n + n / 4 + 16);
}
static void bt_forget(mkt_bamtext* p) {                  // a new stream may follow
    p->held = p->consumed = p->records_before = 0;
    p->hdr_done = false;
    p->hdr = BtHeader();
    p->hdr_out.clear();
}
static int bt_refuse(mkt_bamtext* p, mkt_bamtext_info* I, uint32_t reason, uint64_t record, uint64_t offset) {
    I->reason = reason; I->bad_record = record; I->bad_offset = offset;
    bt_forget(p);
    p->ran = false; p->text_len = 0;
    p->text.reset();
    return tfail(p, MKT_E_FORMAT, "record %llu at %llu: %s [%s]", (unsigned long long)record, (unsigned long long)offset, bt_reason_text(reason), bt_reason_key(reason));
}
static int bt_room(mkt_bamtext* p, size_t n) {
    const size_t need = p->held + n;
    if (!p->buf.fits(need + 64)) {
        size_t ncap = p->buf.cap() > 64 ? p->buf.cap() - 64 : ((size_t)1 << 20);
        while (ncap < need) ncap *= 2;
        TCHK(p, p->buf.regrow_keep(ncap + 64, p->held));
    }
    return MKT_OK;
}

// the header from the first bytes of the stream; *start the offset of the first record in buf, or MKT_OK with hdr_done still false
static int bt_read_header(mkt_bamtext* p, mkt_bamtext_info* I) {
    std::vector<uint8_t> h;
    for (uint64_t want = 1 << 16;; want *= 4) {
        const uint64_t got = want < p->held ? want : p->held;
        h.resize(got + 1);
        if (got) TCHK(p, hipMemcpy(h.data(), p->buf.get(), got, hipMemcpyDeviceToHost));
        const uint32_t r = bt_header(h.data(), got, p->hdr);
        if (r == kBtIncomplete && got < p->held) continue;
        if (r == kBtIncomplete) return MKT_OK;
        if (r) return bt_refuse(p, I, r, 0, 0);
        break;
    }
    const size_t nr = p->hdr.names.size();
    std::vector<uint32_t> off(nr + 1, 0);
    std::string tab;
    for (size_t k = 0; k < nr; ++k) { tab += p->hdr.names[k]; off[k + 1] = (uint32_t)tab.size(); }
    TCHK(p, p->dnames.alloc(tab.size(), 64));
    TCHK(p, p->dnoff.alloc(nr + 1));
    if (!tab.empty()) TCHK(p, hipMemcpy(p->dnames, tab.data(), tab.size(), hipMemcpyHostToDevice));
    TCHK(p, hipMemcpy(p->dnoff, off.data(), (nr + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->hdr_out = bt_header_text(p->hdr.text);
    p->hdr_done = true;
    return MKT_OK;
}

static int bt_run(mkt_bamtext* p, uint32_t seg_bytes, uint32_t max_record, mkt_bamtext_info* I) {
    hipStream_t st = p->stream;
    DevEvents<7> ev;
    TCHK(p, ev.create());
    TCHK(p, hipEventRecord(ev[0], st));
    TCHK(p, bt_need(p->text, 64));
    TCHK(p, hipMemsetAsync(p->text.get(), 0, 64, st));
    uint64_t start = 0;
    if (!p->hdr_done) {
        if (const int rc = bt_read_header(p, I)) return rc;
        if (!p->hdr_done) { I->carry_bytes = p->held; return MKT_OK; }
        start = p->hdr.end;
    }
    I->header_done = 1;
    TCHK(p, hipEventRecord(ev[1], st));
    const uint8_t* s = p->buf.get();
    const uint64_t n = p->held, nseg = (n - start + seg_bytes - 1) / seg_bytes;
    if (nseg >= 0x7FFFFFFFull) return tfail(p, MKT_E_CAPACITY, "%llu segments: a launch takes fewer than 2^31 (feed smaller pieces or raise segment_bytes)", (unsigned long long)nseg);
    const BtRefs R = {p->dnames.get(), p->dnoff.get(), (int32_t)p->hdr.names.size()};
    BtIndex X;
    memset(&X, 0, sizeof X);
    X.tail = start;
    GrowBuf<BtSeg>& seg = p->seg; GrowBuf<BtIndex>& dX = p->dX; GrowBuf<uint64_t>& sbase = p->sbase;
    if (nseg) {
        TCHK(p, bt_need(seg, nseg)); TCHK(p, bt_need(dX, 1)); TCHK(p, bt_need(sbase, nseg + 1));
        hipLaunchKernelGGL(k_bt_guess, dim3((unsigned)nseg), dim3(SWG), 0, st, s, n, start, (uint64_t)seg_bytes, R.n_ref, max_record, seg.get());
        TCHK(p, hipGetLastError());
        TCHK(p, hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_bt_resolve, dim3(1), dim3(64), 0, st, s, n, start, (uint64_t)seg_bytes, nseg, max_record, seg.get(), dX.get());
        TCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_bt_scan_counts, dim3(1), dim3(SWG), 0, st, (const BtSeg*)seg.get(), nseg, sbase.get());
        TCHK(p, hipGetLastError());
        TCHK(p, hipMemcpyAsync(&X, dX.get(), sizeof X, hipMemcpyDeviceToHost, st));
        TCHK(p, hipStreamSynchronize(st));              // the number of records sizes what follows
    } else TCHK(p, hipEventRecord(ev[2], st));
    I->segments = nseg; I->repairs = X.repairs;
    if (X.reason) return bt_refuse(p, I, X.reason, p->records_before + X.bad_record, p->consumed + X.bad_offset);
    const uint64_t nrec = X.records, nblk = (nrec + SWG - 1) / SWG;
    if (nblk >= 0x7FFFFFFFull / (SWG / kBtPerWg)) return tfail(p, MKT_E_CAPACITY, "%llu records in one run: feed smaller pieces", (unsigned long long)nrec);
    BtSums S;
    memset(&S, 0, sizeof S);
    S.first_bad = kBtNone;
    if (nrec) {
        GrowBuf<uint64_t>&rec_off = p->rec_off, &line_off = p->line_off, &blk_len = p->blk_len, &tbase = p->tbase, &fbase = p->fbase;
        GrowBuf<uint32_t>&r32 = p->r32, &b32 = p->b32, &fbits = p->fbits;
        GrowBuf<BtSums>& dS = p->dS;
        TCHK(p, bt_need(rec_off, nrec)); TCHK(p, bt_need(line_off, nrec)); TCHK(p, bt_need(blk_len, nblk)); TCHK(p, bt_need(tbase, nblk + 1)); TCHK(p, bt_need(fbase, nblk + 1));
        TCHK(p, bt_need(r32, 5 * nrec)); TCHK(p, bt_need(b32, 3 * nblk)); TCHK(p, bt_need(dS, 1));
        uint32_t* len = r32.get(); uint32_t* seq_at = len + nrec; uint32_t* nf = seq_at + nrec; uint32_t* rst = nf + nrec; uint32_t* foff = rst + nrec;
        uint32_t* blk_nf = b32.get(); uint32_t* blk_frec = blk_nf + nblk; uint32_t* blk_bad = blk_frec + nblk;
        hipLaunchKernelGGL(k_bt_fill, dim3((unsigned)((nseg + SWG - 1) / SWG)), dim3(SWG), 0, st, s, (const BtSeg*)seg.get(), nseg, (const uint64_t*)sbase.get(), nrec, rec_off.get());
        TCHK(p, hipGetLastError());
        TCHK(p, hipEventRecord(ev[3], st));
        BtFloats F = {nullptr, nullptr};
        GrowBuf<uint8_t>&fstr = p->fstr, &flen = p->flen;
        float ms_len = 0, ms_scan = 0;
        for (int pass = 0; pass < 2; ++pass) {            // a second turn only where the stream holds floats: their text comes from the host
            DevEvents<3> pe;
            TCHK(p, pe.create());
            TCHK(p, hipEventRecord(pe[0], st));
            hipLaunchKernelGGL(k_bt_len, dim3((unsigned)nblk), dim3(SWG), 0, st, s, nrec, (const uint64_t*)rec_off.get(), R, F, (const uint64_t*)fbase.get(), (const uint32_t*)foff, len, seq_at, nf, rst);
            TCHK(p, hipGetLastError());
            TCHK(p, hipEventRecord(pe[1], st));
            hipLaunchKernelGGL(k_bt_sums, dim3((unsigned)nblk), dim3(SWG), 0, st, nrec, (const uint32_t*)len, (const uint32_t*)nf, (const uint32_t*)rst, line_off.get(), foff, blk_len.get(), blk_nf, blk_frec, blk_bad);
            TCHK(p, hipGetLastError());
            hipLaunchKernelGGL(k_bt_bases, dim3(1), dim3(SWG), 0, st, nblk, (const uint64_t*)blk_len.get(), (const uint32_t*)blk_nf, (const uint32_t*)blk_frec, (const uint32_t*)blk_bad, (const uint32_t*)rst,
                               tbase.get(), fbase.get(), dS.get());
            TCHK(p, hipGetLastError());
            TCHK(p, hipEventRecord(pe[2], st));
            TCHK(p, hipMemcpyAsync(&S, dS.get(), sizeof S, hipMemcpyDeviceToHost, st));
            TCHK(p, hipStreamSynchronize(st));          // the size of the text, the number of floats, the first record refused
            float a = 0, b = 0;
            TCHK(p, hipEventElapsedTime(&a, pe[0], pe[1])); TCHK(p, hipEventElapsedTime(&b, pe[1], pe[2]));
            ms_len += a; ms_scan += b;
            if (S.first_bad != kBtNone) {
                uint64_t at = 0;
                TCHK(p, hipMemcpy(&at, rec_off.get() + S.first_bad, sizeof at, hipMemcpyDeviceToHost));
                return bt_refuse(p, I, S.reason, p->records_before + S.first_bad, p->consumed + at);
            }
            if (pass || !S.floats) break;
            TCHK(p, bt_need(fbits, S.floats));
            hipLaunchKernelGGL(k_bt_floats, dim3((unsigned)nblk), dim3(SWG), 0, st, s, nrec, (const uint64_t*)rec_off.get(), (const uint32_t*)nf, (const uint64_t*)fbase.get(), (const uint32_t*)foff, fbits.get());
            TCHK(p, hipGetLastError());
            std::vector<uint32_t> hb(S.floats);
            TCHK(p, hipMemcpyAsync(hb.data(), fbits.get(), S.floats * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            TCHK(p, hipStreamSynchronize(st));
            std::vector<uint8_t> hs(S.floats * kBtFloatSlot, 0), hl(S.floats);
            for (uint64_t k = 0; k < S.floats; ++k) hl[k] = (uint8_t)bt_format_float(hb[k], hs.data() + k * kBtFloatSlot);
            TCHK(p, bt_need(fstr, hs.size())); TCHK(p, bt_need(flen, hl.size()));
            TCHK(p, hipMemcpyAsync(fstr, hs.data(), hs.size(), hipMemcpyHostToDevice, st));
            TCHK(p, hipMemcpyAsync(flen, hl.data(), hl.size(), hipMemcpyHostToDevice, st));
            TCHK(p, hipStreamSynchronize(st));          // the host vectors end here
            F.str = fstr.get(); F.len = flen.get();
        }
        p->ms[3] = ms_len; p->ms[4] = ms_scan;
        TCHK(p, bt_need(p->text, S.text_bytes + 64));
        TCHK(p, hipMemsetAsync(p->text.get() + S.text_bytes, 0, 64, st));
        TCHK(p, hipEventRecord(ev[4], st));
        hipLaunchKernelGGL(k_bt_emit, dim3((unsigned)((nrec + kBtPerWg - 1) / kBtPerWg)), dim3(SWG), 0, st, s, nrec, (const uint64_t*)rec_off.get(), R, F, (const uint64_t*)fbase.get(), (const uint32_t*)foff,
                           (const uint32_t*)len, (const uint32_t*)seq_at, (const uint64_t*)tbase.get(), (const uint64_t*)line_off.get(), p->text.get(), S.text_bytes);
        TCHK(p, hipGetLastError());
        TCHK(p, hipEventRecord(ev[5], st));
        TCHK(p, hipStreamSynchronize(st));              // the record arrays end here
        float f = 0;
        TCHK(p, hipEventElapsedTime(&f, ev[2], ev[3])); p->ms[2] = f;
        TCHK(p, hipEventElapsedTime(&f, ev[4], ev[5])); p->ms[5] = f;
    }
    TCHK(p, hipStreamSynchronize(st));
    { float f = 0; TCHK(p, hipEventElapsedTime(&f, ev[0], ev[1])); p->ms[0] = f; TCHK(p, hipEventElapsedTime(&f, ev[1], ev[2])); p->ms[1] = f; }
    // the carry: what is no complete record moves to the front (through a second buffer where the two ranges overlap)
    const uint64_t tail = n - X.tail;
    if (tail && X.tail) {
        GrowBuf<uint8_t>& tmp = p->tmp;
        if (X.tail >= tail) TCHK(p, hipMemcpyAsync(p->buf.get(), p->buf.get() + X.tail, tail, hipMemcpyDeviceToDevice, st));
        else {
            TCHK(p, bt_need(tmp, tail));
            TCHK(p, hipMemcpyAsync(tmp.get(), p->buf.get() + X.tail, tail, hipMemcpyDeviceToDevice, st));
            TCHK(p, hipMemcpyAsync(p->buf.get(), tmp.get(), tail, hipMemcpyDeviceToDevice, st));
        }
        TCHK(p, hipStreamSynchronize(st));
    }
    p->held = tail; p->consumed += X.tail; p->records_before += nrec;
    p->text_len = S.text_bytes;
    I->records = nrec; I->text_bytes = S.text_bytes; I->float_records = S.float_records; I->carry_bytes = tail;
    return MKT_OK;
}

extern "C" {

int mkt_bamtext_create(int device, mkt_bamtext** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_bamtext* p = new mkt_bamtext();
    p->device = device;
    if (hipSetDevice(device) != hipSuccess || p->stream.create(hipStreamNonBlocking) != hipSuccess) { mkt_bamtext_destroy(p); return MKT_E_HIP; }
    *out = p;
    return MKT_OK;
}
void mkt_bamtext_destroy(mkt_bamtext* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;
}
const char* mkt_bamtext_error(const mkt_bamtext* p) { return p ? p->err.c_str() : ""; }

int mkt_bamtext_add(mkt_bamtext* p, const char* bytes, size_t n) {
    if (!p || (n && !bytes)) return MKT_E_ARG;
    TCHK(p, hipSetDevice(p->device));
    if (const int rc = bt_room(p, n)) return rc;
    if (n) TCHK(p, hipMemcpyAsync(p->buf.get() + p->held, bytes, n, hipMemcpyHostToDevice, p->stream));
    TCHK(p, hipStreamSynchronize(p->stream));           // the caller may reuse `bytes`
    p->held += n;
    return MKT_OK;
}
int mkt_bamtext_add_device(mkt_bamtext* p, const void* d_bytes, uint64_t n) {
    if (!p || (n && !d_bytes)) return MKT_E_ARG;
    TCHK(p, hipSetDevice(p->device));
    if (const int rc = bt_room(p, n)) return rc;
    if (n) TCHK(p, hipMemcpyAsync(p->buf.get() + p->held, d_bytes, n, hipMemcpyDeviceToDevice, p->stream));
    TCHK(p, hipStreamSynchronize(p->stream));           // the caller may free or overwrite `d_bytes`
    p->held += n;
    return MKT_OK;
}
void mkt_bamtext_opts_default(mkt_bamtext_opts* o) { if (o) memset(o, 0, sizeof *o); }

int mkt_bamtext_run(mkt_bamtext* p, const mkt_bamtext_opts* opts, mkt_bamtext_info* info) {
    if (!p) return MKT_E_ARG;
    uint32_t seg = kBtDefaultSegment, maxrec = kBtMaxRecord;
    if (opts) {
        for (uint32_t r : opts->reserved) if (r) return tfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
        if (opts->segment_bytes) seg = opts->segment_bytes;
        if (opts->max_record) maxrec = opts->max_record;
        if (seg < kBtMinSegment || (seg & (seg - 1))) return tfail(p, MKT_E_ARG, "segment_bytes is 0 or a power of two of at least 256");
        if (maxrec < 32 || maxrec > kBtMaxRecord) return tfail(p, MKT_E_ARG, "max_record is 0 or lies in [32, 16 MiB]");
    }
    mkt_bamtext_info I;
    memset(&I, 0, sizeof I);
    if (info) *info = I;
    TCHK(p, hipSetDevice(p->device));
    p->ran = false; p->text_len = 0;
    for (double& m : p->ms) m = 0;
    if (!p->buf.get()) TCHK(p, p->buf.regrow(((size_t)1 << 20) + 64));
    const int rc = bt_run(p, seg, maxrec, &I);
    if (info) *info = I;
    if (rc != MKT_OK) { p->text.reset(); p->text_len = 0; return rc; }
    p->ran = true;
    return MKT_OK;
}
int mkt_bamtext_finish(mkt_bamtext* p, mkt_bamtext_info* info) {
    if (!p) return MKT_E_ARG;
    mkt_bamtext_info I;
    memset(&I, 0, sizeof I);
    I.header_done = p->hdr_done ? 1u : 0u;
    I.carry_bytes = p->held;
    int rc = MKT_OK;
    if (!p->hdr_done) rc = bt_refuse(p, &I, BT_HEADER_TRUNCATED, 0, p->held);
    else if (p->held) rc = bt_refuse(p, &I, BT_TRUNCATED, p->records_before, p->consumed);
    else { p->held = p->consumed = p->records_before = 0; p->hdr_done = false; }      // the header and the text of the last run stay until the next stream's
    if (info) *info = I;
    return rc;
}
int mkt_bamtext_fetch_header(mkt_bamtext* p, uint64_t off, char* out, size_t n, uint64_t* total) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (p->hdr.end == 0) return tfail(p, MKT_E_STATE, "header before a run that reached the end of it");
    if (total) *total = p->hdr_out.size();
    if (off > p->hdr_out.size() || n > p->hdr_out.size() - off) return tfail(p, MKT_E_ARG, "range past the end of the header text");
    if (n) memcpy(out, p->hdr_out.data() + off, n);
    return MKT_OK;
}
int mkt_bamtext_fetch_ref(mkt_bamtext* p, uint32_t k, char* name, size_t cap, int32_t* length, uint32_t* n_ref) {
    if (!p) return MKT_E_ARG;
    if (p->hdr.end == 0) return tfail(p, MKT_E_STATE, "references before a run that reached the end of the header");
    if (n_ref) *n_ref = (uint32_t)p->hdr.names.size();
    if (!name && !length) return MKT_OK;
    if (k >= p->hdr.names.size()) return tfail(p, MKT_E_ARG, "no such reference");
    if (name) { if (cap < p->hdr.names[k].size() + 1) return tfail(p, MKT_E_ARG, "the name takes %zu bytes", p->hdr.names[k].size() + 1); memcpy(name, p->hdr.names[k].c_str(), p->hdr.names[k].size() + 1); }
    if (length) *length = p->hdr.lengths[k];
    return MKT_OK;
}
int mkt_bamtext_fetch_text(mkt_bamtext* p, uint64_t off, char* out, size_t n) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->ran) return tfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    if (off > p->text_len || n > p->text_len - off) return tfail(p, MKT_E_ARG, "range past the end of the text");
    TCHK(p, hipSetDevice(p->device));
    if (n) TCHK(p, hipMemcpy(out, p->text.get() + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_bamtext_device_text(mkt_bamtext* p, const void** d_ptr, uint64_t* n) {
    if (!p || !d_ptr || !n) return MKT_E_ARG;
    if (!p->ran) return tfail(p, MKT_E_STATE, "device text before a run that succeeded");
    *d_ptr = p->text.get();
    *n = p->text_len;
    return MKT_OK;
}
int mkt_bamtext_timing(const mkt_bamtext* p, double ms[6]) {
    if (!p || !ms) return MKT_E_ARG;
    for (int k = 0; k < 6; ++k) ms[k] = p->ms[k];
    return MKT_OK;
}

}  // extern "C"
