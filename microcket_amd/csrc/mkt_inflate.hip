// mkt_inflate.hip -- BGZF (SAMv1 4.1) read back on the GPU: the inflate of RFC 1951 with one wavefront per BGZF block, the CRC-32 and
// ISIZE of every inflated block checked against its footer, the region queries through a .px2, and the reader object of include/mkt.h
// (mkt_bgzf_*).  DESIGN.md 6g has the layout and the arguments of the inflate, 6h those of the queries; mkt_inflate.h the functions that
// decide what is accepted, mkt_px2query.h the plan of a query and its line filter (both shared with the host drivers).
//
// One workgroup is one wavefront.  It copies the compressed span of its block into LDS, decodes symbols serially (every lane runs the
// same decode on the same LDS words, so all values of the decode are the same in every lane), keeps a batch of up to kInfBatch tokens, one per
// lane, and expands the batch into an LDS image of the block's output: literals at the offsets a wave scan of the token lengths gives,
// then the matches in order, 64 bytes per step.  A match reads bytes that other lanes wrote just before it; both sides are LDS accesses
// of one workgroup with a barrier between them, and nothing of the output is in global memory until the block is complete.  The only
// global reads are the coalesced copy of the member's bytes, the only global writes the coalesced copy of out[0, ISIZE) and one
// status record.  No atomics.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_deflate.h"
#include "mkt_devbuf.h"
#include "mkt_blockscan.h"
#include "mkt_inflate.h"
#include "mkt_px2query.h"

using namespace mkt;

namespace mkt {

static_assert(kInfMaxIsize == BGZF_STRIDE, "a BGZF block inflates to at most 64 KiB");
constexpr uint32_t kInfWave = 64;
constexpr uint32_t kInfInBytes = BGZF_STRIDE + 16;      // 3 bytes of alignment + a span of at most 65510 bytes + kInfSpanPad zeros
constexpr int kCrcWg = 256;

struct InfResult { uint32_t status, kinds[3]; };        // per block: why it is refused (0: it is not); deflate blocks stored / fixed / dynamic

struct InfLds {
    alignas(16) uint8_t in[kInfInBytes];
    alignas(16) uint8_t out[kInfMaxIsize];
    InfTables t;
};
static_assert(sizeof(InfLds) <= 140 * 1024, "one workgroup per CU: 160 KiB of LDS");

// list: the blocks to inflate (nullptr: block blockIdx.x).  Block j of the launch writes text[tbase[j] .. + ISIZE) where tbase is given
// (a query's compact buffer), else text[toff of the block ..).
__global__ __launch_bounds__(kInfWave) void k_inflate(const uint8_t* __restrict__ gz, const InfBlock* __restrict__ blocks, const uint32_t* __restrict__ list,
                                                      const uint64_t* __restrict__ tbase, uint8_t* __restrict__ text, InfResult* __restrict__ res) {
    __shared__ InfLds L;
    const uint32_t lane = threadIdx.x;
    const uint32_t j = blockIdx.x;
    const InfBlock B = blocks[list ? list[j] : j];
    const uint32_t isize = B.isize;                      // <= kInfMaxIsize: the block table refuses more
    const uint32_t nspan = B.bsize - kInfHead - kInfFoot;    // bsize in [26, 65536]: the block table refuses anything else
    // ---- the member's bytes -> LDS, as aligned words.  The words may begin up to 3 bytes before the span (in the member's header)
    // and end up to 3 bytes behind it (in its footer): never outside the member.
    const uint8_t* src = gz + B.coff + kInfHead;
    const uint32_t a = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t* src4 = (const uint32_t*)(src - a);
    const uint32_t nwords = (a + nspan + 3u) >> 2;       // <= (3 + 65510 + 3) / 4: inside L.in
    for (uint32_t i = lane; i < nwords; i += kInfWave) ((uint32_t*)L.in)[i] = src4[i];
    __syncthreads();
    if (lane < kInfSpanPad) L.in[a + nspan + lane] = 0;  // what the bit reader may look at behind the span
    __syncthreads();

    InfBits b = {L.in, a * 8u, (a + nspan) * 8u};
    uint32_t outpos = 0, status = INF_OK, kinds[3] = {0, 0, 0};
    for (;;) {                                           // the deflate blocks of the member: each turn takes at least 3 bits of the span
        uint32_t bfinal = 0, btype = 0;
        status = inf_block_head(b, &bfinal, &btype);
        if (status) break;
        kinds[btype]++;
        if (btype == 0) {
            uint32_t n = 0;
            status = inf_stored_head(b, outpos, isize, &n);      // n bytes lie inside the span and fit below isize
            if (status) break;
            const uint32_t q = b.p >> 3;
            for (uint32_t i = lane; i < n; i += kInfWave) L.out[outpos + i] = L.in[q + i];
            b.p += 8u * n;
            outpos += n;
            __syncthreads();
        } else {
            if (btype == 1) { if (lane == 0) inf_fixed(L.t); }
            else {
                // the header is parsed by one lane (it writes the tables); its verdict and the reader's position go to all lanes
                uint32_t st = 0, np = b.p;
                if (lane == 0) { st = inf_dynamic(b, L.t); np = b.p; }
                status = (uint32_t)__shfl((int)st, 0, kInfWave);
                b.p = (uint32_t)__shfl((int)np, 0, kInfWave);
            }
            __syncthreads();
            if (status) break;
            bool eob = false;
            while (!eob) {                               // a batch: every token takes at least one bit of the span
                uint32_t mytok = 0, ntok = 0, pos = outpos;
                while (ntok < kInfBatch) {
                    uint32_t tk = 0;
                    const int r = inf_token(b, L.t, pos, isize, &tk);
                    if (r < 0) { status = (uint32_t)-r; break; }
                    if (r == 1) { eob = true; break; }
                    if (lane == ntok) mytok = tk;
                    pos += tk >> 16;                     // <= isize: inf_token refuses a token that would pass it
                    ++ntok;
                }
                if (status) break;
                // literals: the offset of every token from a wave scan of the lengths
                const uint32_t len = lane < ntok ? mytok >> 16 : 0u;
                uint32_t inc = len;
                for (uint32_t d = 1; d < kInfWave; d <<= 1) {
                    const uint32_t v = (uint32_t)__shfl_up((int)inc, d, kInfWave);
                    if (lane >= d) inc += v;
                }
                const uint32_t off = outpos + inc - len;
                if (len == 1) L.out[off] = (uint8_t)mytok;
                __syncthreads();
                // matches in order; the source of a match lies wholly in front of its first byte when taken modulo the distance
                uint64_t mm = __ballot(len >= 3);
                while (mm) {
                    const int k = __ffsll((unsigned long long)mm) - 1;
                    mm &= mm - 1;
                    const uint32_t ml = (uint32_t)__shfl((int)len, k, kInfWave), md = ((uint32_t)__shfl((int)mytok, k, kInfWave) & 0xFFFFu) + 1u;
                    const uint32_t dst = (uint32_t)__shfl((int)off, k, kInfWave), from = dst - md;      // md <= dst: inf_token refuses another
                    for (uint32_t i = lane; i < ml; i += kInfWave) L.out[dst + i] = L.out[from + (md >= ml ? i : i % md)];
                    __syncthreads();
                }
                outpos = pos;
            }
            if (status) break;
        }
        if (bfinal) break;
    }
    if (!status) status = inf_member_end(b, outpos, isize);
    if (!status) {
        uint8_t* dst = text + (tbase ? tbase[j] : B.toff);
        if ((((uintptr_t)dst) & 3u) == 0) {
            const uint32_t nw = isize >> 2;
            for (uint32_t i = lane; i < nw; i += kInfWave) ((uint32_t*)dst)[i] = ((const uint32_t*)L.out)[i];
            for (uint32_t i = (nw << 2) + lane; i < isize; i += kInfWave) dst[i] = L.out[i];
        } else {
            for (uint32_t i = lane; i < isize; i += kInfWave) dst[i] = L.out[i];
        }
    }
    if (lane == 0) { InfResult r; r.status = status; r.kinds[0] = kinds[0]; r.kinds[1] = kinds[1]; r.kinds[2] = kinds[2]; res[j] = r; }
}

// the CRC-32 of every block that inflated, against its footer (the routine of the BGZF writer: slices combined as polynomials)
__global__ __launch_bounds__(kCrcWg) void k_inflate_crc(const InfBlock* __restrict__ blocks, const uint32_t* __restrict__ list, const uint64_t* __restrict__ tbase,
                                                         const uint8_t* __restrict__ text, const CrcTabs* __restrict__ ct, InfResult* __restrict__ res) {
    __shared__ uint32_t tabl[256], x2n[32], sh[kCrcWg / 64];
    tabl[threadIdx.x] = ct->t[threadIdx.x];
    if (threadIdx.x < 32) x2n[threadIdx.x] = ct->x2n[threadIdx.x];
    __syncthreads();
    const uint32_t j = blockIdx.x;
    if (res[j].status) return;                           // (the same for every thread of the workgroup)
    const InfBlock B = blocks[list ? list[j] : j];
    const uint32_t crc = block_crc<kCrcWg>(text + (tbase ? tbase[j] : B.toff), B.isize, tabl, x2n, sh);
    if (threadIdx.x == 0 && crc != B.crc) res[j].status = INF_CRC;
}


// ---- region queries (mkt_px2query.h has the plan and the line filter) ------------------------------------------------------
// The spans of a batch, in region order, then sub-query order, then file order, are laid one behind the other as "virtual bytes":
// cum[s] is the virtual offset of span s, cum[ns] their sum.  A workgroup takes a tile of kQTile virtual bytes, a thread kQPer
// consecutive ones.  Every read of the text lies inside a span: a byte is a line start when it is its span's first byte or the byte in
// front of it, in the same span, is a newline.  No atomics: counts are scanned, so every array is the same on every call.
constexpr uint32_t kQPer = 16, kQTile = SWG * kQPer;

struct QScanJob { const uint32_t* in; uint64_t* out; uint64_t n; };       // out[0 .. n]: the exclusive sums and the total
struct QScanJobs { QScanJob j[3]; };

__device__ inline uint32_t q_span_of(const uint64_t* __restrict__ cum, uint32_t ns, uint64_t v) {      // the span that holds virtual byte v < cum[ns]
    uint32_t lo = 0, hi = ns;                            // cum[lo] <= v < cum[hi]
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (cum[mid] <= v) lo = mid; else hi = mid; }
    return lo;
}
// the line starts among the kQPer virtual bytes from v0 as a bit mask; *s0 the span of v0
__device__ inline uint32_t q_starts(const uint8_t* __restrict__ text, const QSpan* __restrict__ spans, const uint64_t* __restrict__ cum, uint32_t ns, uint64_t v0, uint32_t* s0) {
    const uint64_t total = cum[ns];
    if (v0 >= total) { *s0 = ns; return 0; }
    uint32_t s = q_span_of(cum, ns, v0), mask = 0;
    *s0 = s;
    uint64_t c0 = cum[s], c1 = cum[s + 1], lo = spans[s].lo;
    for (uint32_t k = 0; k < kQPer; ++k) {
        const uint64_t v = v0 + k;
        if (v >= total) break;
        if (v >= c1) { ++s; c0 = c1; c1 = cum[s + 1]; lo = spans[s].lo; }      // spans are not empty: one step suffices
        if (v == c0 || text[lo + (v - c0) - 1] == '\n') mask |= 1u << k;
    }
    return mask;
}
__global__ __launch_bounds__(SWG) void k_query_count(const uint8_t* __restrict__ text, const QSpan* __restrict__ spans, const uint64_t* __restrict__ cum, uint32_t ns, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t sh[SWG / 64];
    uint32_t s0, tot;
    const uint32_t m = q_starts(text, spans, cum, ns, (uint64_t)blockIdx.x * kQTile + (uint64_t)threadIdx.x * kQPer, &s0);
    (void)blk_exscan((uint32_t)__popc(m), &tot, sh);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}
// exclusive sums of up to three arrays, one workgroup each (the tiles of the spans; the blocks of candidates)
__global__ __launch_bounds__(SWG) void k_query_scan(QScanJobs jobs) {
    __shared__ uint32_t sh[SWG / 64];
    const QScanJob J = jobs.j[blockIdx.x];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < J.n; base += SWG) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < J.n ? J.in[i] : 0u;
        uint32_t tot;
        const uint32_t ex = blk_exscan(v, &tot, sh);
        if (i < J.n) J.out[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) J.out[J.n] = carry;
}
// the candidates: where each line starts (an offset of the text buffer) and in which span; span_first[s]: the first candidate of span s
__global__ __launch_bounds__(SWG) void k_query_lines(const uint8_t* __restrict__ text, const QSpan* __restrict__ spans, const uint64_t* __restrict__ cum, uint32_t ns,
                                                      const uint64_t* __restrict__ tile_base, uint64_t ncand, uint64_t* __restrict__ cand_pos, uint32_t* __restrict__ cand_span,
                                                      uint64_t* __restrict__ span_first) {
    __shared__ uint32_t sh[SWG / 64];
    uint32_t s, tot;
    const uint64_t v0 = (uint64_t)blockIdx.x * kQTile + (uint64_t)threadIdx.x * kQPer;
    uint32_t m = q_starts(text, spans, cum, ns, v0, &s);
    uint64_t at = tile_base[blockIdx.x] + blk_exscan((uint32_t)__popc(m), &tot, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) span_first[ns] = ncand;
    if (!m) return;
    uint64_t c0 = cum[s], c1 = cum[s + 1];
    for (uint32_t k = 0; k < kQPer && (m >> k); ++k) {
        const uint64_t v = v0 + k;
        if (v >= c1) { ++s; c0 = c1; c1 = cum[s + 1]; }
        if (!(m >> k & 1u)) continue;
        if (at < ncand) {                                // (the count of the first pass: never exceeded)
            cand_pos[at] = spans[s].lo + (v - c0);
            cand_span[at] = s;
            if (v == c0) span_first[s] = at;
        }
        ++at;
    }
}
// One work item per candidate line: its end (the newline, or the end of its span), the filter of mkt_px2query.h, and the sums of one
// workgroup: bytes the line takes in the answer (with its '\n'; 0 where it does not match), lines matched, lines unparsed.
__global__ __launch_bounds__(SWG) void k_query_filter(const uint8_t* __restrict__ text, const QSpan* __restrict__ spans, const QSub* __restrict__ subs, const uint8_t* __restrict__ names,
                                                       uint64_t ncand, const uint64_t* __restrict__ cand_pos, const uint32_t* __restrict__ cand_span, uint32_t* __restrict__ cand_len,
                                                       uint32_t* __restrict__ cand_off, uint32_t* __restrict__ cand_before, uint32_t* __restrict__ blk_bytes, uint32_t* __restrict__ blk_lines,
                                                       uint32_t* __restrict__ blk_unparsed) {
    __shared__ uint32_t sh[SWG / 64];
    const uint64_t i = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    uint32_t len = 0, hit = 0, bad = 0;
    if (i < ncand) {
        const QSpan S = spans[cand_span[i]];
        const QSub Q = subs[S.sub];
        const uint64_t p = cand_pos[i];                  // S.lo <= p < S.hi
        uint64_t e = p;
        while (e < S.hi && text[e] != '\n') ++e;
        const uint32_t m = q_match_line(text + p, e - p, names + Q.a_off, Q.a_len, names + Q.b_off, Q.b_len, Q.b1, Q.e1, Q.b2, Q.e2);
        hit = m == 1u; bad = m == 2u;
        len = hit ? (uint32_t)(e - p) + 1u : 0u;         // a match has at most kQMaxLine bytes
    }
    uint32_t tb, tl, tu;
    const uint32_t ob = blk_exscan(len, &tb, sh), ol = blk_exscan(hit, &tl, sh);
    (void)blk_exscan(bad, &tu, sh);
    if (i < ncand) { cand_len[i] = len; cand_off[i] = ob; cand_before[i] = ol; }
    if (threadIdx.x == 0) { blk_bytes[blockIdx.x] = tb; blk_lines[blockIdx.x] = tl; blk_unparsed[blockIdx.x] = tu; }
}
// where the lines of every region begin in the answer, and how many lines stand in front of them
__global__ __launch_bounds__(SWG) void k_query_regions(const uint64_t* __restrict__ region_first, uint32_t nreg, uint32_t ns, const uint64_t* __restrict__ span_first, uint64_t ncand,
                                                        const uint32_t* __restrict__ cand_off, const uint32_t* __restrict__ cand_before, const uint64_t* __restrict__ base_bytes,
                                                        const uint64_t* __restrict__ base_lines, uint64_t nblk, uint64_t* __restrict__ region_off, uint64_t* __restrict__ region_before) {
    const uint32_t r = blockIdx.x * SWG + threadIdx.x;
    if (r > nreg) return;
    const uint64_t fs = region_first[r];                 // <= ns
    const uint64_t c = span_first[fs < ns ? fs : ns];
    if (c < ncand) { region_off[r] = base_bytes[c / SWG] + cand_off[c]; region_before[r] = base_lines[c / SWG] + cand_before[c]; }
    else { region_off[r] = base_bytes[nblk]; region_before[r] = base_lines[nblk]; }
}
// the matched lines of one block of candidates into the answer, a wavefront per line, each with a '\n' behind it
__global__ __launch_bounds__(SWG) void k_query_gather(const uint8_t* __restrict__ text, uint64_t ncand, const uint64_t* __restrict__ cand_pos, const uint32_t* __restrict__ cand_len,
                                                       const uint32_t* __restrict__ cand_off, const uint64_t* __restrict__ base_bytes, uint8_t* __restrict__ ans, uint64_t ans_len) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t b0 = (uint64_t)blockIdx.x * SWG, base = base_bytes[blockIdx.x];
    for (uint32_t k = wv; k < (uint32_t)SWG; k += SWG / 64) {
        const uint64_t i = b0 + k;
        if (i >= ncand) break;
        const uint32_t len = cand_len[i];
        if (!len) continue;
        const uint64_t dst = base + cand_off[i];
        if (dst + len > ans_len) continue;               // (the counted size: never exceeded)
        const uint8_t* src = text + cand_pos[i];
        for (uint32_t x = lane; x < len - 1u; x += 64u) ans[dst + x] = src[x];
        if (lane == 0) ans[dst + len - 1u] = '\n';
    }
}
}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------------
struct mkt_bgzf {
    int device = 0;
    DevStream stream;                                   // declared first: destroyed after every buffer
    std::vector<uint8_t> hgz;                           // the compressed bytes as they were added (the block table is walked on the host)
    GrowBuf<uint8_t> gz;                                // ... and on the device
    DevBuf<CrcTabs> ct;
    DevBuf<uint8_t> text; uint64_t text_len = 0;
    bool ran = false, have_index = false;
    uint64_t index_lines = 0;
    // region queries: the index as it was loaded (its name table also on the device), the block table of the file as it stands, the last answer
    Px2Index ix;
    DevBuf<uint8_t> dnames;
    std::vector<InfBlock> blocks;
    DevBuf<InfBlock> dblocks;
    bool have_blocks = false, index_checked = false, have_query = false;
    DevBuf<uint8_t> qans; uint64_t qans_len = 0;
    std::vector<uint64_t> qoff, qcnt;                    // n + 1 offsets of the regions' lines in the answer; n line counts
    double ms[5] = {0, 0, 0, 0, 0};
    std::string err;
};
static int bfail(mkt_bgzf* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf;
    return code;
}
#define BCHK(p, call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return bfail((p), MKT_E_NOMEM, "%s: the device memory does not suffice (the compressed bytes and the whole text are resident; there is no streaming in batches)", #call); } \
                           if (e_ != hipSuccess) return bfail((p), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// Inflates the BGZF file h_gz[0, n) (the same bytes at d_gz) into `text` (64 bytes of zeros behind it).  I gets the counters, or the
// reason and offset of the first block that is refused.  ms[0 .. 2]: table upload, inflate, CRC.
static int bz_inflate_file(mkt_bgzf* p, const uint8_t* h_gz, const uint8_t* d_gz, uint64_t n, const char* what, DevBuf<uint8_t>& text, uint64_t* text_len, mkt_bgzf_info* I, double* ms) {
    hipStream_t st = p->stream;
    memset(I, 0, sizeof *I);
    I->gz_bytes = n;
    std::vector<InfBlock> blocks;
    uint64_t bad = 0;
    bool has_eof = false;
    if (const uint32_t r = inf_block_table(h_gz, n, blocks, &bad, &has_eof)) {
        I->reason = r; I->bad_offset = bad;
        return bfail(p, MKT_E_FORMAT, "%s: block at %llu: %s [%s]", what, (unsigned long long)bad, inf_reason_text(r), inf_reason_key(r));
    }
    const uint64_t nb = blocks.size(), total = nb ? blocks.back().toff + blocks.back().isize : 0;
    if (nb >= 0x7FFFFFFFull) return bfail(p, MKT_E_CAPACITY, "%s: %llu blocks: a launch takes fewer than 2^31", what, (unsigned long long)nb);
    DevEvents<4> ev;
    BCHK(p, ev.create());
    BCHK(p, text.alloc(total, 64));
    BCHK(p, hipMemsetAsync(text + total, 0, 64, st));
    std::vector<InfResult> res(nb);
    BCHK(p, hipEventRecord(ev[0], st));
    if (nb) {
        DevBuf<InfBlock> dblocks;
        DevBuf<InfResult> dres;
        BCHK(p, dblocks.alloc(nb));
        BCHK(p, dres.alloc(nb));
        BCHK(p, hipMemcpyAsync(dblocks, blocks.data(), nb * sizeof(InfBlock), hipMemcpyHostToDevice, st));
        BCHK(p, hipEventRecord(ev[1], st));
        hipLaunchKernelGGL(k_inflate, dim3((unsigned)nb), dim3(kInfWave), 0, st, d_gz, (const InfBlock*)dblocks.get(), (const uint32_t*)nullptr, (const uint64_t*)nullptr, text.get(), dres.get());
        BCHK(p, hipGetLastError());
        BCHK(p, hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_inflate_crc, dim3((unsigned)nb), dim3(kCrcWg), 0, st, (const InfBlock*)dblocks.get(), (const uint32_t*)nullptr, (const uint64_t*)nullptr, (const uint8_t*)text.get(),
                           (const CrcTabs*)p->ct.get(), dres.get());
        BCHK(p, hipGetLastError());
        BCHK(p, hipEventRecord(ev[3], st));
        BCHK(p, hipMemcpyAsync(res.data(), dres, nb * sizeof(InfResult), hipMemcpyDeviceToHost, st));
        BCHK(p, hipStreamSynchronize(st));              // the table and the results end here
        for (int k = 0; k < 3; ++k) { float f = 0; BCHK(p, hipEventElapsedTime(&f, ev[k], ev[k + 1])); ms[k] = f; }
    }
    I->blocks = nb; I->text_bytes = total; I->has_eof = has_eof ? 1u : 0u;
    for (uint64_t k = 0; k < nb; ++k) {
        if (res[k].status) {
            I->reason = res[k].status; I->bad_offset = blocks[k].coff;
            return bfail(p, MKT_E_FORMAT, "%s: block at %llu: %s [%s]", what, (unsigned long long)blocks[k].coff, inf_reason_text(res[k].status), inf_reason_key(res[k].status));
        }
        I->stored += res[k].kinds[0]; I->fixed += res[k].kinds[1]; I->dynamic += res[k].kinds[2];
    }
    *text_len = total;
    return MKT_OK;
}

extern "C" {

int mkt_bgzf_create(int device, mkt_bgzf** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_bgzf* p = new mkt_bgzf();
    p->device = device;
    CrcTabs ct;
    crc_tables(&ct);
    if (hipSetDevice(device) != hipSuccess || p->stream.create(hipStreamNonBlocking) != hipSuccess || p->ct.alloc(1) != hipSuccess ||
        hipMemcpy(p->ct, &ct, sizeof ct, hipMemcpyHostToDevice) != hipSuccess) { mkt_bgzf_destroy(p); return MKT_E_HIP; }
    *out = p;
    return MKT_OK;
}
void mkt_bgzf_destroy(mkt_bgzf* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;                                           // the buffers, then the stream
}
const char* mkt_bgzf_error(const mkt_bgzf* p) { return p ? p->err.c_str() : ""; }

int mkt_bgzf_add(mkt_bgzf* p, const char* bytes, size_t n) {
    if (!p || (n && !bytes)) return MKT_E_ARG;
    BCHK(p, hipSetDevice(p->device));
    p->ran = false; p->text_len = 0;
    p->text.reset();
    p->have_blocks = p->index_checked = p->have_query = false;      // the file grows: its block table and the last answer go, a loaded index stays
    p->qans.reset();
    const size_t have = p->hgz.size(), need = have + n;
    if (!p->gz.fits(need + 64)) {
        size_t ncap = p->gz.cap() ? p->gz.cap() - 64 : ((size_t)1 << 20);
        while (ncap < need) ncap *= 2;
        BCHK(p, p->gz.regrow_keep(ncap + 64, have));
    }
    if (n) BCHK(p, hipMemcpyAsync(p->gz + have, bytes, n, hipMemcpyHostToDevice, p->stream));
    BCHK(p, hipStreamSynchronize(p->stream));           // the caller may reuse `bytes`
    p->hgz.insert(p->hgz.end(), (const uint8_t*)bytes, (const uint8_t*)bytes + n);
    return MKT_OK;
}

void mkt_bgzf_opts_default(mkt_bgzf_opts* o) { if (o) memset(o, 0, sizeof *o); }

int mkt_bgzf_run(mkt_bgzf* p, const mkt_bgzf_opts* opts, mkt_bgzf_info* info) {
    if (!p) return MKT_E_ARG;
    if (opts) for (uint32_t r : opts->reserved) if (r) return bfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    mkt_bgzf_info I;
    memset(&I, 0, sizeof I);
    if (info) *info = I;
    BCHK(p, hipSetDevice(p->device));
    p->ran = false; p->text_len = 0;
    p->text.reset();
    p->ms[0] = p->ms[1] = p->ms[2] = 0;
    p->have_query = false;
    p->qans.reset();
    if (!p->gz.get()) BCHK(p, p->gz.regrow(((size_t)1 << 20) + 64));
    const int rc = bz_inflate_file(p, p->hgz.data(), p->gz, p->hgz.size(), "the file", p->text, &p->text_len, &I, p->ms);
    if (info) *info = I;
    if (rc != MKT_OK) { p->text.reset(); return rc; }
    p->ran = true;
    return MKT_OK;
}

int mkt_bgzf_fetch_text(mkt_bgzf* p, uint64_t off, char* out, size_t n) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->ran) return bfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    if (off > p->text_len || n > p->text_len - off) return bfail(p, MKT_E_ARG, "range past the end of the text");
    BCHK(p, hipSetDevice(p->device));
    if (n) BCHK(p, hipMemcpy(out, p->text + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_bgzf_device_text(mkt_bgzf* p, const void** d_ptr, uint64_t* n) {
    if (!p || !d_ptr || !n) return MKT_E_ARG;
    if (!p->ran) return bfail(p, MKT_E_STATE, "device text before a run that succeeded");
    *d_ptr = p->text.get();
    *n = p->text_len;
    return MKT_OK;
}

// The .px2 is BGZF itself: inflated by the same kernel, its fields walked on the host (every byte accounted for, as tests/px2def.py
// parse_px2_raw does) and kept: names, bins, chunks and linear indexes (px2_parse of mkt_px2query.h).  The file that was added stays.
int mkt_bgzf_load_index(mkt_bgzf* p, const char* px2, size_t n) {
    if (!p || (n && !px2)) return MKT_E_ARG;
    BCHK(p, hipSetDevice(p->device));
    p->have_index = p->index_checked = p->have_query = false;
    p->qans.reset();
    DevBuf<uint8_t> dx, dtext;
    BCHK(p, dx.alloc(n, 64));
    if (n) BCHK(p, hipMemcpy(dx, px2, n, hipMemcpyHostToDevice));
    mkt_bgzf_info I;
    uint64_t len = 0;
    double ms[3] = {0, 0, 0};
    if (const int rc = bz_inflate_file(p, (const uint8_t*)px2, dx, n, "the index", dtext, &len, &I, ms)) return rc;
    if (!I.has_eof) return bfail(p, MKT_E_FORMAT, "the index: no EOF block");
    std::vector<uint8_t> d(len + 1);
    if (len) BCHK(p, hipMemcpy(d.data(), dtext, len, hipMemcpyDeviceToHost));
    std::string err;
    if (!px2_parse(d.data(), len, p->ix, err)) return bfail(p, MKT_E_FORMAT, "%s", err.c_str());
    BCHK(p, p->dnames.alloc(p->ix.names.size(), 64));
    if (!p->ix.names.empty()) BCHK(p, hipMemcpy(p->dnames, p->ix.names.data(), p->ix.names.size(), hipMemcpyHostToDevice));
    p->index_lines = p->ix.n_lines;
    p->have_index = true;
    return MKT_OK;
}
int mkt_bgzf_count(mkt_bgzf* p, uint64_t* n_lines) {
    if (!p || !n_lines) return MKT_E_ARG;
    if (!p->have_index) return bfail(p, MKT_E_STATE, "count before an index was loaded");
    *n_lines = p->index_lines;
    return MKT_OK;
}
int mkt_bgzf_timing(const mkt_bgzf* p, double ms[5]) {
    if (!p || !ms) return MKT_E_ARG;
    for (int k = 0; k < 5; ++k) ms[k] = p->ms[k];
    return MKT_OK;
}

// ---- region queries ------------------------------------------------------------------------------------------------------------------
static int bq_fail_member(mkt_bgzf* p, mkt_bgzf_query_info* I, uint32_t reason, uint64_t coff) {
    I->reason = reason; I->bad_offset = coff;
    return bfail(p, MKT_E_FORMAT, "the file: block at %llu: %s [%s]", (unsigned long long)coff, inf_reason_text(reason), inf_reason_key(reason));
}
static int bq_query(mkt_bgzf* p, const char* const* regions, uint32_t n, bool autoflip, mkt_bgzf_query_info* I) {
    hipStream_t st = p->stream;
    if (!p->have_blocks) {                                // the block table of the file as it stands, kept until the next add
        uint64_t bad = 0;
        bool has_eof = false;
        if (const uint32_t r = inf_block_table(p->hgz.data(), p->hgz.size(), p->blocks, &bad, &has_eof)) return bq_fail_member(p, I, r, bad);
        if (p->blocks.size() >= 0x7FFFFFFFull) return bfail(p, MKT_E_CAPACITY, "%llu blocks: a launch takes fewer than 2^31", (unsigned long long)p->blocks.size());
        BCHK(p, p->dblocks.alloc(p->blocks.size() + 1));
        if (!p->blocks.empty()) BCHK(p, hipMemcpyAsync(p->dblocks, p->blocks.data(), p->blocks.size() * sizeof(InfBlock), hipMemcpyHostToDevice, st));
        BCHK(p, hipStreamSynchronize(st));
        p->have_blocks = true;
    }
    if (!p->index_checked) {
        if (!q_index_belongs(p->ix, p->blocks, p->hgz.size())) return bfail(p, MKT_E_FORMAT, "the index does not belong to this file: a chunk points at no block of it");
        p->index_checked = true;
    }
    QPlan P;
    std::string err;
    if (const int rc = q_plan(p->ix, p->blocks, p->hgz.size(), regions, n, autoflip, P, err)) return bfail(p, rc == 1 ? MKT_E_ARG : MKT_E_FORMAT, "%s", err.c_str());
    const bool resident = p->ran;
    q_layout(P, p->blocks, resident);
    const uint64_t ns = P.spans.size(), nm = P.members.size();
    std::vector<uint64_t> cum(ns + 1, 0);
    for (uint64_t s = 0; s < ns; ++s) cum[s + 1] = cum[s] + (P.spans[s].hi - P.spans[s].lo);
    const uint64_t ntiles = (cum[ns] + kQTile - 1) / kQTile;
    if (ns >= 0x7FFFFFFFull || ntiles >= 0x7FFFFFFFull || n == 0xFFFFFFFFu) return bfail(p, MKT_E_CAPACITY, "%llu spans of %llu bytes: a launch takes fewer than 2^31 tiles", (unsigned long long)ns, (unsigned long long)cum[ns]);
    I->regions = n; I->subqueries = P.subs.size(); I->chunks = ns;
    I->blocks_inflated = nm; I->bytes_inflated = P.member_bytes;
    p->qoff.assign((size_t)n + 1, 0);
    p->qcnt.assign(n, 0);
    p->qans_len = 0;
    BCHK(p, p->qans.alloc(0, 64));
    BCHK(p, hipMemsetAsync(p->qans.get(), 0, 64, st));

    DevEvents<3> ev;
    BCHK(p, ev.create());
    BCHK(p, hipEventRecord(ev[0], st));
    // ---- the plan goes up; the members of the plan are inflated into the compact buffer and their CRC-32 checked
    DevBuf<uint8_t> compact;
    DevBuf<QSpan> dspans; DevBuf<QSub> dsubs; DevBuf<uint64_t> dcum, dfirst;
    BCHK(p, dspans.alloc(ns + 1)); BCHK(p, dsubs.alloc(P.subs.size() + 1)); BCHK(p, dcum.alloc(ns + 1)); BCHK(p, dfirst.alloc((size_t)n + 1));
    if (ns) BCHK(p, hipMemcpyAsync(dspans, P.spans.data(), ns * sizeof(QSpan), hipMemcpyHostToDevice, st));
    if (!P.subs.empty()) BCHK(p, hipMemcpyAsync(dsubs, P.subs.data(), P.subs.size() * sizeof(QSub), hipMemcpyHostToDevice, st));
    BCHK(p, hipMemcpyAsync(dcum, cum.data(), (ns + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    BCHK(p, hipMemcpyAsync(dfirst, P.region_first.data(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (nm) {
        DevBuf<uint32_t> dlist; DevBuf<uint64_t> dtbase; DevBuf<InfResult> dres;
        BCHK(p, compact.alloc(P.compact_bytes, 64));
        BCHK(p, hipMemsetAsync(compact.get(), 0, P.compact_bytes + 64, st));
        BCHK(p, dlist.alloc(nm)); BCHK(p, dtbase.alloc(nm)); BCHK(p, dres.alloc(nm));
        BCHK(p, hipMemcpyAsync(dlist, P.members.data(), nm * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        BCHK(p, hipMemcpyAsync(dtbase, P.tbase.data(), nm * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_inflate, dim3((unsigned)nm), dim3(kInfWave), 0, st, (const uint8_t*)p->gz.get(), (const InfBlock*)p->dblocks.get(), (const uint32_t*)dlist.get(), (const uint64_t*)dtbase.get(),
                           compact.get(), dres.get());
        BCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_inflate_crc, dim3((unsigned)nm), dim3(kCrcWg), 0, st, (const InfBlock*)p->dblocks.get(), (const uint32_t*)dlist.get(), (const uint64_t*)dtbase.get(), (const uint8_t*)compact.get(),
                           (const CrcTabs*)p->ct.get(), dres.get());
        BCHK(p, hipGetLastError());
        std::vector<InfResult> res(nm);
        BCHK(p, hipMemcpyAsync(res.data(), dres, nm * sizeof(InfResult), hipMemcpyDeviceToHost, st));
        BCHK(p, hipStreamSynchronize(st));                // the lists and the results end here
        for (uint64_t j = 0; j < nm; ++j) if (res[j].status) return bq_fail_member(p, I, res[j].status, p->blocks[P.members[j]].coff);
    }
    BCHK(p, hipEventRecord(ev[1], st));
    const uint8_t* text = resident ? p->text.get() : compact.get();
    // ---- line starts inside the spans, the filter, the scan of the matched lengths, the gather
    uint64_t ncand = 0, nblk = 0;
    std::vector<uint64_t> roff((size_t)n + 1, 0), rbefore((size_t)n + 1, 0);
    if (ns) {
        DevBuf<uint32_t> tile_cnt; DevBuf<uint64_t> tile_base;
        BCHK(p, tile_cnt.alloc(ntiles)); BCHK(p, tile_base.alloc(ntiles + 1));
        hipLaunchKernelGGL(k_query_count, dim3((unsigned)ntiles), dim3(SWG), 0, st, text, (const QSpan*)dspans.get(), (const uint64_t*)dcum.get(), (uint32_t)ns, tile_cnt.get());
        BCHK(p, hipGetLastError());
        QScanJobs J1 = {};
        J1.j[0] = QScanJob{tile_cnt.get(), tile_base.get(), ntiles};
        hipLaunchKernelGGL(k_query_scan, dim3(1), dim3(SWG), 0, st, J1);
        BCHK(p, hipGetLastError());
        BCHK(p, hipMemcpyAsync(&ncand, tile_base.get() + ntiles, sizeof ncand, hipMemcpyDeviceToHost, st));
        BCHK(p, hipStreamSynchronize(st));                // the number of candidate lines sizes what follows
        nblk = (ncand + SWG - 1) / SWG;
        if (nblk >= 0x7FFFFFFFull) return bfail(p, MKT_E_CAPACITY, "%llu candidate lines: a launch takes fewer than 2^31 blocks of them", (unsigned long long)ncand);
        DevBuf<uint64_t> cand_pos, span_first, base, rout;
        DevBuf<uint32_t> cand_u32, blk;
        BCHK(p, cand_pos.alloc(ncand)); BCHK(p, span_first.alloc(ns + 1)); BCHK(p, cand_u32.alloc(4 * ncand)); BCHK(p, blk.alloc(3 * nblk)); BCHK(p, base.alloc(3 * (nblk + 1)));
        BCHK(p, rout.alloc(2 * ((size_t)n + 1)));
        uint32_t* cand_span = cand_u32.get(); uint32_t* cand_len = cand_span + ncand; uint32_t* cand_off = cand_len + ncand; uint32_t* cand_before = cand_off + ncand;
        hipLaunchKernelGGL(k_query_lines, dim3((unsigned)ntiles), dim3(SWG), 0, st, text, (const QSpan*)dspans.get(), (const uint64_t*)dcum.get(), (uint32_t)ns, (const uint64_t*)tile_base.get(), ncand,
                           cand_pos.get(), cand_span, span_first.get());
        BCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_query_filter, dim3((unsigned)nblk), dim3(SWG), 0, st, text, (const QSpan*)dspans.get(), (const QSub*)dsubs.get(), (const uint8_t*)p->dnames.get(), ncand,
                           (const uint64_t*)cand_pos.get(), (const uint32_t*)cand_span, cand_len, cand_off, cand_before, blk.get(), blk.get() + nblk, blk.get() + 2 * nblk);
        BCHK(p, hipGetLastError());
        QScanJobs J2 = {};
        for (int k = 0; k < 3; ++k) J2.j[k] = QScanJob{blk.get() + k * nblk, base.get() + k * (nblk + 1), nblk};
        hipLaunchKernelGGL(k_query_scan, dim3(3), dim3(SWG), 0, st, J2);
        BCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_query_regions, dim3((unsigned)(((uint64_t)n + 1 + SWG - 1) / SWG)), dim3(SWG), 0, st, (const uint64_t*)dfirst.get(), n, (uint32_t)ns, (const uint64_t*)span_first.get(), ncand,
                           (const uint32_t*)cand_off, (const uint32_t*)cand_before, (const uint64_t*)base.get(), (const uint64_t*)(base.get() + (nblk + 1)), nblk, rout.get(), rout.get() + ((size_t)n + 1));
        BCHK(p, hipGetLastError());
        uint64_t totals[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) BCHK(p, hipMemcpyAsync(&totals[k], base.get() + k * (nblk + 1) + nblk, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BCHK(p, hipMemcpyAsync(roff.data(), rout.get(), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BCHK(p, hipMemcpyAsync(rbefore.data(), rout.get() + ((size_t)n + 1), ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        BCHK(p, hipStreamSynchronize(st));                // the size of the answer
        BCHK(p, p->qans.alloc(totals[0], 64));
        BCHK(p, hipMemsetAsync(p->qans.get() + totals[0], 0, 64, st));
        if (nblk) {
            hipLaunchKernelGGL(k_query_gather, dim3((unsigned)nblk), dim3(SWG), 0, st, text, ncand, (const uint64_t*)cand_pos.get(), (const uint32_t*)cand_len, (const uint32_t*)cand_off,
                               (const uint64_t*)base.get(), p->qans.get(), totals[0]);
            BCHK(p, hipGetLastError());
        }
        BCHK(p, hipEventRecord(ev[2], st));
        BCHK(p, hipStreamSynchronize(st));                // the candidate arrays end here
        p->qans_len = totals[0];
        I->lines = totals[1]; I->unparsed = totals[2];
    } else {
        BCHK(p, hipEventRecord(ev[2], st));
        BCHK(p, hipStreamSynchronize(st));
    }
    I->candidate_lines = ncand; I->answer_bytes = p->qans_len;
    for (uint32_t r = 0; r < n; ++r) { p->qoff[r] = roff[r]; p->qcnt[r] = rbefore[r + 1] - rbefore[r]; }
    p->qoff[n] = p->qans_len;
    for (int k = 0; k < 2; ++k) { float f = 0; BCHK(p, hipEventElapsedTime(&f, ev[k], ev[k + 1])); p->ms[3 + k] = f; }
    p->have_query = true;
    return MKT_OK;
}

int mkt_bgzf_query(mkt_bgzf* p, const char* const* regions, uint32_t n, const mkt_bgzf_query_opts* opts, mkt_bgzf_query_info* info) {
    if (!p || (n && !regions)) return MKT_E_ARG;
    if (opts) for (uint32_t r : opts->reserved) if (r) return bfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    if (opts && opts->autoflip > 1) return bfail(p, MKT_E_ARG, "autoflip is 0 or 1");
    mkt_bgzf_query_info I;
    memset(&I, 0, sizeof I);
    if (info) *info = I;
    p->have_query = false;
    p->qans.reset();
    p->ms[3] = p->ms[4] = 0;
    if (p->hgz.empty()) return bfail(p, MKT_E_STATE, "query before a file was added");
    if (!p->have_index) return bfail(p, MKT_E_STATE, "query before an index was loaded");
    BCHK(p, hipSetDevice(p->device));
    const int rc = bq_query(p, regions, n, opts && opts->autoflip, &I);
    if (info) *info = I;
    if (rc != MKT_OK) { p->have_query = false; p->qans.reset(); }
    return rc;
}
int mkt_bgzf_fetch_query(mkt_bgzf* p, uint64_t off, char* out, size_t n) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->have_query) return bfail(p, MKT_E_STATE, "fetch before a query that succeeded");
    if (off > p->qans_len || n > p->qans_len - off) return bfail(p, MKT_E_ARG, "range past the end of the answer");
    BCHK(p, hipSetDevice(p->device));
    if (n) BCHK(p, hipMemcpy(out, p->qans + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_bgzf_fetch_query_offsets(mkt_bgzf* p, uint64_t* out) {
    if (!p || !out) return MKT_E_ARG;
    if (!p->have_query) return bfail(p, MKT_E_STATE, "fetch before a query that succeeded");
    memcpy(out, p->qoff.data(), p->qoff.size() * sizeof(uint64_t));
    return MKT_OK;
}
int mkt_bgzf_fetch_query_counts(mkt_bgzf* p, uint64_t* out) {
    if (!p || (!out && !p->qcnt.empty())) return MKT_E_ARG;
    if (!p->have_query) return bfail(p, MKT_E_STATE, "fetch before a query that succeeded");
    if (!p->qcnt.empty()) memcpy(out, p->qcnt.data(), p->qcnt.size() * sizeof(uint64_t));
    return MKT_OK;
}
int mkt_bgzf_query_device(mkt_bgzf* p, const void** d_ptr, uint64_t* n) {
    if (!p || !d_ptr || !n) return MKT_E_ARG;
    if (!p->have_query) return bfail(p, MKT_E_STATE, "device answer before a query that succeeded");
    *d_ptr = p->qans.get();
    *n = p->qans_len;
    return MKT_OK;
}
int mkt_bgzf_clear(mkt_bgzf* p) {
    if (!p) return MKT_E_ARG;
    BCHK(p, hipSetDevice(p->device));
    BCHK(p, hipStreamSynchronize(p->stream));
    p->hgz.clear();                                     // (the device buffer of the compressed bytes keeps its room: nothing of it is read again)
    p->text.reset(); p->text_len = 0;
    p->ran = p->have_index = p->have_blocks = p->index_checked = p->have_query = false;
    p->index_lines = 0;
    p->ix = Px2Index();
    p->dnames.reset(); p->dblocks.reset(); p->qans.reset(); p->qans_len = 0;
    p->blocks.clear(); p->qoff.clear(); p->qcnt.clear();
    for (double& m : p->ms) m = 0;
    return MKT_OK;
}
int mkt_bgzf_names(mkt_bgzf* p, uint64_t off, char* out, size_t n, uint64_t* total) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->have_index) return bfail(p, MKT_E_STATE, "names before an index was loaded");
    const uint64_t len = p->ix.names.size();
    if (total) *total = len;
    if (off > len || n > len - off) return bfail(p, MKT_E_ARG, "range past the end of the name table");
    if (n) memcpy(out, p->ix.names.data() + off, n);
    return MKT_OK;
}

}  // extern "C"
