// mkt_inflate.hip -- BGZF (SAMv1 4.1) read back on the GPU: the inflate of RFC 1951 with one wavefront per BGZF block, the CRC-32 and
// ISIZE of every inflated block checked against its footer, and the reader object of include/mkt.h (mkt_bgzf_*).  DESIGN.md 6g has the
// layout and the arguments; mkt_inflate.h the functions that decide what is accepted (shared with the host driver).
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
#include "mkt_inflate.h"

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
// parse_px2_raw does).  Only the line count is kept: region queries are not part of this library yet.
int mkt_bgzf_load_index(mkt_bgzf* p, const char* px2, size_t n) {
    if (!p || (n && !px2)) return MKT_E_ARG;
    BCHK(p, hipSetDevice(p->device));
    p->have_index = false;
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
    auto rd32 = [&](uint64_t at) { return (uint32_t)d[at] | (uint32_t)d[at + 1] << 8 | (uint32_t)d[at + 2] << 16 | (uint32_t)d[at + 3] << 24; };
    if (len < 64 || memcmp(d.data(), "PX2.004\1", 8)) return bfail(p, MKT_E_FORMAT, "the index: not a PX2.004 file");
    const uint64_t n_ref = rd32(8), l_nm = rd32(60);
    const uint64_t n_lines = (uint64_t)rd32(12) | (uint64_t)rd32(16) << 32;
    if (n_ref > 0x7FFFFFFFull || l_nm > len - 64) return bfail(p, MKT_E_FORMAT, "the index: the name table runs past its end");
    uint64_t at = 64, names = 0;
    for (uint64_t k = 0; k < l_nm; ++k) names += d[at + k] == 0;
    if (names != n_ref || (l_nm && d[at + l_nm - 1] != 0)) return bfail(p, MKT_E_FORMAT, "the index: %llu names for n_ref %llu", (unsigned long long)names, (unsigned long long)n_ref);
    at += l_nm;
    for (uint64_t r = 0; r < n_ref; ++r) {
        if (len - at < 4) return bfail(p, MKT_E_FORMAT, "the index ends inside name %llu", (unsigned long long)r);
        const uint64_t n_bin = rd32(at);
        at += 4;
        for (uint64_t k = 0; k < n_bin; ++k) {
            if (len - at < 8) return bfail(p, MKT_E_FORMAT, "the index ends inside name %llu", (unsigned long long)r);
            const uint64_t n_chunk = rd32(at + 4);
            at += 8;
            if (n_chunk > (len - at) / 16) return bfail(p, MKT_E_FORMAT, "the index ends inside name %llu", (unsigned long long)r);
            at += 16 * n_chunk;
        }
        if (len - at < 4) return bfail(p, MKT_E_FORMAT, "the index ends inside name %llu", (unsigned long long)r);
        const uint64_t n_intv = rd32(at);
        at += 4;
        if (n_intv > (len - at) / 8) return bfail(p, MKT_E_FORMAT, "the index ends inside name %llu", (unsigned long long)r);
        at += 8 * n_intv;
    }
    if (at != len) return bfail(p, MKT_E_FORMAT, "the index: %llu bytes behind the last linear index", (unsigned long long)(len - at));
    p->index_lines = n_lines;
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

}  // extern "C"
