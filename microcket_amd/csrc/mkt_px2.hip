// mkt_px2.hip -- final.pairs.gz (BGZF) and its pairix index final.pairs.gz.px2 from a sorted .pairs text on the GPU: the reference
// driver's `bgzip -c final.pairs > final.pairs.gz; pairix final.pairs.gz`.  include/mkt.h has the definition, DESIGN.md 6f the why.
//
// The text stays on the device.  It is compressed with the BGZF framing of mkt_deflate.hip; the scan of the block sizes gives the
// file offset of every block, which is all a virtual offset needs: the block of a text offset is offset / BGZF_RAW.  One thread per
// line then parses columns 2 to 4 of its line AND of the record before it (through the line index: no halo, no workgroup edge),
// and says whether the pair (chr1, chr2) changes there, whether the window pos1 falls in changes there, and whether the line
// is refused.  Scans of the two flags number the names and the chunks.  Because a file is only accepted when pos1 never goes back inside
// a pair and no pair reappears, every (name, bin) is ONE chunk and the chunks already stand in the order of the file's index:
// nothing is sorted and nothing is merged.  The linear index of a name is the begin of the chunk of each window, an empty window
// repeating the one before it; a thread per window finds its chunk by bisection.  The index is serialised on the device and
// compressed by the same BGZF path.  Integers only and no atomics: the same bytes on every call.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_blockscan.h"
#include "mkt_deflate.h"
#include "mkt_launch.h"
#include "mkt_px2.h"
#include "mkt_sortlib.h"

using namespace mkt;

namespace mkt {

constexpr uint64_t kPxNoBad = ~0ull;

// columns 2 to 4 of a record: [c1, c1e) chr1, pos1, [c2, c2e) chr2 (offsets into the text)
struct PxRec { uint64_t c1, c1e, c2, c2e; uint32_t pos; };

__device__ inline bool px_is_meta(const uint8_t* text, uint64_t ls, uint64_t le) { return le > ls && text[ls] == '#'; }

// Parses text[ls, le) (le: the line's newline, never read past).  -1: a record; else why it is refused.
__device__ inline int px_parse(const uint8_t* text, uint64_t ls, uint64_t le, PxRec& r) {
    uint64_t tab[4];
    int nt = 0;
    for (uint64_t p = ls; p < le; ++p)
        if (text[p] == '\t') { tab[nt++] = p; if (nt == 4) break; }
    if (nt < 4) return PX_BAD_COLUMNS;                  // fewer than five columns
    r.c1 = tab[0] + 1; r.c1e = tab[1];
    r.c2 = tab[2] + 1; r.c2e = tab[3];
    const uint64_t a = tab[1] + 1, b = tab[2];
    if (b == a || b - a > 10) return PX_BAD_POS;
    uint64_t v = 0;
    for (uint64_t q = a; q < b; ++q) {
        const uint32_t d = (uint32_t)text[q] - (uint32_t)'0';
        if (d > 9u) return PX_BAD_POS;
        v = v * 10 + d;
    }
    if (v > kPxPosMax) return PX_BAD_POS;
    r.pos = (uint32_t)v;
    return -1;
}
__device__ inline bool px_bytes_eq(const uint8_t* text, uint64_t a, uint64_t ae, uint64_t b, uint64_t be) {
    if (ae - a != be - b) return false;
    for (uint64_t k = 0; k < ae - a; ++k) if (text[a + k] != text[b + k]) return false;
    return true;
}

// One thread per line.  fa[j]: 1 where a chunk begins (the name or the window differs from the record before), + 2^32 for every record;
// fb[j]: 1 where a name begins; win[j]: the window of a record.  wgbad[workgroup]: the smallest (line << 2 | reason) it refuses.
// The record before line j is the nearest line in front of it that does not begin with '#'.
__global__ __launch_bounds__(SWG) void k_px_lines(const uint8_t* text, const uint64_t* starts, uint64_t nl, uint64_t* fa, uint64_t* fb, uint32_t* win, uint64_t* wgbad) {
    __shared__ uint64_t sh[SWG];
    const uint64_t j = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    uint64_t bad = kPxNoBad;
    if (j < nl) {
        const uint64_t ls = starts[j], le = starts[j + 1] - 1;
        uint64_t a = 0, b = 0;
        uint32_t w = 0;
        if (!px_is_meta(text, ls, le)) {
            PxRec r;
            const int why = px_parse(text, ls, le, r);
            if (why >= 0) bad = j << 2 | (uint64_t)why;
            else {
                w = px_window(r.pos);
                bool same_name = false, same_win = false;
                for (uint64_t k = j; k-- > 0;) {
                    const uint64_t ps = starts[k], pe = starts[k + 1] - 1;
                    if (px_is_meta(text, ps, pe)) continue;
                    PxRec q;
                    if (px_parse(text, ps, pe, q) < 0) {              // a refused line in front: its own thread reports it
                        same_name = px_bytes_eq(text, r.c1, r.c1e, q.c1, q.c1e) && px_bytes_eq(text, r.c2, r.c2e, q.c2, q.c2e);
                        if (same_name && r.pos < q.pos) bad = j << 2 | PX_BAD_ORDER;
                        same_win = same_name && px_window(q.pos) == w;
                    }
                    break;
                }
                a = (1ull << 32) | (same_win ? 0u : 1u);
                b = same_name ? 0u : 1u;
            }
        }
        fa[j] = a; fb[j] = b; win[j] = w;
    }
    sh[threadIdx.x] = bad;
    __syncthreads();
    for (uint32_t s = SWG / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s && sh[threadIdx.x + s] < sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) wgbad[blockIdx.x] = sh[0];
}
// the minimum of v[0, n) by one workgroup
__global__ __launch_bounds__(SWG) void k_px_min(const uint64_t* v, uint64_t n, uint64_t* out) {
    __shared__ uint64_t sh[SWG];
    uint64_t m = kPxNoBad;
    for (uint64_t k = threadIdx.x; k < n; k += SWG) if (v[k] < m) m = v[k];
    sh[threadIdx.x] = m;
    __syncthreads();
    for (uint32_t s = SWG / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s && sh[threadIdx.x + s] < sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// fa, fb: scanned (entry nl holds the totals).  The line of every chunk and of every name, the name of every chunk, the first chunk of every name.
__global__ __launch_bounds__(SWG) void k_px_heads(uint64_t nl, const uint64_t* fa, const uint64_t* fb, uint32_t* chunk_line, uint32_t* chunk_name, uint32_t* name_line,
                                                  uint32_t* name_chunk0) {
    const uint64_t j = (uint64_t)blockIdx.x * SWG + threadIdx.x;
    if (j >= nl) return;
    const uint32_t c = (uint32_t)fa[j], cf = (uint32_t)fa[j + 1] - c;
    const uint64_t nm = fb[j], nf = fb[j + 1] - nm;
    if (cf) { chunk_line[c] = (uint32_t)j; chunk_name[c] = (uint32_t)(nm + nf - 1); }
    if (nf) { name_line[nm] = (uint32_t)j; name_chunk0[nm] = c; }
    if (j == 0) name_chunk0[fb[nl]] = (uint32_t)fa[nl];
}

// per name: the bytes of "chr1|chr2\0" (0 for a line that does not parse: only lines behind a refused one), of its part of the index, and its windows
__global__ void k_px_name_sizes(uint64_t nnames, const uint8_t* text, const uint64_t* starts, const uint32_t* name_line, const uint32_t* name_chunk0, const uint32_t* chunk_line,
                                const uint32_t* win, uint64_t* nlen, uint64_t* size, uint64_t* slots) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnames) return;
    const uint64_t j = name_line[k];
    PxRec r;
    nlen[k] = px_parse(text, starts[j], starts[j + 1] - 1, r) < 0 ? (r.c1e - r.c1) + 1 + (r.c2e - r.c2) + 1 : 0;
    const uint64_t nb = name_chunk0[k + 1] - name_chunk0[k];
    const uint64_t ni = (uint64_t)win[chunk_line[name_chunk0[k + 1] - 1]] + 1;
    size[k] = 4 + 24 * nb + 4 + 8 * ni;
    slots[k] = ni;
}
__global__ void k_px_name_put(uint64_t nnames, const uint8_t* text, const uint64_t* starts, const uint32_t* name_line, const uint64_t* noff, uint8_t* names) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nnames || noff[k + 1] == noff[k]) return;
    const uint64_t j = name_line[k];
    PxRec r;
    (void)px_parse(text, starts[j], starts[j + 1] - 1, r);
    uint8_t* o = names + noff[k];
    for (uint64_t q = r.c1; q < r.c1e; ++q) *o++ = text[q];
    *o++ = '|';
    for (uint64_t q = r.c2; q < r.c2e; ++q) *o++ = text[q];
    *o = 0;
}

// where a reader stands that has consumed text[0, u): in the block that holds byte u; at the end of the text, at the EOF block
struct PxVoff {
    const uint64_t* coff; uint64_t n, nblocks;
    __device__ uint64_t operator()(uint64_t u) const {
        if (u >= n) return coff[nblocks] << 16;
        const uint64_t b = u / BGZF_RAW;
        return coff[b] << 16 | (u - b * BGZF_RAW);
    }
};
__device__ inline void px_store32(uint8_t* o, uint32_t v) { for (int k = 0; k < 4; ++k) o[k] = (uint8_t)(v >> (8 * k)); }
__device__ inline void px_store64(uint8_t* o, uint64_t v) { for (int k = 0; k < 8; ++k) o[k] = (uint8_t)(v >> (8 * k)); }

// One thread per chunk: its bin entry {bin, 1, beg, end}; the first chunk of a name also writes n_bin and n_intv.  body: the index behind the name table.
__global__ void k_px_bins(uint64_t nchunks, PxVoff V, const uint64_t* starts, const uint32_t* chunk_line, const uint32_t* chunk_name, const uint32_t* name_chunk0,
                          const uint32_t* win, const uint64_t* size_off, const uint64_t* slot_off, uint64_t* chunk_beg, uint8_t* body) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    const uint32_t k = chunk_name[c], c0 = name_chunk0[k], nb = name_chunk0[k + 1] - c0;
    uint8_t* base = body + size_off[k];
    if (c == c0) {
        px_store32(base, nb);
        px_store32(base + 4 + 24ull * nb, (uint32_t)(slot_off[k + 1] - slot_off[k]));
    }
    const uint64_t beg = V(starts[chunk_line[c]]), end = c + 1 < nchunks ? V(starts[chunk_line[c + 1]]) : V(V.n);
    uint8_t* e = base + 4 + 24ull * (c - c0);
    px_store32(e, kPxBinFirst + win[chunk_line[c]]);
    px_store32(e + 4, 1);
    px_store64(e + 8, beg);
    px_store64(e + 16, end);
    chunk_beg[c] = beg;
}
// One thread per window of every name: the begin of the last chunk of the name whose window is not behind it; 0 in front of the first.
__global__ void k_px_linear(uint64_t nslots, uint64_t nnames, const uint64_t* slot_off, const uint64_t* size_off, const uint32_t* name_chunk0, const uint32_t* chunk_line,
                            const uint32_t* win, const uint64_t* chunk_beg, uint8_t* body) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    uint64_t lo = 0, hi = nnames;                         // the name k with slot_off[k] <= s < slot_off[k + 1]
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) / 2; if (slot_off[mid] <= s) lo = mid; else hi = mid; }
    const uint64_t k = lo, w = s - slot_off[k];
    const uint32_t c0 = name_chunk0[k], c1 = name_chunk0[k + 1];
    uint32_t a = c0, b = c1;                              // the first chunk in [c0, c1) whose window is behind w
    while (a < b) { const uint32_t mid = a + (b - a) / 2; if (win[chunk_line[mid]] <= w) a = mid + 1; else b = mid; }
    const uint64_t v = a > c0 ? chunk_beg[a - 1] : 0;
    px_store64(body + size_off[k] + 4 + 24ull * (c1 - c0) + 4 + 8 * w, v);
}

}  // namespace mkt

// ---------------------------------------------------------------------------------------------------------------------------------
struct mkt_pairsgz {
    int device = 0;
    DevStream stream;                                   // declared first: destroyed after every buffer
    GrowBuf<uint8_t> text; size_t len = 0;              // the text as it was added
    DevBuf<CrcTabs> ct;
    DevBuf<uint8_t> gz, px2; uint64_t gz_len = 0, px2_len = 0;
    bool ran = false;
    double ms[5] = {0, 0, 0, 0, 0};
    std::string err;
};
static int xfail(mkt_pairsgz* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p) p->err = buf;
    return code;
}
#define XCHK(p, call) do { hipError_t e_ = (call); if (e_ == hipErrorOutOfMemory) { (void)hipGetLastError(); return xfail((p), MKT_E_NOMEM, "%s: the device memory does not suffice (the text, its compressed blocks and 28 bytes per line are resident)", #call); } \
                           if (e_ != hipSuccess) return xfail((p), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// raw[0, n) (readable 64 bytes past n) -> a BGZF file with its EOF block in `out`; coff (nblocks + 1 entries) keeps the file offsets of the blocks
static int px_bgzf(mkt_pairsgz* p, const uint8_t* raw, uint64_t n, int level, DevBuf<uint64_t>& coff, uint64_t* nblocks_out, DevBuf<uint8_t>& out, uint64_t* out_len) {
    hipStream_t st = p->stream;
    const uint64_t nblocks = (n + BGZF_RAW - 1) / BGZF_RAW;
    uint64_t clen = 0;
    XCHK(p, coff.alloc(nblocks + 2));
    XCHK(p, hipMemsetAsync(coff, 0, (nblocks + 2) * sizeof(uint64_t), st));
    DevBuf<uint8_t> comp;
    if (nblocks) {
        DevBuf<uint32_t> scratch;
        XCHK(p, comp.alloc(nblocks * (uint64_t)BGZF_STRIDE, 64));
        uint64_t batch = ((uint64_t)8 << 30) / deflate_scratch_bytes(1);
        if (batch > nblocks) batch = nblocks;
        if (batch < 1) batch = 1;
        if (level > 0) XCHK(p, scratch.alloc(0, deflate_scratch_bytes(batch) + 64));
        XCHK(p, bgzf_launch(raw, n, nblocks, level, p->ct, comp, coff, scratch, batch, st));
        XCHK(p, launch_exscan(coff, nblocks, coff + nblocks, st));
        XCHK(p, hipMemcpyAsync(&clen, coff + nblocks, sizeof clen, hipMemcpyDeviceToHost, st));
        XCHK(p, hipStreamSynchronize(st));              // clen; the scratch ends here
    }
    XCHK(p, out.alloc(clen + 28, 64));
    if (nblocks) XCHK(p, bgzf_pack(comp, coff, nblocks, out, st));
    XCHK(p, hipMemcpyAsync(out + clen, kBgzfEof, 28, hipMemcpyHostToDevice, st));
    XCHK(p, hipStreamSynchronize(st));
    *nblocks_out = nblocks;
    *out_len = clen + 28;
    return MKT_OK;
}

extern "C" {

int mkt_pairsgz_create(int device, mkt_pairsgz** out) {
    if (!out) return MKT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MKT_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return MKT_E_ARG;
    mkt_pairsgz* p = new mkt_pairsgz();
    p->device = device;
    CrcTabs ct;
    crc_tables(&ct);
    if (hipSetDevice(device) != hipSuccess || p->stream.create(hipStreamNonBlocking) != hipSuccess || p->ct.alloc(1) != hipSuccess ||
        hipMemcpy(p->ct, &ct, sizeof ct, hipMemcpyHostToDevice) != hipSuccess) { mkt_pairsgz_destroy(p); return MKT_E_HIP; }
    *out = p;
    return MKT_OK;
}
void mkt_pairsgz_destroy(mkt_pairsgz* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;                                           // the buffers, then the stream
}
const char* mkt_pairsgz_error(const mkt_pairsgz* p) { return p ? p->err.c_str() : ""; }

int mkt_pairsgz_add(mkt_pairsgz* p, const char* bytes, size_t n) {
    if (!p || (n && !bytes)) return MKT_E_ARG;
    XCHK(p, hipSetDevice(p->device));
    const size_t need = p->len + n + 1;                 // + the newline that stands in for a missing last one
    if (!p->text.fits(need + 64)) {
        size_t ncap = p->text.cap() ? p->text.cap() - 64 : ((size_t)1 << 20);
        while (ncap < need) ncap *= 2;
        XCHK(p, p->text.regrow_keep(ncap + 64, p->len));
    }
    if (n) XCHK(p, hipMemcpyAsync(p->text + p->len, bytes, n, hipMemcpyHostToDevice, p->stream));
    XCHK(p, hipStreamSynchronize(p->stream));           // the caller may reuse `bytes`
    p->len += n;
    p->ran = false;
    return MKT_OK;
}

void mkt_pairsgz_opts_default(mkt_pairsgz_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->level = 1; o->preset = MKT_PAIRSGZ_PRESET_PAIRS;
}

int mkt_pairsgz_run(mkt_pairsgz* p, const mkt_pairsgz_opts* opts, mkt_pairsgz_info* info) {
    if (!p) return MKT_E_ARG;
    mkt_pairsgz_opts o;
    mkt_pairsgz_opts_default(&o);
    if (opts) o = *opts;
    if (o.level < 0 || o.level > 2) return xfail(p, MKT_E_ARG, "level %d: 0 (stored), 1 (the fixed code) or 2 (a code per block)", o.level);
    if (o.preset != MKT_PAIRSGZ_PRESET_PAIRS) return xfail(p, MKT_E_ARG, "preset %u: only the 4DN pairs preset (columns 2, 3 and 4, 5) is offered", o.preset);
    for (uint32_t r : o.reserved) if (r) return xfail(p, MKT_E_ARG, "a reserved word of the options is not 0");
    mkt_pairsgz_info I;
    memset(&I, 0, sizeof I);
    if (info) *info = I;
    XCHK(p, hipSetDevice(p->device));
    p->ran = false; p->gz_len = p->px2_len = 0;
    p->gz.reset(); p->px2.reset();
    for (double& m : p->ms) m = 0;
    hipStream_t st = p->stream;
    const uint64_t n = p->len;
    if (!p->text.get()) XCHK(p, p->text.regrow(((size_t)1 << 20) + 64));
    uint8_t* text = p->text;
    // the line index wants a newline at the end: one stands behind the text where the last line has none (it is not compressed)
    char last = '\n';
    if (n) XCHK(p, hipMemcpy(&last, text + n - 1, 1, hipMemcpyDeviceToHost));
    const uint64_t n_ix = n + (last != '\n' ? 1 : 0);
    XCHK(p, hipMemsetAsync(text + n, 0, 64, st));
    if (n_ix > n) XCHK(p, hipMemsetAsync(text + n, '\n', 1, st));
    DevEvents<6> ev;
    XCHK(p, ev.create());
    XCHK(p, hipEventRecord(ev[0], st));

    // ---- the .gz
    DevBuf<uint64_t> coff;
    uint64_t nblocks = 0;
    if (int rc = px_bgzf(p, text, n, o.level, coff, &nblocks, p->gz, &p->gz_len)) return rc;
    XCHK(p, hipEventRecord(ev[1], st));

    // ---- lines
    LineIndex ix;
    uint64_t nl = 0;
    if (n_ix) { XCHK(p, ix.count(text, n_ix, st)); nl = ix.nlines; }
    if (nl >= (1ull << 32) - 1) return xfail(p, MKT_E_CAPACITY, "%llu lines: lines are indexed with 32 bits", (unsigned long long)nl);
    uint64_t nrec = 0, nchunks = 0, nnames = 0, l_nm = 0, body_len = 0, nslots = 0;
    DevBuf<uint64_t> fa, fb, wgbad, nsz, chunk_beg;
    DevBuf<uint32_t> win, chunk_line, chunk_name, name_line, name_chunk0;
    DevBuf<uint8_t> names;
    uint64_t *noff = nullptr, *size_off = nullptr, *slot_off = nullptr;
    if (nl) {
        XCHK(p, ix.fill(text, n_ix, st));
        XCHK(p, hipEventRecord(ev[2], st));
        const uint64_t* starts = ix.starts;
        const unsigned lgrid = (unsigned)((nl + SWG - 1) / SWG);
        XCHK(p, fa.alloc(nl + 1));
        XCHK(p, fb.alloc(nl + 1));
        XCHK(p, win.alloc(nl));
        XCHK(p, wgbad.alloc(lgrid + 1));
        hipLaunchKernelGGL(k_px_lines, dim3(lgrid), dim3(SWG), 0, st, (const uint8_t*)text, starts, nl, fa.get(), fb.get(), win.get(), wgbad.get());
        XCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_px_min, dim3(1), dim3(SWG), 0, st, (const uint64_t*)wgbad.get(), (uint64_t)lgrid, wgbad + lgrid);
        XCHK(p, hipGetLastError());
        XCHK(p, hipEventRecord(ev[3], st));
        // ---- names and chunks
        XCHK(p, launch_exscan(fa, nl, fa + nl, st));
        XCHK(p, launch_exscan(fb, nl, fb + nl, st));
        uint64_t bad = kPxNoBad, ta = 0;
        XCHK(p, hipMemcpyAsync(&bad, wgbad + lgrid, sizeof bad, hipMemcpyDeviceToHost, st));
        XCHK(p, hipMemcpyAsync(&ta, fa + nl, sizeof ta, hipMemcpyDeviceToHost, st));
        XCHK(p, hipMemcpyAsync(&nnames, fb + nl, sizeof nnames, hipMemcpyDeviceToHost, st));
        XCHK(p, hipStreamSynchronize(st));
        nrec = ta >> 32; nchunks = ta & 0xFFFFFFFFull;
        if (nchunks) {
            XCHK(p, chunk_line.alloc(nchunks));
            XCHK(p, chunk_name.alloc(nchunks));
            XCHK(p, name_line.alloc(nnames));
            XCHK(p, name_chunk0.alloc(nnames + 1));
            XCHK(p, nsz.alloc(3 * (nnames + 1)));
            noff = nsz; size_off = nsz + (nnames + 1); slot_off = nsz + 2 * (nnames + 1);
            hipLaunchKernelGGL(k_px_heads, dim3(lgrid), dim3(SWG), 0, st, nl, (const uint64_t*)fa.get(), (const uint64_t*)fb.get(), chunk_line.get(), chunk_name.get(), name_line.get(),
                               name_chunk0.get());
            XCHK(p, hipGetLastError());
            const unsigned ngrid = (unsigned)((nnames + 255) / 256);
            hipLaunchKernelGGL(k_px_name_sizes, dim3(ngrid), dim3(256), 0, st, nnames, (const uint8_t*)text, starts, (const uint32_t*)name_line.get(), (const uint32_t*)name_chunk0.get(),
                               (const uint32_t*)chunk_line.get(), (const uint32_t*)win.get(), noff, size_off, slot_off);
            XCHK(p, hipGetLastError());
            XCHK(p, launch_exscan(noff, nnames, noff + nnames, st));
            XCHK(p, launch_exscan(size_off, nnames, size_off + nnames, st));
            XCHK(p, launch_exscan(slot_off, nnames, slot_off + nnames, st));
            XCHK(p, hipMemcpyAsync(&l_nm, noff + nnames, sizeof l_nm, hipMemcpyDeviceToHost, st));
            XCHK(p, hipMemcpyAsync(&body_len, size_off + nnames, sizeof body_len, hipMemcpyDeviceToHost, st));
            XCHK(p, hipMemcpyAsync(&nslots, slot_off + nnames, sizeof nslots, hipMemcpyDeviceToHost, st));
            XCHK(p, hipStreamSynchronize(st));
            if (l_nm >= 0x7FFFFFFFull) return xfail(p, MKT_E_CAPACITY, "the names of the %llu pairs take %llu bytes: the index counts them with 31 bits", (unsigned long long)nnames, (unsigned long long)l_nm);
            XCHK(p, names.alloc(l_nm + 1));
            hipLaunchKernelGGL(k_px_name_put, dim3(ngrid), dim3(256), 0, st, nnames, (const uint8_t*)text, starts, (const uint32_t*)name_line.get(), (const uint64_t*)noff, names.get());
            XCHK(p, hipGetLastError());
            // the host's share: does a pair reappear?  Only the first line of every run comes over.
            std::vector<char> hnames(l_nm + 1);
            std::vector<uint32_t> hline(nnames);
            XCHK(p, hipMemcpyAsync(hnames.data(), names, l_nm, hipMemcpyDeviceToHost, st));
            XCHK(p, hipMemcpyAsync(hline.data(), name_line, nnames * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            XCHK(p, hipStreamSynchronize(st));
            uint64_t ncheck = nnames;                   // the names in front of the first refused line
            if (bad != kPxNoBad) { ncheck = 0; while (ncheck < nnames && hline[ncheck] < (bad >> 2)) ++ncheck; }
            size_t lcheck = 0;
            for (uint64_t k = 0, at = 0; k < ncheck; ++k) { at += strlen(hnames.data() + at) + 1; lcheck = at; }
            const int64_t re = px_first_reappearing(hnames.data(), lcheck, ncheck);
            if (re != kPxNoName) {
                const size_t at = [&] { size_t a = 0; for (int64_t k = 0; k < re; ++k) a += strlen(hnames.data() + a) + 1; return a; }();
                return xfail(p, MKT_E_ARG, "line %llu: the pair %s reappears: its lines are not contiguous (is the file sorted?)", (unsigned long long)hline[re] + 1, hnames.data() + at);
            }
        }
        if (bad != kPxNoBad) {
            static const char* const why[4] = {"fewer than five columns", "pos1 is not a decimal number below 2^31", "pos1 goes backwards inside its pair (is the file sorted?)", ""};
            return xfail(p, MKT_E_ARG, "line %llu: %s", (unsigned long long)(bad >> 2) + 1, why[bad & 3]);
        }
    } else {
        XCHK(p, hipEventRecord(ev[2], st));
        XCHK(p, hipEventRecord(ev[3], st));
    }
    XCHK(p, hipEventRecord(ev[4], st));

    // ---- the index: head and names, then per name its bins and its linear index
    const std::string head = px_head((uint32_t)nnames, nl, (uint32_t)l_nm);
    const uint64_t raw_len = kPxHeadBytes + l_nm + body_len;
    DevBuf<uint8_t> raw;
    XCHK(p, raw.alloc(raw_len, 64));
    XCHK(p, hipMemsetAsync(raw + raw_len, 0, 64, st));
    XCHK(p, hipMemcpyAsync(raw, head.data(), kPxHeadBytes, hipMemcpyHostToDevice, st));
    if (nchunks) {
        XCHK(p, hipMemcpyAsync(raw + kPxHeadBytes, names, l_nm, hipMemcpyDeviceToDevice, st));
        XCHK(p, chunk_beg.alloc(nchunks));
        uint8_t* body = raw + kPxHeadBytes + l_nm;
        const PxVoff V = {coff.get(), n, nblocks};
        hipLaunchKernelGGL(k_px_bins, dim3((unsigned)((nchunks + 255) / 256)), dim3(256), 0, st, nchunks, V, (const uint64_t*)ix.starts.get(), (const uint32_t*)chunk_line.get(),
                           (const uint32_t*)chunk_name.get(), (const uint32_t*)name_chunk0.get(), (const uint32_t*)win.get(), (const uint64_t*)size_off, (const uint64_t*)slot_off,
                           chunk_beg.get(), body);
        XCHK(p, hipGetLastError());
        hipLaunchKernelGGL(k_px_linear, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, st, nslots, nnames, (const uint64_t*)slot_off, (const uint64_t*)size_off,
                           (const uint32_t*)name_chunk0.get(), (const uint32_t*)chunk_line.get(), (const uint32_t*)win.get(), (const uint64_t*)chunk_beg.get(), body);
        XCHK(p, hipGetLastError());
    }
    DevBuf<uint64_t> xoff;
    uint64_t xblocks = 0;
    if (int rc = px_bgzf(p, raw, raw_len, o.level, xoff, &xblocks, p->px2, &p->px2_len)) return rc;
    XCHK(p, hipEventRecord(ev[5], st));
    XCHK(p, hipStreamSynchronize(st));
    for (int k = 0; k < 5; ++k) { float f = 0; XCHK(p, hipEventElapsedTime(&f, ev[k], ev[k + 1])); p->ms[k] = f; }
    I.lines = nl; I.records = nrec; I.names = nnames; I.bins = nchunks; I.chunks = nchunks; I.blocks = nblocks;
    I.gz_bytes = p->gz_len; I.px2_bytes = p->px2_len;
    p->ran = true;
    if (info) *info = I;
    return MKT_OK;
}

static int px_fetch(mkt_pairsgz* p, const DevBuf<uint8_t>& src, uint64_t have, uint64_t off, char* out, size_t n) {
    if (!p || (n && !out)) return MKT_E_ARG;
    if (!p->ran) return xfail(p, MKT_E_STATE, "fetch before a run that succeeded");
    if (off > have || n > have - off) return xfail(p, MKT_E_ARG, "range past the end of the file");
    XCHK(p, hipSetDevice(p->device));
    if (n) XCHK(p, hipMemcpy(out, src + off, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}
int mkt_pairsgz_fetch_gz(mkt_pairsgz* p, uint64_t off, char* out, size_t n) { return p ? px_fetch(p, p->gz, p->gz_len, off, out, n) : MKT_E_ARG; }
int mkt_pairsgz_fetch_px2(mkt_pairsgz* p, uint64_t off, char* out, size_t n) { return p ? px_fetch(p, p->px2, p->px2_len, off, out, n) : MKT_E_ARG; }
int mkt_pairsgz_timing(const mkt_pairsgz* p, double ms[5]) {
    if (!p || !ms) return MKT_E_ARG;
    for (int k = 0; k < 5; ++k) ms[k] = p->ms[k];
    return MKT_OK;
}

}  // extern "C"
