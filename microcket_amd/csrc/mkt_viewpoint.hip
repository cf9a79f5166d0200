// mkt_viewpoint.hip -- viewpoint contact profiles (a virtual 4C) over the resident pair records of a matrix object: the contacts between
// one chromosome (the viewpoint) and a set of partner chromosomes, the two sides binned at different sizes.  include/mkt.h has the
// definition, mkt_viewpoint.h the host half (hotspot cut, string order, texts); the entry points (mkt_matrix_viewpoint,
// mkt_matrix_fetch_viewpoint_*) are at the end, on the object of mkt_matrix_obj.h.
//
// The hot path is a streaming pass over the n 16-byte records, made twice: one 16-byte vector load per lane, the roles of the two
// chromosomes from a byte table staged in LDS once per workgroup, the two bin indices by one integer division each.
//  * k_vp_scan<false> counts the matching pairs (wave ballot, popcount, one integer add per wave at the end of the walk) and builds the
//    two tracks: dense uint32 histograms with integer atomics.  The viewpoint track is privatised in LDS per workgroup while its bins
//    fit kVpLdsBins and goes to global atomics otherwise; the partner track is always global (its bins are spread over the genome).
//  * k_vp_scan<true> emits one 64-bit key  viewpoint bin << B | global partner bin  per matching pair into a buffer of exactly the
//    counted size: a wave claims its slots with one atomic on a cursor and the lanes take theirs by the popcount prefix of the ballot.
//    The order of the keys in the buffer is not fixed; the sort fixes the result.
// The keys are sorted by the duplicate marker's radix passes (launch_radix64) over the B + Bv significant bits and reduced by the
// run-length passes of the binning (rle_reduce, mkt_rle.h): the link table.  The non-empty cells of the partner track are compacted on
// the device (k_vp_compact) and ordered on the host.  Integers only: no floating point on the device, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <stdarg.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "mkt_launch.h"
#include "mkt_matrix_obj.h"
#include "mkt_rle.h"
#include "mkt_segred.h"

namespace mkt {

constexpr int VP_WG = 256;
constexpr uint32_t VP_MAX_GRID = 2048;            // workgroups of the scan: 8 per CU on 256 CUs, each walks the records with the grid's stride
constexpr uint32_t VP_CHR = 8192;                 // the most chromosomes a table holds (kChrSlots)
typedef unsigned long long vp_u64;

struct VpArgs {
    const uint4* rec; uint64_t n;
    const uint8_t* role; uint32_t nchr;           // 0 none, 1 viewpoint, 2 partner
    const uint32_t* poff;                         // the first partner bin of every chromosome (partners only)
    uint32_t vbin, pbin, origin, second_only;
    int B;
    uint32_t nvb; int lds_track;                  // bins of the viewpoint track; privatised in LDS or not
    uint64_t npb;                                 // bins of the partner track
    uint32_t* vtrack; uint32_t* ptrack;
    vp_u64* counters;                             // [0] matching pairs, [1] the cursor of the keys, [2] 1 + the largest occupied viewpoint bin
    uint64_t* keys; uint64_t cap;
};

template <bool EMIT>
__global__ __launch_bounds__(VP_WG) void k_vp_scan(VpArgs a) {
    __shared__ uint8_t s_role[VP_CHR];
    __shared__ uint32_t s_track[EMIT ? 1 : kVpLdsBins];
    for (uint32_t k = threadIdx.x; k < a.nchr; k += VP_WG) s_role[k] = a.role[k];
    if (!EMIT && a.lds_track) for (uint32_t k = threadIdx.x; k < a.nvb; k += VP_WG) s_track[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    vp_u64 matched = 0;                                                           // lane 0: the wave's matches
    uint32_t top = 0;                                                             // 1 + the lane's largest viewpoint bin
    const uint64_t stride = (uint64_t)gridDim.x * VP_WG;
    // every lane of a wave makes the same number of rounds (the ballots below need the whole wave)
    const uint64_t rounds = (a.n + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t j = r * stride + (uint64_t)blockIdx.x * VP_WG + threadIdx.x;
        bool hit = false;
        uint32_t vb = 0, gb = 0;
        if (j < a.n) {
            const uint4 x = a.rec[j];                                             // ia, pa, ib, pb
            if (x.x < a.nchr && x.z < a.nchr) {                                   // (a skipped record or one that is no pair has ia >= 0xFFFFFFFE)
                const uint32_t ra = s_role[x.x], rb = s_role[x.z];
                const bool second = ra == 2u && rb == 1u;                         // the viewpoint is the second side as stored
                const bool first = ra == 1u && rb == 2u && !a.second_only;
                if (second || first) {
                    const uint32_t vp = second ? x.w : x.y, pp = second ? x.y : x.w, pc = second ? x.x : x.z;
                    vb = (vp - a.origin) / a.vbin;
                    gb = a.poff[pc] + (pp - a.origin) / a.pbin;
                    hit = vb < a.nvb && gb < a.npb;                               // (always, for a record the matrix stage accepted)
                }
            }
        }
        const uint64_t ball = __ballot(hit);
        if (EMIT) {
            uint64_t base = 0;
            if (lane == 0 && ball) base = atomicAdd(&a.counters[1], (vp_u64)__popcll(ball));
            base = (uint64_t)__shfl((long long)base, 0, 64);
            if (hit) {
                const uint64_t slot = base + (uint64_t)__popcll(ball & ((1ull << lane) - 1ull));
                if (slot < a.cap) a.keys[slot] = ((uint64_t)vb << a.B) | (uint64_t)gb;
            }
        } else {
            if (lane == 0) matched += (vp_u64)__popcll(ball);
            if (hit) {
                if (a.lds_track) atomicAdd(&s_track[vb], 1u); else atomicAdd(&a.vtrack[vb], 1u);
                atomicAdd(&a.ptrack[gb], 1u);
                top = top > vb + 1u ? top : vb + 1u;
            }
        }
    }
    if (!EMIT) {
        if (lane == 0 && matched) atomicAdd(&a.counters[0], matched);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint32_t y = (uint32_t)__shfl_down((int)top, d, 64); top = top > y ? top : y; }
        if (lane == 0 && top) atomicMax(&a.counters[2], (vp_u64)top);
        if (a.lds_track) {
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < a.nvb; k += VP_WG) { const uint32_t c = s_track[k]; if (c) atomicAdd(&a.vtrack[k], c); }
        }
    }
}

// the non-empty bins of a dense track as (bin, count) pairs, in any order; *cursor: how many there are (cap of them are stored)
__global__ __launch_bounds__(VP_WG) void k_vp_compact(const uint32_t* track, uint64_t nb, vp_u64* cursor, uint32_t* bin, uint32_t* count, uint64_t cap) {
    const int lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * VP_WG, rounds = (nb + stride - 1) / stride;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t j = r * stride + (uint64_t)blockIdx.x * VP_WG + threadIdx.x;
        const uint32_t c = j < nb ? track[j] : 0u;
        const uint64_t ball = __ballot(c != 0u);
        uint64_t base = 0;
        if (lane == 0 && ball) base = atomicAdd(cursor, (vp_u64)__popcll(ball));
        base = (uint64_t)__shfl((long long)base, 0, 64);
        if (c) {
            const uint64_t slot = base + (uint64_t)__popcll(ball & ((1ull << lane) - 1ull));
            if (slot < cap) { bin[slot] = (uint32_t)j; count[slot] = c; }
        }
    }
}

// the bins a chromosome of length len has at this size and origin: positions 1 .. len
static uint64_t vp_bins(uint64_t len, uint64_t size, uint32_t origin) { return len == 0 ? 0 : (len - origin) / size + 1; }
static int vp_bits(uint64_t n) { int b = 1; while (b < 32 && (1ull << b) < n) ++b; return b; }     // the bits that hold 0 .. n - 1, at least 1

static int vp_fail(std::string* why, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static int vp_fail(std::string* why, int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (why) *why = buf;
    return code;
}
#define VP_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return vp_fail(why, e_ == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "HIP call failed: %s", hipGetErrorString(e_)); } while (0)

int vp_run(VpState& s, const uint4* rec, uint64_t n, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::vector<uint8_t>& role,
           const mkt_viewpoint_opts& o, hipStream_t st, std::string* why) {
    const uint32_t nchr = (uint32_t)lens.size(), origin = (uint32_t)o.origin;
    // the bins of the two sides
    const uint64_t nvb = vp_bins(lens[o.viewpoint], o.vbin, origin);
    std::vector<uint32_t> poff(nchr, 0), pchr;                                    // pchr: the partners in table order
    uint64_t npb = 0;
    for (uint32_t c = 0; c < nchr; ++c) {
        if (role[c] != 2) continue;
        poff[c] = (uint32_t)npb;
        pchr.push_back(c);
        npb += vp_bins(lens[c], o.pbin, origin);
        if (npb >= (1ull << 32)) return vp_fail(why, MKT_E_CAPACITY, "2^32 partner bins or more at a bin size of %u (bin ids are 32-bit)", o.pbin);
    }
    if (nvb >= (1ull << 32)) return vp_fail(why, MKT_E_CAPACITY, "2^32 viewpoint bins or more at a bin size of %u (bin ids are 32-bit)", o.vbin);
    if (nvb && !vp_links_fit(nvb - 1, o.vbin)) return vp_fail(why, MKT_E_ARG, "viewpoint bin %llu of %u bp times %llu does not fit 63 bits (the links text)", (unsigned long long)(nvb - 1), o.vbin, (unsigned long long)kVpEnlarge);
    const int B = vp_bits(npb), Bv = vp_bits(nvb);
    VpState out;
    out.info.viewpoint_bins = 0;
    if (n == 0 || nvb == 0 || npb == 0) { out.built = true; s = std::move(out); return MKT_OK; }

    // half of the free memory at the most for the partner track (it is dense)
    size_t mem_free = 0, mem_total = 0;
    VP_HIP(hipMemGetInfo(&mem_free, &mem_total));
    if ((npb + nvb) * 4 > mem_free / 2) return vp_fail(why, MKT_E_NOMEM, "the dense tracks of %llu partner bins and %llu viewpoint bins do not fit half of the %zu free bytes", (unsigned long long)npb, (unsigned long long)nvb, mem_free);
    DevEvents<4> ev;
    VP_HIP(ev.create());
    DevBuf<uint8_t> d_role;
    DevBuf<uint32_t> d_poff, d_vtrack, d_ptrack;
    DevBuf<vp_u64> d_cnt;
    VP_HIP(d_role.alloc(nchr)); VP_HIP(d_poff.alloc(nchr)); VP_HIP(d_vtrack.alloc(nvb, 64)); VP_HIP(d_ptrack.alloc(npb, 64)); VP_HIP(d_cnt.alloc(4));
    VP_HIP(hipMemcpyAsync(d_role, role.data(), nchr, hipMemcpyHostToDevice, st));
    VP_HIP(hipMemcpyAsync(d_poff, poff.data(), (size_t)nchr * 4, hipMemcpyHostToDevice, st));
    VP_HIP(hipMemsetAsync(d_vtrack, 0, nvb * 4, st));
    VP_HIP(hipMemsetAsync(d_ptrack, 0, npb * 4, st));
    VP_HIP(hipMemsetAsync(d_cnt, 0, 4 * sizeof(vp_u64), st));
    VpArgs a;
    memset(&a, 0, sizeof a);
    a.rec = rec; a.n = n; a.role = d_role; a.nchr = nchr; a.poff = d_poff;
    a.vbin = o.vbin; a.pbin = o.pbin; a.origin = origin; a.second_only = (uint32_t)o.second_side_only;
    a.B = B; a.nvb = (uint32_t)nvb; a.npb = npb; a.lds_track = nvb <= kVpLdsBins;
    a.vtrack = d_vtrack; a.ptrack = d_ptrack; a.counters = d_cnt;
    const unsigned grid = std::min<unsigned>(grid_for(n, VP_WG), VP_MAX_GRID);
    VP_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_vp_scan<false>, dim3(grid), dim3(VP_WG), 0, st, a);
    VP_HIP(hipGetLastError());
    VP_HIP(hipEventRecord(ev[1], st));
    vp_u64 hc[4] = {0, 0, 0, 0};
    VP_HIP(hipMemcpyAsync(hc, d_cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    const uint64_t total = hc[0], top = hc[2];
    if (total > n || top > nvb) return vp_fail(why, MKT_E_KERNEL, "%llu matching pairs of %llu records, viewpoint bin %llu of %llu", (unsigned long long)total, (unsigned long long)n, (unsigned long long)top, (unsigned long long)nvb);
    float ms = 0;
    VP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.scan_ms = ms;
    out.info.total = total;
    if (total == 0) { out.built = true; s = std::move(out); return MKT_OK; }

    // the keys, sized exactly; their sort and the run lengths
    DevBuf<uint64_t> kA, kB, sums;
    DevBuf<uint32_t> radix, d_hi, d_lo, d_c, d_pos;
    VP_HIP(kA.alloc(total, 64)); VP_HIP(kB.alloc(total, 64));
    VP_HIP(radix.alloc(0, radix64_count_bytes(total)));
    VP_HIP(sums.alloc(rle_sums_words(total)));
    a.keys = kA; a.cap = total;
    VP_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_vp_scan<true>, dim3(grid), dim3(VP_WG), 0, st, a);
    VP_HIP(hipGetLastError());
    VP_HIP(hipEventRecord(ev[1], st));
    uint64_t *pA = kA, *pB = kB;
    VP_HIP(launch_radix64(pA, pB, total, 0, B + Bv, radix, st));
    uint64_t nlinks = 0, tb = 0;
    VP_HIP(rle_reduce(pA, total, B, sums, d_hi, d_lo, d_c, d_pos, &nlinks, &tb, st));
    VP_HIP(hipEventRecord(ev[2], st));
    // the partner track: its non-empty cells (there are at most `total`)
    DevBuf<uint32_t> d_pb, d_pc;
    VP_HIP(d_pb.alloc(total)); VP_HIP(d_pc.alloc(total));
    hipLaunchKernelGGL(k_vp_compact, dim3(std::min<unsigned>(grid_for(npb, VP_WG), VP_MAX_GRID)), dim3(VP_WG), 0, st, (const uint32_t*)d_ptrack, npb, d_cnt.get() + 3, d_pb.get(), d_pc.get(), total);
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(hc, d_cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));
    VP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    out.scan_ms += ms;
    VP_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    out.sort_ms = ms;
    const uint64_t ncells = hc[3];
    if (hc[1] != total || nlinks == 0 || nlinks > total || ncells == 0 || ncells > total)
        return vp_fail(why, MKT_E_KERNEL, "%llu keys, %llu links and %llu partner cells from %llu matching pairs", (unsigned long long)hc[1], (unsigned long long)nlinks, (unsigned long long)ncells, (unsigned long long)total);
    std::vector<uint32_t> hi(nlinks), lo(nlinks), lc(nlinks), pb(ncells), pc(ncells);
    out.track.resize(top);
    VP_HIP(hipMemcpyAsync(hi.data(), d_hi, nlinks * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipMemcpyAsync(lo.data(), d_lo, nlinks * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipMemcpyAsync(lc.data(), d_c, nlinks * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipMemcpyAsync(pb.data(), d_pb, ncells * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipMemcpyAsync(pc.data(), d_pc, ncells * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipMemcpyAsync(out.track.data(), d_vtrack, top * 4, hipMemcpyDeviceToHost, st));
    VP_HIP(hipStreamSynchronize(st));

    // a global partner bin -> (chromosome, bin): the last partner whose first bin is not above it
    auto split = [&](uint32_t gb, uint32_t* chrom, uint32_t* bin) {
        size_t lo_ = 0, hi_ = pchr.size();
        while (hi_ - lo_ > 1) { const size_t mid = (lo_ + hi_) / 2; if (poff[pchr[mid]] <= gb) lo_ = mid; else hi_ = mid; }
        // (a partner of length 0 has no bin and shares its first bin with the next one: take the last of equal offsets)
        *chrom = pchr[lo_]; *bin = gb - poff[pchr[lo_]];
    };
    out.links.resize(nlinks);
    for (uint64_t k = 0; k < nlinks; ++k) { VpLink& l = out.links[k]; l.vbin = hi[k]; l.count = lc[k]; split(lo[k], &l.chrom, &l.pbin); }
    std::vector<VpCell> cells(ncells);
    for (uint64_t k = 0; k < ncells; ++k) { cells[k].count = pc[k]; split(pb[k], &cells[k].chrom, &cells[k].pbin); }
    vp_sort_partners(cells, names);
    for (const VpCell& c : cells) if (c.count >= o.min_count) out.partners.push_back(c);
    out.info.links = nlinks;
    out.info.min_loop = vp_min_loop(out.links, total, o.hotspot_ratio);
    for (const VpLink& l : out.links) out.info.links_kept += l.count >= out.info.min_loop;
    out.info.viewpoint_bins = top;
    out.info.partner_cells = ncells;
    out.info.partner_cells_kept = out.partners.size();
    out.built = true;
    s = std::move(out);
    return MKT_OK;
}

}  // namespace mkt

// ---- the entry points -----------------------------------------------------------------------------------------------------------
using namespace mkt;

static int vp_have(mkt_matrix* m) {
    if (!m) return MKT_E_ARG;
    if (!(m->ran && m->vp.built)) return mfail(m, MKT_E_STATE, "no viewpoint profile: viewpoint first");
    return MKT_OK;
}

extern "C" {

void mkt_viewpoint_opts_default(mkt_viewpoint_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->vbin = 200; o->pbin = 1000000; o->min_count = 1; o->hotspot_ratio = 0.01;
}

int mkt_matrix_viewpoint(mkt_matrix* m, const mkt_viewpoint_opts* opts, mkt_viewpoint_info* info) {
    if (!m) return MKT_E_ARG;
    if (info) memset(info, 0, sizeof *info);
    const mkt_viewpoint_opts o = mx_opts(opts, mkt_viewpoint_opts_default);
    const uint32_t nc = (uint32_t)m->names.size();
    if (o.viewpoint >= nc) return mfail(m, MKT_E_ARG, "viewpoint: chromosome index %u of %u", o.viewpoint, nc);
    if (o.partner_mask && o.partner_mask[o.viewpoint]) return mfail(m, MKT_E_ARG, "viewpoint: %s is in its own partner mask", m->names[o.viewpoint].c_str());
    if (o.vbin == 0 || o.pbin == 0) return mfail(m, MKT_E_ARG, "viewpoint: a bin size of 0 (vbin %u, pbin %u)", o.vbin, o.pbin);
    if (o.origin != 0 && o.origin != 1) return mfail(m, MKT_E_ARG, "viewpoint: origin %d (0 or 1)", o.origin);
    if (o.second_side_only != 0 && o.second_side_only != 1) return mfail(m, MKT_E_ARG, "viewpoint: second_side_only %d (0 or 1)", o.second_side_only);
    if (o.min_count == 0) return mfail(m, MKT_E_ARG, "viewpoint: min_count 0 (at least 1 is needed)");
    if (!(o.hotspot_ratio >= 0.0 && o.hotspot_ratio < 1.0)) return mfail(m, MKT_E_ARG, "viewpoint: hotspot_ratio %g is outside [0, 1)", o.hotspot_ratio);
    if (o.reserved[0] != 0 || o.reserved[1] != 0) return mfail(m, MKT_E_ARG, "viewpoint: a reserved word is not 0");
    if (!m->ran) return mfail(m, MKT_E_STATE, "viewpoint before run");
    std::vector<uint8_t> role(nc, 0);
    for (uint32_t c = 0; c < nc; ++c) role[c] = c == o.viewpoint ? 1 : (!o.partner_mask || o.partner_mask[c]) ? 2 : 0;
    MCHK(m, hipSetDevice(m->device));
    VpState vs;                                                         // a refused or failed call leaves the previous results alone
    std::string why;
    const int rc = vp_run(vs, reinterpret_cast<const uint4*>(m->d_rec.get()), m->n, m->names, m->lens, role, o, m->stream, &why);
    if (rc != MKT_OK) return mfail(m, rc, "viewpoint: %s", why.c_str());
    m->vp = std::move(vs);
    if (info) *info = m->vp.info;
    return MKT_OK;
}

int mkt_matrix_fetch_viewpoint_links(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* vbin, uint32_t* chrom, uint32_t* pbin, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<VpLink>& v = m->vp.links;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint links [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    for (uint64_t k = 0; k < n; ++k) {
        const VpLink& l = v[first + k];
        if (vbin) vbin[k] = l.vbin;
        if (chrom) chrom[k] = l.chrom;
        if (pbin) pbin[k] = l.pbin;
        if (count) count[k] = l.count;
    }
    return MKT_OK;
}
int mkt_matrix_fetch_viewpoint_track(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<uint32_t>& v = m->vp.track;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint track bins [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    if (count && n) memcpy(count, v.data() + first, n * 4);
    return MKT_OK;
}
int mkt_matrix_fetch_viewpoint_partners(mkt_matrix* m, uint64_t first, uint64_t n, uint32_t* chrom, uint32_t* pbin, uint32_t* count) {
    if (const int rc = vp_have(m)) return rc;
    const std::vector<VpCell>& v = m->vp.partners;
    if (first > v.size() || n > v.size() - first) return mfail(m, MKT_E_ARG, "viewpoint partner cells [%llu, +%llu) of %zu", (unsigned long long)first, (unsigned long long)n, v.size());
    for (uint64_t k = 0; k < n; ++k) {
        const VpCell& c = v[first + k];
        if (chrom) chrom[k] = c.chrom;
        if (pbin) pbin[k] = c.pbin;
        if (count) count[k] = c.count;
    }
    return MKT_OK;
}
int mkt_matrix_viewpoint_timing(const mkt_matrix* m, double* scan_ms, double* sort_ms) {
    if (!m) return MKT_E_ARG;
    const bool have = m->ran && m->vp.built;
    mx_ms(scan_ms, have, m->vp.scan_ms); mx_ms(sort_ms, have, m->vp.sort_ms);
    return MKT_OK;
}

}  // extern "C"
