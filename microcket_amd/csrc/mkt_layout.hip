// mkt_layout.hip -- the per-resolution cell layout and the grouping of cells by a key (mkt_layout.h).
//
// The cells arrive sorted by (bin1, bin2), so row k (the cells with bin1 == k) is a contiguous segment: rowptr is a lower bound per
// bin.  The other half of bin k are the cells with bin2 == k; for those a transposed copy (bin1, count) ordered by (bin2, bin1) is
// made once, by grouping bin2 << 32 | cell index.
#include <hip/hip_runtime.h>

#include <vector>

#include "mkt_launch.h"
#include "mkt_layout.h"
#include "mkt_segred.h"

namespace mkt {

constexpr int LYWG = 256;

__global__ __launch_bounds__(LYWG) void k_ly_chr(const uint32_t* off, uint32_t nchr, uint64_t nbins, uint16_t* chr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nbins) return;
    chr[k] = (uint16_t)(seg_lower_bound(off, 0u, nchr, k + 1) - 1u);      // first c with off[c] > k; off[0] == 0, so it is >= 1
}
__global__ __launch_bounds__(LYWG) void k_ly_rowptr(const uint32_t* b1, uint32_t nnz, uint64_t nbins, uint32_t* ptr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= nbins) ptr[k] = k == nbins ? nnz : seg_lower_bound(b1, 0u, nnz, (uint32_t)k);
}
__global__ __launch_bounds__(LYWG) void k_ly_tkeys(const uint32_t* b2, uint32_t nnz, uint64_t* key) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nnz) key[s] = ((uint64_t)b2[s] << 32) | s;
}
__global__ __launch_bounds__(LYWG) void k_ly_gather(const uint64_t* key, const uint32_t* b1, const uint32_t* cnt, uint32_t nnz, uint2* tr) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nnz) { const uint32_t s = (uint32_t)key[j]; tr[j] = make_uint2(b1[s], cnt[s]); }
}
__global__ __launch_bounds__(LYWG) void k_ly_keyptr(const uint64_t* key, int shift, uint32_t n, uint64_t last, uint32_t* ptr) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= last) ptr[k] = k == last ? n : seg_lower_bound_key(key, 0u, n, shift, k);
}

hipError_t KeyGroup::alloc(uint64_t n) {
    MKT_TRY(a_.alloc(n, 64));
    MKT_TRY(b_.alloc(n, 64));
    MKT_TRY(radix_.alloc(0, radix64_count_bytes(n)));
    ka_ = a_; kb_ = b_;
    return hipSuccess;
}
hipError_t KeyGroup::group(uint64_t n, int lo_bit, int nbits, int shift, uint64_t nptr, uint32_t* ptr_out, hipStream_t st) {
    MKT_TRY(launch_radix64(ka_, kb_, n, lo_bit, nbits, radix_, st));
    hipLaunchKernelGGL(k_ly_keyptr, dim3(grid_for(nptr, LYWG)), dim3(LYWG), 0, st, (const uint64_t*)ka_, shift, (uint32_t)n, nptr - 1, ptr_out);
    return hipGetLastError();
}

static bool ly_fits(const MxCells& c) { return c.nnz < (1ull << 32) && c.nbins < (1ull << 32); }

hipError_t layout_chr(MxLayout& L, const MxCells& c, hipStream_t st) {
    if (L.has_chr) return hipSuccess;
    if (!ly_fits(c)) return hipErrorInvalidValue;
    MKT_TRY(L.chr.alloc(c.nbins, 64));
    if (c.nbins) hipLaunchKernelGGL(k_ly_chr, dim3(grid_for(c.nbins, LYWG)), dim3(LYWG), 0, st, c.off, c.nchr, c.nbins, L.chr.get());
    MKT_TRY(hipGetLastError());
    L.has_chr = true;
    return hipSuccess;
}

hipError_t layout_rows(MxLayout& L, const MxCells& c, hipStream_t st) {
    MKT_TRY(layout_chr(L, c, st));
    if (L.has_rows) return hipSuccess;
    MKT_TRY(L.rowptr.alloc(c.nbins + 1));
    if (c.nnz == 0) MKT_TRY(hipMemsetAsync(L.rowptr, 0, (size_t)(c.nbins + 1) * 4, st));
    else hipLaunchKernelGGL(k_ly_rowptr, dim3(grid_for(c.nbins + 1, LYWG)), dim3(LYWG), 0, st, c.b1, (uint32_t)c.nnz, c.nbins, L.rowptr.get());
    MKT_TRY(hipGetLastError());
    L.has_rows = true;
    return hipSuccess;
}

hipError_t layout_full(MxLayout& L, const MxCells& c, hipStream_t st) {
    MKT_TRY(layout_rows(L, c, st));
    if (L.has_full) return hipSuccess;
    const uint64_t nnz = c.nnz, nbins = c.nbins;
    const size_t pbytes = (size_t)(nbins + 1) * 4;
    MKT_TRY(L.colptr.alloc(nbins + 1));
    MKT_TRY(L.tr.alloc(nnz, 64));
    KeyGroup g;                                                             // its scratch goes behind the synchronise below
    if (nnz == 0) MKT_TRY(hipMemsetAsync(L.colptr, 0, pbytes, st));
    else {
        MKT_TRY(g.alloc(nnz));
        hipLaunchKernelGGL(k_ly_tkeys, dim3(grid_for(nnz, LYWG)), dim3(LYWG), 0, st, c.b2, (uint32_t)nnz, g.keys());
        MKT_TRY(g.group(nnz, 32, c.B, 32, nbins + 1, L.colptr, st));        // stable: (bin2, bin1) order from (bin1, bin2) order
        hipLaunchKernelGGL(k_ly_gather, dim3(grid_for(nnz, LYWG)), dim3(LYWG), 0, st, (const uint64_t*)g.keys(), c.b1, c.cnt, (uint32_t)nnz, L.tr.get());
        MKT_TRY(hipGetLastError());
    }
    // the long bins, from the two pointer arrays (once per resolution)
    std::vector<uint32_t> rp(nbins + 1), cp(nbins + 1), lb;
    MKT_TRY(hipMemcpyAsync(rp.data(), L.rowptr, pbytes, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipMemcpyAsync(cp.data(), L.colptr, pbytes, hipMemcpyDeviceToHost, st));
    MKT_TRY(hipStreamSynchronize(st));
    for (uint64_t k = 0; k < nbins; ++k)
        if ((uint64_t)(rp[k + 1] - rp[k]) + (cp[k + 1] - cp[k]) > kBalLong) lb.push_back((uint32_t)k);
    L.nlong = (uint32_t)lb.size();
    if (L.nlong) {
        MKT_TRY(L.longbins.alloc(L.nlong));
        MKT_TRY(hipMemcpy(L.longbins, lb.data(), (size_t)L.nlong * 4, hipMemcpyHostToDevice));
    }
    L.width = seg_width(nbins ? 2 * nnz / nbins : 0);                       // cells a bin walks on average
    L.has_full = true;
    return hipSuccess;
}

}  // namespace mkt
