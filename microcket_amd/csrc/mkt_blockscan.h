// mkt_blockscan.h -- device code that the kernels of mkt_sort.hip and of mkt_rmdup.hip share: their workgroup size and the
// exclusive scan over one workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mkt {

constexpr int SWG = 256;

__device__ inline uint32_t blk_exscan(uint32_t v, uint32_t* total, uint32_t* sh /* [SWG / 64] */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= d) inc += y; }
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SWG / 64; ++w) { if (w < wv) pre += sh[w]; tot += sh[w]; }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

}  // namespace mkt
