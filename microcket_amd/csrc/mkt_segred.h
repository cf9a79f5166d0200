// mkt_segred.h -- what the matrix analyses share on the device: the lower bound, the fixed-order reduction trees and the lane-width
// rule with its dispatch.  DESIGN.md 7f has the two rules that keep the bits: this header holds additions and shuffles only (it is
// compiled with and without floating-point contraction, so a multiply that feeds an add would compile two ways), and the walks that
// feed the trees stay with their kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace mkt {

inline unsigned grid_for(uint64_t n, uint32_t wg) { return (unsigned)((n + wg - 1) / wg); }
__device__ inline double dev_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// first i in [lo, hi) with (a[i] >> shift) >= v, hi when there is none
template <typename T, typename V>
__device__ inline uint32_t seg_lower_bound_key(const T* a, uint32_t lo, uint32_t hi, int shift, V v) {
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((a[mid] >> shift) < v) lo = mid + 1; else hi = mid; }
    return lo;
}
template <typename T, typename V>
__device__ inline uint32_t seg_lower_bound(const T* a, uint32_t lo, uint32_t hi, V v) { return seg_lower_bound_key(a, lo, hi, 0, v); }

// the two spellings of the adder: the sites that were written with + and the ones that were written with __dadd_rn keep theirs
struct AddPlain {
    template <typename T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct AddRn {
    __device__ double operator()(double a, double b) const { return __dadd_rn(a, b); }
    __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a + b; }
};

// W lanes (a power of two up to 64) hold one value each: lane l + d is added to lane l for d = W / 2 .. 1; the sum is in lane 0.
// Several values (of any types the adder takes) go down the tree together, step by step.
template <int W, typename Add, typename... T>
__device__ inline void lane_tree_v(Add add, T&... v) {
#pragma unroll
    for (int d = W / 2; d >= 1; d >>= 1) ((v = add(v, __shfl_down(v, d, W))), ...);
}
template <int W, typename T, typename Add, size_t... I>
__device__ inline void lane_tree_idx(T* v, Add add, std::index_sequence<I...>) { lane_tree_v<W>(add, v[I]...); }
template <int W, int N, typename T, typename Add = AddPlain>
__device__ inline void lane_tree_n(T (&v)[N], Add add = Add()) { lane_tree_idx<W>(v, add, std::make_index_sequence<N>()); }
template <int W, typename T, typename Add = AddPlain>
__device__ inline T lane_tree(T v, Add add = Add()) {
    lane_tree_v<W>(add, v);
    return v;
}
// four partial sums in their order
template <typename T, typename Add = AddPlain>
__device__ inline T sum4(T s0, T s1, T s2, T s3, Add add = Add()) { return add(add(add(s0, s1), s2), s3); }
// a workgroup of four waves: the tree per wave, the four wave sums through sh[4][N] added in wave order; valid in thread 0
template <int N, typename T, typename Add = AddPlain>
__device__ inline void wg_tree_n(T (&v)[N], T* sh, Add add = Add()) {
    lane_tree_n<64>(v, add);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) sh[(threadIdx.x >> 6) * N + j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = sum4(sh[j], sh[N + j], sh[2 * N + j], sh[3 * N + j], add);
    }
}
// the same for two values of two types behind one barrier (a sum and the count that rides along)
template <typename Add, typename A, typename B>
__device__ inline void wg_tree2(Add add, A& a, A* sha /* [4] */, B& b, B* shb /* [4] */) {
    lane_tree_v<64>(add, a, b);
    if ((threadIdx.x & 63) == 0) { sha[threadIdx.x >> 6] = a; shb[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = sum4(sha[0], sha[1], sha[2], sha[3], add);
        b = sum4(shb[0], shb[1], shb[2], shb[3], add);
    }
}
template <typename T, typename Add = AddPlain>
__device__ inline T wg_tree(T v, T* sh /* [4] */, Add add = Add()) {
    T a[1] = {v};
    wg_tree_n(a, sh, add);
    return a[0];
}

// lanes per segment from the cells a segment holds on average
inline int seg_width(uint64_t avg) { return avg >= 48 ? 64 : avg >= 24 ? 32 : avg >= 12 ? 16 : 8; }
// f(std::integral_constant<int, W>) for the W that seg_width chose
template <typename F>
inline void dispatch_width(int width, F&& f) {
    switch (width) {
        case 64: f(std::integral_constant<int, 64>()); break;
        case 32: f(std::integral_constant<int, 32>()); break;
        case 16: f(std::integral_constant<int, 16>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

}  // namespace mkt
