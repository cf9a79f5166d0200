// mkt_deflate_codes.h -- the code construction of the deflate kernel (k_bgzf_deflate in mkt_deflate.hip), written once for
// the gfx950 kernel and for the host driver of the CPU tests (tests/host/deflate_codes.cpp): RFC 1951 length / distance symbols,
// minimum-redundancy code lengths, the length limiter and the canonical codes.  Nothing here is a product CPU path: the library
// only ever runs this code inside HIP kernels.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MKT_DZ_HD __host__ __device__ inline
#else
#define MKT_DZ_HD inline
#endif

namespace mkt {

MKT_DZ_HD uint32_t dz_brev(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
#endif
}
MKT_DZ_HD uint32_t dz_clz(uint32_t v) {                 // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clz((int)v);
#else
    return (uint32_t)__builtin_clz(v);
#endif
}

MKT_DZ_HD uint32_t bitrev(uint32_t v, int n) { return dz_brev(v) >> (32 - n); }
MKT_DZ_HD void len_code(uint32_t len, uint32_t& sym, uint32_t& eb, uint32_t& ev) {       // 3..258
    if (len == 258) { sym = 285; eb = 0; ev = 0; return; }
    const uint32_t l = len - 3;
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    const uint32_t k = 31u - dz_clz(l);                        // 3..7
    eb = k - 2;
    sym = 257 + 4 * eb + 4 + ((l >> eb) & 3u);
    ev = l & ((1u << eb) - 1u);
}
MKT_DZ_HD void dist_code(uint32_t dist, uint32_t& sym, uint32_t& eb, uint32_t& ev) {     // 1..32768
    const uint32_t d = dist - 1;
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    const uint32_t k = 31u - dz_clz(d);
    eb = k - 1;
    sym = 2 * k + ((d >> eb) & 1u);
    ev = d & ((1u << eb) - 1u);
}
// code lengths for n symbols whose counts stand in A[0, n) in ascending order (Moffat & Katajainen, "In-place calculation of
// minimum-redundancy codes", 1995): A[i] becomes the length of the i-th rarest symbol's code.  One lane.
MKT_DZ_HD void mk_lengths(uint32_t* A, int n) {
    if (n == 0) return;
    if (n == 1) { A[0] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2; next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used; ++dpth; used = 0;
    }
}
// One lane: lengths (<= maxbits) and canonical codes for the n used symbols listed rarest first in ssym (their counts in skey);
// table[sym] = bit-reversed code | length << 16 (0 for unused symbols).
MKT_DZ_HD void huff_codes(uint32_t* skey, const uint16_t* ssym, int n, int maxbits, uint32_t* table, int nsym) {
    uint32_t num[33];
    for (int i = 0; i <= 32; ++i) num[i] = 0;
    mk_lengths(skey, n);
    for (int i = 0; i < n; ++i) num[skey[i] > 32u ? 32u : skey[i]]++;
    for (int i = maxbits + 1; i <= 32; ++i) { num[maxbits] += num[i]; num[i] = 0; }
    uint32_t total = 0;
    for (int i = maxbits; i > 0; --i) total += num[i] << (maxbits - i);
    while (total > (1u << maxbits)) {                    // too many long codes: one leaves the deepest level, one code one level up splits
        num[maxbits]--;
        for (int i = maxbits - 1; i > 0; --i) if (num[i]) { num[i]--; num[i + 1] += 2; break; }
        --total;
    }
    for (int s = 0; s < nsym; ++s) table[s] = 0;
    int j = n;
    for (int i = 1; i <= maxbits; ++i) for (uint32_t l = num[i]; l > 0; --l) table[ssym[--j]] = (uint32_t)i << 16;      // short codes to the frequent
    uint32_t next_code[17];
    uint32_t code = 0;
    next_code[0] = 0;
    for (int i = 1; i <= maxbits; ++i) { code = (code + num[i - 1]) << 1; next_code[i] = code; }
    for (int s = 0; s < nsym; ++s) {
        const uint32_t l = table[s] >> 16;
        if (l) table[s] |= bitrev(next_code[l]++, (int)l);
    }
}

}  // namespace mkt
