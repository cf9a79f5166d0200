// mkt_pairstat.h -- pair statistics of a .pairs text (include/mkt.h has the definition, DESIGN.md 6k the kernels).
//
// Two halves.  SHARED with the kernels (MKT_HD): the edge table and the bin lookup, the parse of one line and the classification of
// one pair -- what a pair adds to which counter is decided here and nowhere else.  HOST only: the exact areas and P(s), the
// convergence rule, the counters of an info and the two text writers.  Nothing here needs HIP: a stand-alone program can include this
// file and compute the whole result on the CPU (tests/host/pairstat_host.cpp does); mkt_pairstat.hip does the counting on the device
// and hands the counters to the same host functions.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_chromtab.h"

namespace mkt {

constexpr int kPsBins = MKT_PAIRSTAT_BINS;          // 74
constexpr uint32_t kPsMaxChrom = MKT_PAIRSTAT_MAX_CHROM;
// 0, then round(10^(k/8)) for k = 0 .. 72 (tests/test_pairstat_host.py derives them again); the repeated 1 and 2 are meant
#define MKT_PS_EDGES                                                                                                                     \
    0u, 1u, 1u, 2u, 2u, 3u, 4u, 6u, 7u, 10u, 13u, 18u, 24u, 32u, 42u, 56u, 75u, 100u, 133u, 178u, 237u, 316u, 422u, 562u, 750u, 1000u,  \
    1334u, 1778u, 2371u, 3162u, 4217u, 5623u, 7499u, 10000u, 13335u, 17783u, 23714u, 31623u, 42170u, 56234u, 74989u, 100000u, 133352u,  \
    177828u, 237137u, 316228u, 421697u, 562341u, 749894u, 1000000u, 1333521u, 1778279u, 2371374u, 3162278u, 4216965u, 5623413u,         \
    7498942u, 10000000u, 13335214u, 17782794u, 23713737u, 31622777u, 42169650u, 56234133u, 74989421u, 100000000u, 133352143u,           \
    177827941u, 237137371u, 316227766u, 421696503u, 562341325u, 749894209u, 1000000000u
constexpr uint32_t kPsEdges[kPsBins] = {MKT_PS_EDGES};
constexpr uint64_t kPsLastHi = 1ull << 32;          // where bin 73 ends for its area
constexpr uint32_t kPsThresholds[6] = {1000u, 2000u, 4000u, 10000u, 20000u, 40000u};

// the counters: 74 x 4 distance cells (bin * 4 + orientation, ++ +- -+ --), then the scalars
enum { PS_TOTAL = 0, PS_SKIPPED, PS_CIS, PS_TRANS, PS_NO_STRAND, PS_HEADER, PS_GE0, PS_REF0 = PS_GE0 + 6, PS_SCALARS = PS_REF0 + 4 };
enum { PS_REF_CIS0 = 0, PS_REF_CIS1K, PS_REF_CIS10K, PS_REF_TRANS };      // the reference's classes: by name bytes and distance alone, no table
constexpr int kPsDistCells = kPsBins * 4;
constexpr int kPsCells = kPsDistCells + PS_SCALARS;
constexpr uint32_t kPsNoOri = 4;

// (number of edges <= d) - 1
MKT_HD uint32_t ps_bin(uint32_t d) {
    const uint32_t e[kPsBins] = {MKT_PS_EDGES};
    uint32_t lo = 0, hi = kPsBins;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (e[mid] <= d) lo = mid + 1; else hi = mid; }
    return lo - 1u;                                 // e[0] = 0 <= d: lo >= 1
}

// what one line is, and what it adds
enum { PS_K_HEADER = 0, PS_K_BAD, PS_K_SKIPPED, PS_K_CIS, PS_K_TRANS };
struct PsClass {
    uint32_t kind;
    uint32_t cell;                                  // chr1 index * n + chr2 index of a counted pair
    uint32_t dist;                                  // of a cis pair
    uint32_t ori;                                   // 0 .. 3, or kPsNoOri
    uint32_t ref;                                   // PS_REF_* of a data line, skipped or not
};
// table indices (MX_SKIP: not in the table), positions, orientation, whether the two names are the same bytes -> class.  n: names in the table
MKT_HD PsClass ps_classify(uint32_t ia, uint64_t pa, uint32_t ib, uint64_t pb, uint32_t ori, bool same_name, const MxTab* tab, uint32_t n) {
    PsClass c;
    c.kind = PS_K_SKIPPED; c.cell = 0; c.dist = 0; c.ori = ori;
    const uint64_t dr = pa > pb ? pa - pb : pb - pa;
    c.ref = !same_name ? PS_REF_TRANS : dr < 1000u ? PS_REF_CIS0 : dr < 10000u ? PS_REF_CIS1K : PS_REF_CIS10K;
    if (ia >= n || ib >= n || pa < 1 || pb < 1 || pa > tab->len[ia] || pb > tab->len[ib]) return c;
    c.cell = ia * n + ib;
    if (ia != ib) { c.kind = PS_K_TRANS; return c; }
    c.kind = PS_K_CIS;
    c.dist = (uint32_t)(pa > pb ? pa - pb : pb - pa);         // both at most 2^32 - 1
    return c;
}
// the scalar counters a line of this class adds 1 to, as bits PS_TOTAL ..
MKT_HD uint32_t ps_scalar_mask(const PsClass& c) {
    if (c.kind == PS_K_HEADER) return 1u << PS_HEADER;
    if (c.kind == PS_K_BAD) return 0;
    uint32_t m = (1u << PS_TOTAL) | (1u << (PS_REF0 + c.ref));
    if (c.kind == PS_K_SKIPPED) return m | (1u << PS_SKIPPED);
    if (c.ori >= kPsNoOri) m |= 1u << PS_NO_STRAND;
    if (c.kind == PS_K_TRANS) return m | (1u << PS_TRANS);
    m |= 1u << PS_CIS;
    const uint32_t t[6] = {1000u, 2000u, 4000u, 10000u, 20000u, 40000u};
    for (int k = 0; k < 6; ++k) if (c.dist >= t[k]) m |= 1u << (PS_GE0 + k);
    return m;
}
// the distance cell it adds 1 to, or -1
MKT_HD int ps_dist_cell(const PsClass& c) { return c.kind == PS_K_CIS && c.ori < kPsNoOri ? (int)(ps_bin(c.dist) * 4u + c.ori) : -1; }

// the line text[ls, le) (le: its newline): columns 2 .. 7
MKT_HD PsClass ps_parse_line(const uint8_t* text, uint64_t ls, uint64_t le, const MxTab* tab, uint32_t n) {
    PsClass bad;
    bad.kind = PS_K_BAD; bad.cell = 0; bad.dist = 0; bad.ori = kPsNoOri; bad.ref = 0;
    if (ls < le && text[ls] == '#') { bad.kind = PS_K_HEADER; return bad; }
    uint64_t tabs[7];
    int nt = 0;
    for (uint64_t p = ls; p < le && nt < 7; ++p) if (text[p] == '\t') tabs[nt++] = p;
    if (nt < 4) return bad;
    const uint64_t e5 = nt >= 5 ? tabs[4] : le;
    uint64_t pos[2];
    for (int s = 0; s < 2; ++s) {                   // a plain decimal field; what exceeds 2^40 counts as 2^40
        const uint64_t a = tabs[s ? 3 : 1] + 1, b = s ? e5 : tabs[2];
        if (a == b) return bad;
        uint64_t v = 0;
        for (uint64_t p = a; p < b; ++p) {
            const uint32_t d = (uint32_t)text[p] - (uint32_t)'0';
            if (d > 9u) return bad;
            v = v * 10 + d;
            if (v > (1ull << 40)) v = 1ull << 40;
        }
        pos[s] = v;
    }
    uint32_t ori = kPsNoOri;
    if (nt >= 6) {                                  // columns 6 and 7 are there: one byte each, '+' or '-'
        const uint64_t e7 = nt >= 7 ? tabs[6] : le;
        const uint8_t s1 = text[tabs[4] + 1], s2 = text[tabs[5] + 1];      // (a byte of the line or its newline)
        if (tabs[5] == tabs[4] + 2 && e7 == tabs[5] + 2 && (s1 == '+' || s1 == '-') && (s2 == '+' || s2 == '-')) ori = (s1 == '-' ? 2u : 0u) | (s2 == '-' ? 1u : 0u);
    }
    const uint64_t a1 = tabs[0] + 1, l1 = tabs[1] - a1, a2 = tabs[2] + 1, l2 = tabs[3] - a2;
    bool same = l1 == l2;
    for (uint64_t k = 0; same && k < l1; ++k) same = text[a1 + k] == text[a2 + k];
    return ps_classify(mx_tab_find(tab, text, a1, tabs[1]), pos[0], mx_tab_find(tab, text, a2, tabs[3]), pos[1], ori, same, tab, n);
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 ps_u128;

// one line into host counters (what the kernels do with LDS and atomics): ctr[kPsCells], chrom[n * n]
inline void ps_count_host(const PsClass& c, uint64_t* ctr, uint64_t* chrom) {
    const uint32_t m = ps_scalar_mask(c);
    for (int s = 0; s < PS_SCALARS; ++s) if ((m >> s) & 1u) ++ctr[kPsDistCells + s];
    const int d = ps_dist_cell(c);
    if (d >= 0) ++ctr[d];
    if (c.kind == PS_K_CIS || c.kind == PS_K_TRANS) ++chrom[c.cell];
}

inline uint64_t ps_bin_hi(int k) { return k + 1 < kPsBins ? kPsEdges[k + 1] : kPsLastHi; }
// area[k] = sum over chromosomes of sum_{d = lo}^{min(hi, L) - 1} (L - d)
inline void ps_areas(const std::vector<uint32_t>& lens, ps_u128* area) {
    for (int k = 0; k < kPsBins; ++k) {
        const uint64_t lo = kPsEdges[k], hi = ps_bin_hi(k);
        ps_u128 a = 0;
        for (const uint32_t L : lens) {
            const uint64_t m = hi < L ? hi : L;
            if (m <= lo) continue;
            const ps_u128 cnt = m - lo;
            a += cnt * L - (ps_u128)(lo + m - 1) * cnt / 2;           // (lo + m - 1) * cnt is even: cnt consecutive integers from lo
        }
        area[k] = a;
    }
}
inline std::string ps_u128_str(ps_u128 v) {
    char buf[48];
    int at = (int)sizeof buf;
    buf[--at] = 0;
    do { buf[--at] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
    return buf + at;
}
inline std::string ps_double_str(double x) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.17g", x);
    return buf;
}
inline void ps_scaling(const uint64_t* dist, const ps_u128* area, double* area_d, double* p) {
    for (int k = 0; k < kPsBins; ++k) {
        const uint64_t T = dist[k * 4] + dist[k * 4 + 1] + dist[k * 4 + 2] + dist[k * 4 + 3];
        area_d[k] = (double)area[k];                                 // round to nearest even, once
        p[k] = area[k] ? (double)T / area_d[k] : 0.0;
    }
}
// edge[K] of the smallest K such that bin K is thick and balanced and every thick bin behind it is balanced; -1: none
inline int64_t ps_convergence(const uint64_t* dist, uint32_t tol_permille, uint64_t min_count) {
    int K = -1;
    for (int k = kPsBins - 1; k >= 0; --k) {
        const uint64_t* c = dist + k * 4;
        const uint64_t T = c[0] + c[1] + c[2] + c[3];
        if (T < min_count) continue;
        bool balanced = true;
        for (int o = 0; o < 4; ++o) {
            const ps_u128 x = (ps_u128)4 * c[o], dev = x > T ? x - T : T - x;
            if (dev * 1000 > (ps_u128)4 * T * tol_permille) balanced = false;
        }
        if (!balanced) break;
        K = k;
    }
    return K < 0 ? -1 : (int64_t)kPsEdges[K];
}
inline void ps_info(const uint64_t* ctr, uint32_t n_chrom, int64_t convergence, mkt_pairstat_info& I) {
    memset(&I, 0, sizeof I);
    const uint64_t* s = ctr + kPsDistCells;
    I.total = s[PS_TOTAL]; I.skipped = s[PS_SKIPPED]; I.counted = I.total - I.skipped;
    I.cis = s[PS_CIS]; I.trans = s[PS_TRANS]; I.no_strand = s[PS_NO_STRAND]; I.header_lines = s[PS_HEADER];
    for (int k = 0; k < 6; ++k) I.cis_ge[k] = s[PS_GE0 + k];
    I.cis0 = s[PS_REF0 + PS_REF_CIS0]; I.cis1K = s[PS_REF0 + PS_REF_CIS1K]; I.cis10K = s[PS_REF0 + PS_REF_CIS10K]; I.ref_trans = s[PS_REF0 + PS_REF_TRANS];
    I.convergence_dist = convergence;
    I.n_chrom = n_chrom;
}
inline const char* ps_ori_name(int o) { static const char* const nm[4] = {"++", "+-", "-+", "--"}; return nm[o]; }
inline std::string ps_bin_name(int k) {
    if (k + 1 == kPsBins) return std::to_string(kPsEdges[k]) + "+";
    return std::to_string(kPsEdges[k]) + "-" + std::to_string(kPsEdges[k + 1]);
}
// PREFIX.pairs.stat
inline std::string ps_stat_text(const mkt_pairstat_info& I, const std::vector<std::string>& names, const uint64_t* chrom, const uint64_t* dist) {
    static const char* const ge[6] = {"cis_1kb+", "cis_2kb+", "cis_4kb+", "cis_10kb+", "cis_20kb+", "cis_40kb+"};
    std::string o;
    auto kv = [&](const std::string& k, uint64_t v) { o += k; o += '\t'; o += std::to_string(v); o += '\n'; };
    auto frac = [&](const std::string& k, uint64_t v) { o += "summary/frac_" + k + "\t" + ps_double_str(I.counted ? (double)v / (double)I.counted : 0.0) + "\n"; };
    kv("total", I.total); kv("skipped", I.skipped); kv("counted", I.counted); kv("cis", I.cis); kv("trans", I.trans); kv("no_strand", I.no_strand);
    kv("header_lines", I.header_lines);
    for (int k = 0; k < 6; ++k) kv(ge[k], I.cis_ge[k]);
    kv("reference/trans", I.ref_trans); kv("reference/cis10K", I.cis10K); kv("reference/cis1K", I.cis1K); kv("reference/cis0", I.cis0);
    frac("cis", I.cis);
    for (int k = 0; k < 6; ++k) frac(ge[k], I.cis_ge[k]);
    frac("trans", I.trans);
    o += "summary/convergence_dist\t" + std::to_string((long long)I.convergence_dist) + "\n";
    const size_t n = names.size();
    for (size_t a = 0; a < n; ++a)
        for (size_t b = 0; b < n; ++b)
            if (chrom[a * n + b]) kv("chrom_freq/" + names[a] + "/" + names[b], chrom[a * n + b]);
    for (int k = 0; k < kPsBins; ++k)
        for (int q = 0; q < 4; ++q) kv("dist_freq/" + ps_bin_name(k) + "/" + ps_ori_name(q), dist[k * 4 + q]);
    return o;
}
// PREFIX.scaling.tsv
inline std::string ps_scaling_text(const uint64_t* dist, const ps_u128* area, const double* p) {
    std::string o = "lo\thi\tarea\t++\t+-\t-+\t--\ttotal\tP\n";
    for (int k = 0; k < kPsBins; ++k) {
        const uint64_t* c = dist + k * 4;
        o += std::to_string(kPsEdges[k]) + "\t" + std::to_string(ps_bin_hi(k)) + "\t" + ps_u128_str(area[k]);
        for (int q = 0; q < 4; ++q) o += "\t" + std::to_string(c[q]);
        o += "\t" + std::to_string(c[0] + c[1] + c[2] + c[3]) + "\t" + ps_double_str(p[k]) + "\n";
    }
    return o;
}

// everything behind the counters, as the library and the host driver keep it
struct PsResult {
    mkt_pairstat_info info;
    ps_u128 area[kPsBins];
    double area_d[kPsBins], p[kPsBins];
    std::string stat, scaling;
};
inline void ps_finish(const uint64_t* ctr, const uint64_t* chrom, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, uint32_t tol_permille,
                      uint64_t min_count, PsResult& R) {
    ps_info(ctr, (uint32_t)names.size(), ps_convergence(ctr, tol_permille, min_count), R.info);
    ps_areas(lens, R.area);
    ps_scaling(ctr, R.area, R.area_d, R.p);
    R.stat = ps_stat_text(R.info, names, chrom, ctr);
    R.scaling = ps_scaling_text(ctr, R.area, R.p);
}

}  // namespace mkt
