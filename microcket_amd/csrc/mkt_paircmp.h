// mkt_paircmp.h -- pair-level concordance of two .pairs texts (include/mkt.h has the definition; DESIGN.md 6e the join).
//
// Two halves.  The HOST half needs no GPU and no HIP header: the report, the comparison of two records and the exact grouping by id
// string that resolves a run of records whose keys are equal although their ids are not (a hash collision; with the hash_bits knob,
// every run).  A stand-alone program can include this file and call it (tests/host/paircmp_host.cpp does).  The DEVICE half
// (mkt_paircmp.hip) shares the record of a parsed line with it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mkt.h"

#if defined(__HIPCC__)
#define MKT_PC_HD __host__ __device__
#else
#define MKT_PC_HD
#endif

namespace mkt {

enum { PC_COMMENT = 0, PC_SUPERSEDED = 1, PC_ONLY = 2, PC_CONSISTENT = 3, PC_DISCORDANT = 4 };
constexpr uint32_t kPcDefaultDist = 200;
constexpr uint32_t kPcNoPartner = 0xFFFFFFFFu;

// a parsed line: where its first four tabs and the end of its fifth field lie (offsets from the line's start) and its two positions
struct PcLine { uint32_t t0, t1, t2, t3, e5, p1, p2, data; };

// one record of a run, its strings pointing into the bytes of its line
struct PcItem {
    uint32_t line;                        // the caller's index of the line
    uint32_t side;                        // 0 = A, 1 = B
    const char* text;                     // the line's first byte
    PcLine ln;
    const char* id() const { return text; }
    uint32_t id_len() const { return ln.t0; }
    const char* c1() const { return text + ln.t0 + 1; }
    uint32_t c1_len() const { return ln.t1 - ln.t0 - 1; }
    const char* c2() const { return text + ln.t2 + 1; }
    uint32_t c2_len() const { return ln.t3 - ln.t2 - 1; }
};

inline bool pc_same(const char* a, uint32_t la, const char* b, uint32_t lb) { return la == lb && (la == 0 || memcmp(a, b, la) == 0); }
MKT_PC_HD inline uint32_t pc_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
MKT_PC_HD inline uint32_t pc_dist(uint32_t max_dist) { return max_dist ? max_dist : kPcDefaultDist; }

// straight or swapped, both comparisons strict
inline bool pc_consistent(const PcItem& a, const PcItem& b, uint32_t D) {
    const bool straight = pc_same(a.c1(), a.c1_len(), b.c1(), b.c1_len()) && pc_absdiff(a.ln.p1, b.ln.p1) < D &&
                          pc_same(a.c2(), a.c2_len(), b.c2(), b.c2_len()) && pc_absdiff(a.ln.p2, b.ln.p2) < D;
    const bool swapped = pc_same(a.c1(), a.c1_len(), b.c2(), b.c2_len()) && pc_absdiff(a.ln.p1, b.ln.p2) < D &&
                         pc_same(a.c2(), a.c2_len(), b.c1(), b.c1_len()) && pc_absdiff(a.ln.p2, b.ln.p1) < D;
    return straight || swapped;
}

// The classes of the records of one run -- A records in file order, then B records in file order, as the stable sort leaves them -- by
// exact grouping on the id string: the last A record of an id is its value, the first B record of an id claims it.  cls[k] and
// partner[k] (the `line` of the claimed A record for a consistent or discordant B record, else kPcNoPartner) per item.
inline void pc_resolve(const std::vector<PcItem>& items, uint32_t D, std::vector<uint8_t>& cls, std::vector<uint32_t>& partner) {
    cls.assign(items.size(), PC_ONLY);
    partner.assign(items.size(), kPcNoPartner);
    std::unordered_map<std::string, size_t> value;                 // id -> the A item that is its unclaimed value
    for (size_t k = 0; k < items.size(); ++k) {
        const PcItem& it = items[k];
        if (it.side != 0) continue;
        auto ins = value.emplace(std::string(it.id(), it.id_len()), k);
        if (!ins.second) { cls[ins.first->second] = PC_SUPERSEDED; ins.first->second = k; }
    }
    for (size_t k = 0; k < items.size(); ++k) {
        const PcItem& it = items[k];
        if (it.side == 0) continue;
        auto at = value.find(std::string(it.id(), it.id_len()));
        if (at == value.end()) continue;                           // B-only: no such id in A, or already claimed
        const size_t a = at->second;
        cls[a] = cls[k] = pc_consistent(items[a], it, D) ? PC_CONSISTENT : PC_DISCORDANT;
        partner[k] = items[a].line;
        value.erase(at);
    }
}

// the counters of an info from the class bytes of the two sides
inline void pc_count_classes(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, mkt_paircmp_info& info) {
    info.distinct_a = info.consistent = info.discordant = info.a_only = info.b_only = 0;
    for (uint64_t k = 0; k < na; ++k) {
        if (a[k] >= PC_ONLY) ++info.distinct_a;
        if (a[k] == PC_ONLY) ++info.a_only;
    }
    for (uint64_t k = 0; k < nb; ++k) {
        if (b[k] == PC_ONLY) ++info.b_only;
        if (b[k] == PC_CONSISTENT) ++info.consistent;
        if (b[k] == PC_DISCORDANT) ++info.discordant;
    }
}

// a count in millions as the script prints a double
inline std::string pc_millions(uint64_t count) {
    char buf[64];
    snprintf(buf, sizeof buf, "%.15g", (double)count / 1e6);
    return buf;
}

inline std::string pc_report(const mkt_paircmp_info& i, uint32_t max_dist, const std::string& name_a, const std::string& name_b) {
    std::string o = "Using Distance: " + std::to_string(pc_dist(max_dist)) + "\nLoading file A: " + name_a + " ...\nLoading file B: " + name_b + " ...\n\n";
    o += "Overalp report:\nA_only\t" + pc_millions(i.a_only + i.discordant) + "\nB_only\t" + pc_millions(i.b_only + i.discordant) + "\nConsistent\t" + pc_millions(i.consistent) +
         "\n#Disconcordant\t" + pc_millions(i.discordant) + "\n\n";
    for (int s = 0; s < 2; ++s)
        o += std::string("Pairs distribution report (file ") + (s ? "B" : "A") + "):\nCis (<1 K)\t" + pc_millions(i.dist[s][0]) + "\nCis (1-10 K)\t" + pc_millions(i.dist[s][1]) +
             "\nCis (>10 K)\t" + pc_millions(i.dist[s][2]) + "\nTrans\t" + pc_millions(i.dist[s][3]) + "\n\n";
    return o;
}

}  // namespace mkt
