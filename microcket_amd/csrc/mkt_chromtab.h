// mkt_chromtab.h -- the chrom.sizes table of the matrix stage and of the pair statistics: its grammar, the read-only device table with
// its name lookup, and how the host fills it.  No HIP header is needed: a stand-alone host program can include this file and look names
// up exactly as the kernels do (tests/host/pairstat_host.cpp does).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "mkt_core.h"

namespace mkt {

constexpr uint32_t MX_SKIP = 0xFFFFFFFFu;          // MxRec::ia of a skipped pair; what the lookup gives for a name that is not in the table

// the given table, read-only on the device: open addressing over FNV-1a of the name (nothing is ever inserted by a kernel)
constexpr uint32_t kMxSlots = 2 * kChrSlots;
struct MxTab {
    unsigned long long hash[kMxSlots];             // 0 = empty
    uint16_t idx[kMxSlots];                        // table index of the slot's name
    uint8_t name[kChrSlots][64];                   // by table index; [63] = length (<= 63)
    uint32_t len[kChrSlots];                       // L_i
};

MKT_HD uint64_t mx_fnv(const uint8_t* p, uint64_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h ? h : 1ull;
}
// the table index of the name text[a, b), or MX_SKIP
MKT_HD uint32_t mx_tab_find(const MxTab* tab, const uint8_t* text, uint64_t a, uint64_t b) {
    const uint64_t L = b - a;
    if (L == 0 || L > 63) return MX_SKIP;
    const uint64_t h = mx_fnv(text + a, L);
    uint32_t s = (uint32_t)(h >> 17) & (kMxSlots - 1u);
    for (uint32_t probe = 0; probe < kMxSlots; ++probe) {
        const unsigned long long cur = tab->hash[s];
        if (cur == 0ull) return MX_SKIP;
        if (cur == h) {
            const uint32_t i = tab->idx[s];
            const uint8_t* nm = tab->name[i];
            bool same = nm[63] == (uint8_t)L;
            for (uint64_t k = 0; same && k < L; ++k) same = nm[k] == text[a + k];
            if (same) return i;
        }
        s = (s + 1u) & (kMxSlots - 1u);
    }
    return MX_SKIP;
}

// lines name \t length [\t ...]; empty lines and '#' lines are ignored.  Returns an empty string or what is wrong.
inline std::string mx_parse_table(const char* txt, size_t len, std::vector<std::string>& names, std::vector<uint32_t>& lens) {
    size_t p = 0, line = 0;
    char msg[160];
    while (p < len) {
        const char* nlp = (const char*)memchr(txt + p, '\n', len - p);
        size_t q = nlp ? (size_t)(nlp - txt) : len, e = q;
        ++line;
        if (e > p && txt[e - 1] == '\r') --e;
        if (e > p && txt[p] != '#') {
            size_t t = p;
            while (t < e && txt[t] != '\t') ++t;
            if (t == p || t - p > 63) { snprintf(msg, sizeof msg, "chromosome table line %zu: a name of 1 .. 63 bytes is needed", line); return msg; }
            size_t d = t + 1;
            uint64_t v = 0;
            size_t nd = 0;
            while (d < e && txt[d] >= '0' && txt[d] <= '9' && nd < 11) { v = v * 10 + (uint64_t)(txt[d] - '0'); ++d; ++nd; }
            if (t >= e || nd == 0 || (d < e && txt[d] != '\t') || v > 0xFFFFFFFFull) { snprintf(msg, sizeof msg, "chromosome table line %zu: no length (name<TAB>length, length < 2^32)", line); return msg; }
            names.emplace_back(txt + p, t - p);
            lens.push_back((uint32_t)v);
        }
        p = q + 1;
    }
    if (names.empty()) return "chromosome table: no chromosome";
    if (names.size() > kChrSlots) return "chromosome table: more than 8192 chromosomes";
    return "";
}

// the table of distinct names (at most kChrSlots of them) into *ht, which holds zeros
inline void mx_tab_fill(MxTab* ht, const std::vector<std::string>& names, const std::vector<uint32_t>& lens) {
    for (uint32_t i = 0; i < (uint32_t)names.size(); ++i) {
        const std::string& nm = names[i];
        memcpy(ht->name[i], nm.data(), nm.size());
        ht->name[i][63] = (uint8_t)nm.size();
        ht->len[i] = lens[i];
        const uint64_t h = mx_fnv((const uint8_t*)nm.data(), nm.size());
        uint32_t s = (uint32_t)(h >> 17) & (kMxSlots - 1u);
        while (ht->hash[s]) s = (s + 1u) & (kMxSlots - 1u);            // at most 8192 names in 16384 slots
        ht->hash[s] = h; ht->idx[s] = (uint16_t)i;
    }
}

}  // namespace mkt
