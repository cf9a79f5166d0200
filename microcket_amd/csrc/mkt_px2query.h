// mkt_px2query.h -- region queries on a BGZF .pairs.gz through its pairix .px2 (include/mkt.h has the definition, DESIGN.md 6h the
// plan and the kernels; tests/pairsquerydef.py states the same in Python).
//
// The host half, as plain inline functions: the walk over an inflated .px2 that keeps names, bins, chunks and linear indexes
// (px2_parse), the region grammar with its refusals (q_parse_region), the expansion of `*` and of a flipped pair into sub-queries, the
// selection of chunks through bins and the linear index, and the block plan: which members of the file a batch touches and where
// each lands in a compact text buffer (q_plan, q_layout).  The shared half: the filter of one candidate line (q_match_line), which
// the kernel of mkt_inflate.hip and the host driver (tests/host/pairsquery_host.cpp) both run.  Compiled without hipcc this file
// includes no HIP header, like mkt_inflate.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "mkt_inflate.h"

#if defined(__HIPCC__)
#define MKT_Q_UNROLL _Pragma("unroll")
#else
#define MKT_Q_UNROLL
#endif

namespace mkt {

constexpr int64_t kQEndMax = (int64_t)1 << 30;            // pairix clips the first range of a region here
constexpr int64_t kQWholeEnd = (int64_t)1 << 30;          // a side without a range is [0, 2^30)
constexpr uint32_t kQMaxDigits = 18;                      // a bound of more digits is no number
constexpr uint64_t kQMaxLine = ((uint64_t)1 << 24) - 2;   // a longer candidate line never matches (256 of them with their '\n' fit 32 bits)
constexpr uint64_t kQPosMax = 0x7FFFFFFFull;
constexpr uint64_t kQRunGap = 64;                         // bytes between two runs of members in the compact buffer

// ---- the index ---------------------------------------------------------------------------------------------------------------------
struct Px2Bin { uint32_t id, n_chunk; uint64_t first; };  // chunks [first, first + n_chunk) of cbeg / cend
struct Px2Index {
    uint64_t n_lines = 0;
    std::string names;                                    // the name table as it stands in the file: every name with its NUL
    std::vector<uint32_t> name_off;                       // n_ref + 1 offsets into names
    std::vector<uint64_t> bin_first, lin_first;           // n_ref + 1 each
    std::vector<Px2Bin> bins;                             // the bins of a name ascending by id
    std::vector<uint64_t> cbeg, cend, lin;
    std::unordered_map<std::string, uint32_t> by_name;    // the first name id of a pair
    uint32_t n_ref() const { return name_off.empty() ? 0u : (uint32_t)name_off.size() - 1u; }
    void clear() { *this = Px2Index(); }
};

// The fields of the uncompressed bytes d[0, len) of a .px2, every byte accounted for (tests/px2def.py parse_px2_raw).  d is readable
// one byte past len.  false: err says why.
inline bool px2_parse(const uint8_t* d, uint64_t len, Px2Index& ix, std::string& err) {
    ix.clear();
    auto rd32 = [&](uint64_t at) { return (uint32_t)d[at] | (uint32_t)d[at + 1] << 8 | (uint32_t)d[at + 2] << 16 | (uint32_t)d[at + 3] << 24; };
    auto rd64 = [&](uint64_t at) { return (uint64_t)rd32(at) | (uint64_t)rd32(at + 4) << 32; };
    auto inside = [&](uint64_t r) { err = "the index ends inside name " + std::to_string(r); return false; };
    if (len < 64 || memcmp(d, "PX2.004\1", 8)) { err = "the index: not a PX2.004 file"; return false; }
    const uint64_t n_ref = rd32(8), l_nm = rd32(60);
    ix.n_lines = rd64(12);
    if (n_ref > 0x7FFFFFFFull || l_nm > len - 64) { err = "the index: the name table runs past its end"; return false; }
    uint64_t at = 64, names = 0;
    ix.name_off.push_back(0);
    for (uint64_t k = 0; k < l_nm; ++k) if (d[at + k] == 0) { ++names; ix.name_off.push_back((uint32_t)(k + 1)); }
    if (names != n_ref || (l_nm && d[at + l_nm - 1] != 0)) { err = "the index: " + std::to_string(names) + " names for n_ref " + std::to_string(n_ref); return false; }
    ix.names.assign((const char*)d + at, l_nm);
    at += l_nm;
    for (uint64_t r = 0; r < n_ref; ++r) {
        if (len - at < 4) return inside(r);
        const uint64_t n_bin = rd32(at);
        at += 4;
        ix.bin_first.push_back(ix.bins.size());
        for (uint64_t k = 0; k < n_bin; ++k) {
            if (len - at < 8) return inside(r);
            const uint64_t n_chunk = rd32(at + 4);
            const uint32_t id = rd32(at);
            at += 8;
            if (n_chunk > (len - at) / 16) return inside(r);
            ix.bins.push_back(Px2Bin{id, (uint32_t)n_chunk, (uint64_t)ix.cbeg.size()});
            for (uint64_t c = 0; c < n_chunk; ++c) { ix.cbeg.push_back(rd64(at + 16 * c)); ix.cend.push_back(rd64(at + 16 * c + 8)); }
            at += 16 * n_chunk;
        }
        std::stable_sort(ix.bins.begin() + (ptrdiff_t)ix.bin_first.back(), ix.bins.end(), [](const Px2Bin& a, const Px2Bin& b) { return a.id < b.id; });
        if (len - at < 4) return inside(r);
        const uint64_t n_intv = rd32(at);
        at += 4;
        if (n_intv > (len - at) / 8) return inside(r);
        ix.lin_first.push_back(ix.lin.size());
        for (uint64_t k = 0; k < n_intv; ++k) ix.lin.push_back(rd64(at + 8 * k));
        at += 8 * n_intv;
    }
    ix.bin_first.push_back(ix.bins.size());
    ix.lin_first.push_back(ix.lin.size());
    if (at != len) { err = "the index: " + std::to_string(len - at) + " bytes behind the last linear index"; ix.clear(); return false; }
    for (uint32_t r = 0; r < (uint32_t)n_ref; ++r) ix.by_name.emplace(std::string(ix.names.data() + ix.name_off[r], ix.name_off[r + 1] - ix.name_off[r] - 1), r);
    return true;
}

// ---- regions ---------------------------------------------------------------------------------------------------------------------------
struct QSide { bool star = false; std::string chr; int64_t b = 0, e = kQWholeEnd; };

inline bool q_bound(const std::string& s, int64_t* v) {
    uint32_t digits = 0;
    int64_t x = 0;
    for (char c : s) {
        if (c == ',') continue;
        if (c < '0' || c > '9' || ++digits > kQMaxDigits) return false;
        x = x * 10 + (c - '0');
    }
    *v = x;
    return digits > 0;
}
// nullptr, or why the side is refused
inline const char* q_parse_side(const std::string& s, QSide& o) {
    o = QSide();
    if (s == "*") { o.star = true; return nullptr; }
    const size_t c = s.rfind(':');
    if (c == std::string::npos) {
        if (s.empty()) return "an empty chromosome name";
        o.chr = s;
        return nullptr;
    }
    if (c == 0) return "an empty chromosome name";
    o.chr = s.substr(0, c);
    if (o.chr == "*") return "the * side takes no range";
    const std::string r = s.substr(c + 1);
    const size_t m = r.find('-');
    int64_t b = 0, e = 0;
    if (m == std::string::npos || r.find('-', m + 1) != std::string::npos || !q_bound(r.substr(0, m), &b) || !q_bound(r.substr(m + 1), &e)) return "a bound of a range is no number";
    if (b > e) return "the start coordinate must not exceed the end coordinate";
    o.b = b > 0 ? b - 1 : 0;                             // pairix answers b = 0 as b = 1
    o.e = e;
    return nullptr;
}
inline const char* q_parse_region(const std::string& r, QSide& a, QSide& b) {
    const size_t bar = r.find('|');
    if (bar == std::string::npos) return "no '|': a one-sided query on a 2D file is not offered";
    if (r.find('|', bar + 1) != std::string::npos) return "more than one '|'";
    if (const char* w = q_parse_side(r.substr(0, bar), a)) return w;
    if (const char* w = q_parse_side(r.substr(bar + 1), b)) return w;
    if (a.star && b.star) return "*|* is not offered";
    return nullptr;
}

// ---- the plan --------------------------------------------------------------------------------------------------------------------------
// A sub-query: one name of the table with its two ranges (0-based half-open, e1 clipped).  a_* / b_*: the two chromosomes in the name table.
struct QSub { uint32_t a_off, a_len, b_off, b_len; int64_t b1, e1, b2, e2; uint32_t region, tid; };
static_assert(sizeof(QSub) == 56, "QSub is shared with the device as it is");
// A span of text that one sub-query scans: [lo, hi) first in text offsets (q_plan), then in offsets of the buffer scanned (q_layout).
struct QSpan { uint64_t lo, hi; uint32_t sub, first_member; };
static_assert(sizeof(QSpan) == 24, "QSpan is shared with the device as it is");

struct QPlan {
    std::vector<QSub> subs;
    std::vector<QSpan> spans;                             // region order, then sub-query order, then file order
    std::vector<uint64_t> region_first;                   // n + 1: the first span of every region
    std::vector<uint32_t> members;                        // the members to inflate, ascending
    std::vector<uint64_t> tbase;                          // where each lands in the compact buffer
    uint64_t compact_bytes = 0, member_bytes = 0, runs = 0;
};

// the member and the text offset a virtual offset points to; false: the index does not belong to this file
inline bool q_member_of(const std::vector<InfBlock>& blocks, uint64_t gz_len, uint64_t v, uint64_t* k, uint64_t* toff) {
    const uint64_t c = v >> 16, o = v & 0xFFFFu;
    if (c == gz_len && o == 0) { *k = blocks.size(); *toff = blocks.empty() ? 0 : blocks.back().toff + blocks.back().isize; return true; }
    const auto it = std::lower_bound(blocks.begin(), blocks.end(), c, [](const InfBlock& b, uint64_t x) { return b.coff < x; });
    if (it == blocks.end() || it->coff != c || o > it->isize) return false;
    *k = (uint64_t)(it - blocks.begin());
    *toff = it->toff + o;
    return true;
}
inline bool q_index_belongs(const Px2Index& ix, const std::vector<InfBlock>& blocks, uint64_t gz_len) {
    uint64_t k, t;
    for (size_t c = 0; c < ix.cbeg.size(); ++c)
        if (!q_member_of(blocks, gz_len, ix.cbeg[c], &k, &t) || !q_member_of(blocks, gz_len, ix.cend[c], &k, &t)) return false;
    return true;
}

inline void q_add_sub(const Px2Index& ix, uint32_t tid, const QSide& r1, const QSide& r2, uint32_t region, std::vector<QSub>& out) {
    const char* nm = ix.names.data() + ix.name_off[tid];
    const uint32_t n = ix.name_off[tid + 1] - ix.name_off[tid] - 1;
    const void* bar = memchr(nm, '|', n);
    const uint32_t la = bar ? (uint32_t)((const char*)bar - nm) : n;
    QSub s;
    s.a_off = ix.name_off[tid]; s.a_len = la;
    s.b_off = ix.name_off[tid] + (bar ? la + 1 : n); s.b_len = bar ? n - la - 1 : 0;
    s.b1 = r1.b; s.e1 = std::min(r1.e, kQEndMax); s.b2 = r2.b; s.e2 = r2.e;
    s.region = region; s.tid = tid;
    out.push_back(s);
}
// The sub-queries of one region: a star is every name whose other side is the chromosome given, in name-table order; with
// autoflip an absent pair whose flip is present is answered flipped.  nullptr, or why the region is refused.
inline const char* q_expand(const Px2Index& ix, const std::string& region, bool autoflip, uint32_t r, std::vector<QSub>& out) {
    QSide a, b;
    if (const char* w = q_parse_region(region, a, b)) return w;
    if (a.star || b.star) {
        const std::string& want = a.star ? b.chr : a.chr;
        for (uint32_t t = 0; t < ix.n_ref(); ++t) {
            const char* nm = ix.names.data() + ix.name_off[t];
            const uint32_t n = ix.name_off[t + 1] - ix.name_off[t] - 1;
            const void* bar = memchr(nm, '|', n);
            const uint32_t la = bar ? (uint32_t)((const char*)bar - nm) : n;
            const char* side = a.star ? nm + (bar ? la + 1 : n) : nm;
            const uint32_t ls = a.star ? (bar ? n - la - 1 : 0) : la;
            if (ls == want.size() && !memcmp(side, want.data(), ls)) q_add_sub(ix, t, a, b, r, out);
        }
        return nullptr;
    }
    auto it = ix.by_name.find(a.chr + "|" + b.chr);
    if (it != ix.by_name.end()) { q_add_sub(ix, it->second, a, b, r, out); return nullptr; }
    if (autoflip && (it = ix.by_name.find(b.chr + "|" + a.chr)) != ix.by_name.end()) q_add_sub(ix, it->second, b, a, r, out);
    return nullptr;
}

// The spans of sub-query s (index si) in text offsets, appended to plan.spans; the members they touch are appended to `touched` as
// [first, last] pairs.  false: a chunk points at no member of this file.
inline bool q_select(const Px2Index& ix, const std::vector<InfBlock>& blocks, uint64_t gz_len, const QSub& s, uint32_t si, std::vector<QSpan>& spans,
                     std::vector<std::pair<uint32_t, uint32_t>>& touched) {
    static const uint32_t level_first[6] = {0, 1, 9, 73, 585, 4681};
    if (s.b1 >= s.e1) return true;
    const uint64_t l0 = ix.lin_first[s.tid], nl = ix.lin_first[s.tid + 1] - l0;
    const uint64_t w = (uint64_t)s.b1 >> 15;
    const uint64_t min_off = nl ? ix.lin[l0 + std::min(w, nl - 1)] : 0;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    const auto b0 = ix.bins.begin() + (ptrdiff_t)ix.bin_first[s.tid], b1 = ix.bins.begin() + (ptrdiff_t)ix.bin_first[s.tid + 1];
    for (int lv = 0; lv < 6; ++lv) {                      // e1 <= 2^30: the bins of a level that overlap [b1, e1) are a range of ids
        const int sh = 15 + 3 * (5 - lv);
        const uint64_t lo = level_first[lv] + ((uint64_t)s.b1 >> sh), hi = level_first[lv] + ((uint64_t)(s.e1 - 1) >> sh);
        for (auto it = std::lower_bound(b0, b1, lo, [](const Px2Bin& b, uint64_t x) { return b.id < x; }); it != b1 && it->id <= hi; ++it)
            for (uint64_t c = it->first; c < it->first + it->n_chunk; ++c)
                if (ix.cend[c] > min_off) chunks.emplace_back(ix.cbeg[c], ix.cend[c]);
    }
    std::sort(chunks.begin(), chunks.end());
    const size_t first = spans.size();
    for (const auto& ch : chunks) {
        uint64_t kx, a, ky, z;
        if (!q_member_of(blocks, gz_len, ch.first, &kx, &a) || !q_member_of(blocks, gz_len, ch.second, &ky, &z)) return false;
        if (z <= a) continue;
        const uint32_t kend = (uint32_t)((ch.second & 0xFFFFu) ? ky : ky - 1);      // z > a: ky >= 1 where the offset is 0
        if (spans.size() > first && a < spans.back().hi) {                           // overlapping chunks of a foreign index: one span
            spans.back().hi = std::max(spans.back().hi, z);
            touched.back().second = std::max(touched.back().second, kend);
        } else {
            spans.push_back(QSpan{a, z, si, (uint32_t)kx});
            touched.emplace_back((uint32_t)kx, kend);
        }
    }
    return true;
}

// The plan of a batch.  0; 1 with err "region R: why" (R: the index in the batch); 2 "the index does not belong to this file".
inline int q_plan(const Px2Index& ix, const std::vector<InfBlock>& blocks, uint64_t gz_len, const char* const* regions, uint32_t n, bool autoflip, QPlan& P, std::string& err) {
    P = QPlan();
    std::vector<std::pair<uint32_t, uint32_t>> touched;
    for (uint32_t r = 0; r < n; ++r) {
        P.region_first.push_back(P.spans.size());
        const size_t s0 = P.subs.size();
        if (const char* w = q_expand(ix, regions[r] ? regions[r] : "", autoflip, r, P.subs)) { err = "region " + std::to_string(r) + ": " + w; return 1; }
        for (size_t s = s0; s < P.subs.size(); ++s)
            if (!q_select(ix, blocks, gz_len, P.subs[s], (uint32_t)s, P.spans, touched)) { err = "the index does not belong to this file"; return 2; }
    }
    P.region_first.push_back(P.spans.size());
    std::vector<uint8_t> mark(blocks.size(), 0);
    for (const auto& t : touched) for (uint32_t k = t.first; k <= t.second; ++k) mark[k] = 1;
    for (uint32_t k = 0; k < (uint32_t)blocks.size(); ++k) if (mark[k]) P.members.push_back(k);
    return 0;
}

// Where every member lands (runs of members adjacent in the file are adjacent in the compact buffer, so that a line that straddles a
// member edge is contiguous; kQRunGap bytes between two runs) and every span as offsets of the buffer scanned: the compact buffer,
// or with `resident` the whole text, of which nothing is inflated.
inline void q_layout(QPlan& P, const std::vector<InfBlock>& blocks, bool resident) {
    P.tbase.clear();
    P.compact_bytes = P.member_bytes = P.runs = 0;
    if (resident) { P.members.clear(); return; }
    std::vector<uint64_t> base_of(blocks.size(), 0);
    uint64_t at = 0;
    for (size_t j = 0; j < P.members.size(); ++j) {
        const uint32_t k = P.members[j];
        if (j == 0 || P.members[j - 1] + 1 != k) { if (j) at += kQRunGap; ++P.runs; }
        P.tbase.push_back(at);
        base_of[k] = at;
        at += blocks[k].isize;
        P.member_bytes += blocks[k].isize;
    }
    P.compact_bytes = at;
    for (QSpan& s : P.spans) {
        const uint64_t lo = base_of[s.first_member] + (s.lo - blocks[s.first_member].toff);
        s.hi = lo + (s.hi - s.lo);
        s.lo = lo;
    }
}

// ---- the filter of one candidate line (shared with the kernel) ---------------------------------------------------------------------------
// s[0, n): the line without its newline.  A, B: the two chromosomes of the sub-query.  0 no match, 1 match, 2 unparsed: fewer than
// five columns, a pos1 or pos2 that is no decimal number <= 2^31 - 1, or more than kQMaxLine bytes.  Reads s[0, n) only.
MKT_INF_HD inline bool q_number(const uint8_t* s, uint64_t n, int64_t* v) {
    if (n == 0 || n > 10) return false;
    uint64_t x = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t c = (uint32_t)s[i] - '0';
        if (c > 9u) return false;
        x = x * 10u + c;
    }
    *v = (int64_t)x;
    return x <= kQPosMax;
}
MKT_INF_HD inline bool q_same(const uint8_t* s, uint64_t n, const uint8_t* name, uint32_t ln) {
    if (n != ln) return false;
    for (uint32_t i = 0; i < ln; ++i) if (s[i] != name[i]) return false;
    return true;
}
MKT_INF_HD inline uint32_t q_match_line(const uint8_t* s, uint64_t n, const uint8_t* A, uint32_t la, const uint8_t* B, uint32_t lb, int64_t b1, int64_t e1, int64_t b2, int64_t e2) {
    if (n && s[0] == '#') return 0;
    if (n > kQMaxLine) return 2;
    uint64_t t[5], i = 0;                                 // t[k]: the end of column k (the line's end where it has no tab behind it)
    uint32_t tabs = 0;
    MKT_Q_UNROLL
    for (int k = 0; k < 5; ++k) {
        while (i < n && s[i] != '\t') ++i;
        t[k] = i;
        if (i < n) { ++tabs; ++i; }
    }
    if (tabs < 4) return 2;
    int64_t p1 = 0, p2 = 0;
    if (!q_number(s + t[1] + 1, t[2] - t[1] - 1, &p1) || !q_number(s + t[3] + 1, t[4] - t[3] - 1, &p2)) return 2;
    if (!q_same(s + t[0] + 1, t[1] - t[0] - 1, A, la) || !q_same(s + t[2] + 1, t[3] - t[2] - 1, B, lb)) return 0;
    const int64_t l1 = p1 > 0 ? p1 - 1 : 0, h1 = p1 > 1 ? p1 : 1, l2 = p2 > 0 ? p2 - 1 : 0, h2 = p2 > 1 ? p2 : 1;
    return (l1 < e1 && b1 < h1 && l2 < e2 && b2 < h2) ? 1u : 0u;
}

}  // namespace mkt
