// mkt_px2.h -- final.pairs.gz and its pairix index final.pairs.gz.px2 (include/mkt.h has the definition; DESIGN.md 6f the kernels).
//
// Two halves.  The HOST half needs no GPU and no HIP header: the constants of the binning, the fixed part of the index's header, and
// the check of the name table for a pair that reappears.  A stand-alone program can include this file and call it
// (tests/host/px2_host.cpp does).  The DEVICE half (mkt_px2.hip) shares the constants with it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <string_view>
#include <unordered_set>

#if defined(__HIPCC__)
#define MKT_PX_HD __host__ __device__
#else
#define MKT_PX_HD
#endif

namespace mkt {

constexpr uint32_t kPxShift = 15;                       // the finest bin and the linear window: 2^15 positions
constexpr uint32_t kPxBinFirst = 4681;                  // first bin of the finest level
constexpr uint32_t kPxPosMax = 0x7FFFFFFFu;             // pairix keeps a position in an int32
constexpr uint32_t kPxHeadBytes = 64;                   // the .px2 up to its name table
constexpr int64_t kPxNoName = -1;
enum { PX_BAD_COLUMNS = 0, PX_BAD_POS = 1, PX_BAD_ORDER = 2 };      // why the per-line kernel refuses a line

// pairix indexes the one base [pos1 - 1, pos1) (a position 0 counts as 1), which always fits the finest level
MKT_PX_HD inline uint32_t px_window(uint32_t pos1) { return (pos1 ? pos1 - 1u : 0u) >> kPxShift; }

inline void px_put32(std::string& o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((char)(v >> (8 * k))); }
inline void px_put64(std::string& o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((char)(v >> (8 * k))); }

// The first kPxHeadBytes of the uncompressed index: magic, n_ref, the count of all lines, the preset `pairs` (columns 2, 3, 3 and
// 4, 5, 5), delimiter and region separator, meta character, lines to skip, the length of the name table.
inline std::string px_head(uint32_t n_ref, uint64_t n_lines, uint32_t l_nm) {
    std::string o("PX2.004\1", 8);
    px_put32(o, n_ref);
    px_put64(o, n_lines);
    for (uint32_t v : {3u, 2u, 3u, 3u, 4u, 5u, 5u}) px_put32(o, v);
    o.push_back('\t'); o.push_back('|'); o.push_back(0); o.push_back(0);
    px_put32(o, '#');
    px_put32(o, 0);
    px_put32(o, l_nm);
    return o;
}

// names[0, l_nm): n_ref names, each ending with a NUL, in the order of the runs of the file.  The index of the first name that
// stands in the table a second time (its run is where a pair reappears), or kPxNoName.
inline int64_t px_first_reappearing(const char* names, size_t l_nm, uint64_t n_ref) {
    std::unordered_set<std::string_view> seen;
    seen.reserve(n_ref * 2 + 1);
    size_t at = 0;
    for (uint64_t k = 0; k < n_ref; ++k) {
        const void* z = at < l_nm ? memchr(names + at, 0, l_nm - at) : nullptr;
        if (!z) return (int64_t)k;                         // a table that ends early: treated as the fault of name k
        const size_t len = (size_t)((const char*)z - (names + at));
        if (!seen.insert(std::string_view(names + at, len)).second) return (int64_t)k;
        at += len + 1;
    }
    return kPxNoName;
}

}  // namespace mkt
