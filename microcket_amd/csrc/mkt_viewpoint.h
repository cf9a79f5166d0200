// mkt_viewpoint.h -- viewpoint contact profiles (a virtual 4C) of the resident pair records of a matrix object: the contacts between one
// chromosome and a set of partner chromosomes, the two sides binned at different sizes.  include/mkt.h has the definition.
//
// Two halves.  The HOST half is everything behind the exact counts and needs no GPU and no HIP header: the hotspot cut, the string
// order of the kept links and the three texts (viewpoint bedgraph, partner bedgraph, Circos links).  A stand-alone program can include
// this file and call it (tests/host/viewpoint_host.cpp does).  The DEVICE half (vp_run, mkt_viewpoint.hip) is declared for hipcc only.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/mkt.h"

namespace mkt {

constexpr uint64_t kVpEnlarge = 5000;             // the factor by which the links text stretches the viewpoint chromosome

struct VpLink { uint32_t vbin, chrom, pbin, count; };      // ascending in (vbin, chrom, pbin)
struct VpCell { uint32_t chrom, pbin, count; };

// the smallest count a link needs to be kept: the histogram of the counts walked from the largest down, until the pairs in the links
// seen so far EXCEED (uint64)(total * ratio); then one above that count, clipped to the largest count.  0 without links.
inline uint32_t vp_min_loop(const std::vector<VpLink>& links, uint64_t total, double ratio) {
    if (links.empty()) return 0;
    std::map<uint32_t, uint64_t> hist;
    for (const VpLink& l : links) ++hist[l.count];
    const uint64_t cutoff = (uint64_t)((double)total * ratio);
    const uint32_t largest = hist.rbegin()->first;
    uint64_t accum = 0;
    uint64_t min_loop = (uint64_t)largest + 1;
    for (auto it = hist.rbegin(); it != hist.rend(); ++it) {
        accum += (uint64_t)it->first * it->second;
        if (accum > cutoff) { min_loop = (uint64_t)it->first + 1; break; }
    }
    return min_loop > largest ? largest : (uint32_t)min_loop;
}

// the name with its first "chr" (anywhere) replaced by "hs"
inline std::string vp_hs_name(const std::string& name) {
    const size_t at = name.find("chr");
    return at == std::string::npos ? name : name.substr(0, at) + "hs" + name.substr(at + 3);
}

// the indices of the links with count >= min_loop, in the bytewise order of the text "<vbin>\t<hs name>\t<pbin>"
inline std::vector<size_t> vp_kept_links(const std::vector<VpLink>& links, const std::vector<std::string>& names, uint32_t min_loop) {
    std::vector<std::pair<std::string, size_t>> keyed;
    for (size_t k = 0; k < links.size(); ++k) {
        const VpLink& l = links[k];
        if (l.count < min_loop) continue;
        keyed.emplace_back(std::to_string(l.vbin) + "\t" + vp_hs_name(names[l.chrom]) + "\t" + std::to_string(l.pbin), k);
    }
    std::sort(keyed.begin(), keyed.end());
    std::vector<size_t> out;
    for (const auto& kv : keyed) out.push_back(kv.second);
    return out;
}

// floor(log2(count)) the way the links text has it: in doubles through the C library, NOT a bit length
inline int vp_thickness(uint32_t count) { return (int)(std::log((double)count) / std::log(2.0)); }

// does the largest start of the links text, max_vbin * vbin * 5000 (+ one bin), stay below 2^63?
inline bool vp_links_fit(uint64_t max_vbin, uint64_t vbin) {
    const unsigned __int128 v = ((unsigned __int128)max_vbin + 1) * vbin * kVpEnlarge;
    return v < ((unsigned __int128)1 << 63);
}

// hs0 \t start \t end \t hs<c> \t start \t end \t thickness=<t>p per kept link
inline std::string vp_links_text(const std::vector<VpLink>& links, const std::vector<std::string>& names, uint32_t min_loop, uint64_t vbin, uint64_t pbin) {
    std::string out;
    for (size_t k : vp_kept_links(links, names, min_loop)) {
        const VpLink& l = links[k];
        const uint64_t i = (uint64_t)l.vbin * vbin * kVpEnlarge, j = (uint64_t)l.pbin * pbin;
        out += "hs0\t" + std::to_string(i) + "\t" + std::to_string(i + vbin * kVpEnlarge) + "\t" + vp_hs_name(names[l.chrom]) + "\t" + std::to_string(j) + "\t" + std::to_string(j + pbin) +
               "\tthickness=" + std::to_string(vp_thickness(l.count)) + "p\n";
    }
    return out;
}

// name \t start \t end \t count for every bin of the dense viewpoint track
inline std::string vp_track_text(const std::vector<uint32_t>& track, const std::string& name, uint64_t vbin) {
    std::string out;
    for (size_t i = 0; i < track.size(); ++i)
        out += name + "\t" + std::to_string((uint64_t)i * vbin) + "\t" + std::to_string((uint64_t)i * vbin + vbin) + "\t" + std::to_string(track[i]) + "\n";
    return out;
}

// the partner cells in (name bytewise, bin) order; the order of the cells with count >= min_count among them
inline void vp_sort_partners(std::vector<VpCell>& cells, const std::vector<std::string>& names) {
    std::sort(cells.begin(), cells.end(), [&](const VpCell& a, const VpCell& b) {
        if (a.chrom != b.chrom) return names[a.chrom] < names[b.chrom];
        return a.pbin < b.pbin;
    });
}
// name \t start \t end \t count for the partner cells given (already cut and in order)
inline std::string vp_partners_text(const std::vector<VpCell>& cells, const std::vector<std::string>& names, uint64_t pbin) {
    std::string out;
    for (const VpCell& c : cells)
        out += names[c.chrom] + "\t" + std::to_string((uint64_t)c.pbin * pbin) + "\t" + std::to_string((uint64_t)c.pbin * pbin + pbin) + "\t" + std::to_string(c.count) + "\n";
    return out;
}

// the results of the last mkt_matrix_viewpoint of a matrix object, on the host
struct VpState {
    std::vector<VpLink> links;
    std::vector<uint32_t> track;                  // bins 0 .. the largest occupied one
    std::vector<VpCell> partners;                 // count >= min_count, in (name, bin) order
    mkt_viewpoint_info info = {};
    double scan_ms = 0, sort_ms = 0;
    bool built = false;
};

}  // namespace mkt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace mkt {
constexpr uint32_t kVpLdsBins = 8192;             // viewpoint bins up to which the track is privatised in LDS (32 KiB per workgroup)
// The exact counts of a checked set of options over the n resident 16-byte records (MxRec as uint4: ia, pa, ib, pb); role: one byte
// per chromosome (0 none, 1 viewpoint, 2 partner).  Fills links, track, partners (cut and ordered), info and the two times; the hotspot
// cut is made here too.  Synchronises the stream.  MKT_OK, or MKT_E_CAPACITY / MKT_E_NOMEM / MKT_E_HIP / MKT_E_KERNEL with *why set.
int vp_run(VpState& s, const uint4* rec, uint64_t n, const std::vector<std::string>& names, const std::vector<uint32_t>& lens, const std::vector<uint8_t>& role,
           const mkt_viewpoint_opts& o, hipStream_t st, std::string* why);
}  // namespace mkt
#endif
