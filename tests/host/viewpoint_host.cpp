// viewpoint_host -- the host half of the viewpoint profiles (microcket_amd/csrc/mkt_viewpoint.h: the hotspot cut, the string order of
// the kept links and the three texts) on link tables from stdin, with no GPU and no HIP header.  tests/test_viewpoint_host.py feeds it
// the link tables of tests/viewpointdef.py and compares what it prints with the reference's texts.
//
// stdin, whitespace separated:  n_names  name ..  viewpoint_name  vbin  pbin  track_bin  min_count  total  ratio
//                               n_links  (vbin chrom pbin count) ..  n_track  count ..  n_cells  (chrom pbin count) ..
// stdout:  "min_loop <m> kept <k>\n", then the three texts, each behind a line "== <name> <bytes>".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../microcket_amd/csrc/mkt_viewpoint.h"

int main() {
    using namespace mkt;
    size_t nn = 0;
    if (!(std::cin >> nn)) return 2;
    std::vector<std::string> names(nn);
    for (std::string& s : names) std::cin >> s;
    std::string vname;
    uint64_t vbin = 0, pbin = 0, tbin = 0, total = 0;
    uint32_t min_count = 0;
    double ratio = 0;
    std::string rs;
    std::cin >> vname >> vbin >> pbin >> tbin >> min_count >> total >> rs;
    ratio = strtod(rs.c_str(), nullptr);
    size_t nl = 0;
    std::cin >> nl;
    std::vector<VpLink> links(nl);
    for (VpLink& l : links) std::cin >> l.vbin >> l.chrom >> l.pbin >> l.count;
    size_t nt = 0;
    std::cin >> nt;
    std::vector<uint32_t> track(nt);
    for (uint32_t& c : track) std::cin >> c;
    size_t nc = 0;
    std::cin >> nc;
    std::vector<VpCell> cells(nc);
    for (VpCell& c : cells) std::cin >> c.chrom >> c.pbin >> c.count;
    if (!std::cin) return 2;
    for (const VpLink& l : links) if (l.chrom >= nn) return 2;
    for (const VpCell& c : cells) if (c.chrom >= nn) return 2;
    if (!track.empty() && !vp_links_fit(track.size() - 1, vbin)) { fprintf(stderr, "the links text does not fit 63 bits\n"); return 3; }

    const uint32_t min_loop = vp_min_loop(links, total, ratio);
    printf("min_loop %u kept %zu\n", min_loop, vp_kept_links(links, names, min_loop).size());
    vp_sort_partners(cells, names);
    std::vector<VpCell> kept;
    for (const VpCell& c : cells) if (c.count >= min_count) kept.push_back(c);
    const std::string texts[3] = {vp_track_text(track, vname, vbin), vp_links_text(links, names, min_loop, vbin, pbin), vp_partners_text(kept, names, tbin)};
    static const char* const label[3] = {"bedgraph", "links", "partners"};
    for (int k = 0; k < 3; ++k) {
        printf("== %s %zu\n", label[k], texts[k].size());
        fwrite(texts[k].data(), 1, texts[k].size(), stdout);
    }
    return 0;
}
