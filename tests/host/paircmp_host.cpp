// paircmp_host -- stand-alone driver of the host half of the pair comparison (microcket_amd/csrc/mkt_paircmp.h): the report and the
// exact grouping by id string that the library applies to runs of records whose keys collide.  No GPU, no HIP.
//
//   paircmp_host <a.pairs> <b.pairs> <max_dist> <bits> <name a> <name b>
//
// The lines are parsed here (the library parses them on the device), put into 2^bits runs by a hash of their id -- A lines in file
// order, then B lines in file order, as the library's stable sort leaves a run -- and every run goes through pc_resolve.  Output: the
// line "classes A <n>", n class digits, a newline, the same for B, and then the report.  Exit 3 for a line outside the domain.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../microcket_amd/csrc/mkt_paircmp.h"

using namespace mkt;

static bool slurp(const char* fn, std::string& out) {
    FILE* f = fopen(fn, "rb");
    if (!f) return false;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    fclose(f);
    return true;
}

struct Side { std::string text; std::vector<size_t> start; std::vector<PcLine> ln; };

static bool number(const std::string& t, size_t a, size_t b, uint32_t& out) {
    if (a >= b) return false;
    uint64_t v = 0;
    for (size_t q = a; q < b; ++q) {
        if (t[q] < '0' || t[q] > '9') return false;
        v = v * 10 + (uint64_t)(t[q] - '0');
        if (v > 0x7FFFFFFFull) return false;
    }
    out = (uint32_t)v;
    return true;
}

static int parse(Side& s, const char* name, mkt_paircmp_info& info, int side) {
    if (!s.text.empty() && s.text.back() != '\n') s.text += '\n';
    for (size_t p = 0; p < s.text.size();) {
        const size_t e = s.text.find('\n', p);
        PcLine L = {0, 0, 0, 0, 0, 0, 0, 0};
        if (!(e > p && s.text[p] == '#')) {
            uint32_t tabs[5];
            int nt = 0;
            for (size_t q = p; q < e && nt < 5; ++q) if (s.text[q] == '\t') tabs[nt++] = (uint32_t)(q - p);
            bool ok = nt >= 4;
            if (ok) {
                L.t0 = tabs[0]; L.t1 = tabs[1]; L.t2 = tabs[2]; L.t3 = tabs[3]; L.e5 = nt == 5 ? tabs[4] : (uint32_t)(e - p);
                ok = number(s.text, p + L.t1 + 1, p + L.t2, L.p1) && number(s.text, p + L.t3 + 1, p + L.e5, L.p2);
            }
            if (!ok) { fprintf(stderr, "file %s line %zu is outside the domain\n", name, s.start.size() + 1); return 3; }
            L.data = 1;
            const PcItem it = {0, 0, s.text.data() + p, L};
            int cls = 3;
            if (pc_same(it.c1(), it.c1_len(), it.c2(), it.c2_len())) { const uint32_t d = pc_absdiff(L.p1, L.p2); cls = d > 10000u ? 2 : d < 1000u ? 0 : 1; }
            ++info.dist[side][cls];
            ++info.data_lines[side];
        }
        s.start.push_back(p);
        s.ln.push_back(L);
        p = e + 1;
    }
    info.lines[side] = s.start.size();
    return 0;
}

int main(int argc, char* argv[]) {
    if (argc != 7) { fprintf(stderr, "usage: %s a.pairs b.pairs max_dist bits name_a name_b\n", argv[0]); return 2; }
    Side s[2];
    if (!slurp(argv[1], s[0].text) || !slurp(argv[2], s[1].text)) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
    const uint32_t max_dist = (uint32_t)strtoul(argv[3], nullptr, 10);
    const int bits = atoi(argv[4]);
    mkt_paircmp_info info;
    memset(&info, 0, sizeof info);
    for (int k = 0; k < 2; ++k) if (int rc = parse(s[k], k ? "B" : "A", info, k)) return rc;
    const size_t nA = s[0].start.size();
    std::vector<std::vector<PcItem>> runs((size_t)1 << bits);
    for (int k = 0; k < 2; ++k)
        for (size_t j = 0; j < s[k].start.size(); ++j) {
            if (!s[k].ln[j].data) continue;
            const PcItem it = {(uint32_t)(k ? nA + j : j), (uint32_t)k, s[k].text.data() + s[k].start[j], s[k].ln[j]};
            uint32_t h = 0x811c9dc5u;
            for (uint32_t q = 0; q < it.id_len(); ++q) h = (h ^ (uint8_t)it.id()[q]) * 16777619u;
            runs[(h ^ (h >> 15)) & (((size_t)1 << bits) - 1)].push_back(it);
        }
    std::vector<uint8_t> cls(nA + s[1].start.size(), PC_COMMENT), c;
    std::vector<uint32_t> partner;
    for (const auto& run : runs) {
        pc_resolve(run, pc_dist(max_dist), c, partner);
        for (size_t k = 0; k < run.size(); ++k) {
            cls[run[k].line] = c[k];
            if ((c[k] == PC_CONSISTENT || c[k] == PC_DISCORDANT) && run[k].side == 1 && (partner[k] >= nA || cls[partner[k]] != c[k])) { fprintf(stderr, "partner of line %u\n", run[k].line); return 4; }
        }
    }
    pc_count_classes(cls.data(), nA, cls.data() + nA, cls.size() - nA, info);
    for (int k = 0; k < 2; ++k) {
        const size_t n = s[k].start.size();
        printf("classes %s %zu\n", k ? "B" : "A", n);
        for (size_t j = 0; j < n; ++j) putchar('0' + cls[(k ? nA : 0) + j]);
        putchar('\n');
    }
    fputs(pc_report(info, max_dist, argv[5], argv[6]).c_str(), stdout);
    return 0;
}
