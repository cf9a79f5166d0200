// pairstat_host -- stand-alone driver of the host and shared half of the pair statistics (microcket_amd/csrc/mkt_pairstat.h): the parse
// and the classes of a line as the kernels apply them, the areas, P(s), the convergence rule and the two texts.  No GPU, no HIP.
//
//   pairstat_host <chrom.sizes> <in.pairs> <tol_permille> <min_count> <out prefix>
//
// Writes <prefix>.pairs.stat and <prefix>.scaling.tsv; prints the counters as "key value" lines, the 74 x 4 distance cells, and the bit
// patterns of area and P as hexadecimal words.  Exit 3 with "line N" on stderr for a refused line, 4 for a refused table, 5 for a table
// of more than 2048 names.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../microcket_amd/csrc/mkt_pairstat.h"

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
static bool spill(const std::string& fn, const std::string& s) {
    FILE* f = fopen(fn.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    return fclose(f) == 0 && ok;
}

int main(int argc, char* argv[]) {
    if (argc != 6) { fprintf(stderr, "usage: %s chrom.sizes in.pairs tol_permille min_count prefix\n", argv[0]); return 2; }
    std::string ttxt, text;
    if (!slurp(argv[1], ttxt) || !slurp(argv[2], text)) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    const std::string bad = mx_parse_table(ttxt.data(), ttxt.size(), names, lens);
    if (names.size() > kPsMaxChrom) { fprintf(stderr, "%zu names\n", names.size()); return 5; }
    if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 4; }
    const uint32_t n = (uint32_t)names.size();
    std::vector<MxTab> tab(1);
    memset(tab.data(), 0, sizeof(MxTab));
    mx_tab_fill(tab.data(), names, lens);
    if (!text.empty() && text.back() != '\n') text += '\n';
    std::vector<uint64_t> ctr(kPsCells, 0), chrom((size_t)n * n, 0);
    const uint8_t* t = reinterpret_cast<const uint8_t*>(text.data());
    size_t number = 0;
    for (size_t p = 0; p < text.size();) {
        const size_t e = text.find('\n', p);
        ++number;
        const PsClass c = ps_parse_line(t, p, e, tab.data(), n);
        if (c.kind == PS_K_BAD) { fprintf(stderr, "line %zu\n", number); return 3; }
        ps_count_host(c, ctr.data(), chrom.data());
        p = e + 1;
    }
    PsResult R;
    ps_finish(ctr.data(), chrom.data(), names, lens, (uint32_t)strtoul(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), R);
    const mkt_pairstat_info& I = R.info;
    printf("total %llu\nskipped %llu\ncounted %llu\ncis %llu\ntrans %llu\nno_strand %llu\nheader_lines %llu\n", (unsigned long long)I.total, (unsigned long long)I.skipped,
           (unsigned long long)I.counted, (unsigned long long)I.cis, (unsigned long long)I.trans, (unsigned long long)I.no_strand, (unsigned long long)I.header_lines);
    for (int k = 0; k < 6; ++k) printf("cis_ge%d %llu\n", k, (unsigned long long)I.cis_ge[k]);
    printf("cis0 %llu\ncis1K %llu\ncis10K %llu\nref_trans %llu\nconvergence_dist %lld\n", (unsigned long long)I.cis0, (unsigned long long)I.cis1K, (unsigned long long)I.cis10K,
           (unsigned long long)I.ref_trans, (long long)I.convergence_dist);
    printf("dist");
    for (int k = 0; k < kPsDistCells; ++k) printf(" %llu", (unsigned long long)ctr[k]);
    printf("\narea");
    for (int k = 0; k < kPsBins; ++k) { uint64_t w; memcpy(&w, &R.area_d[k], 8); printf(" %016llx", (unsigned long long)w); }
    printf("\nP");
    for (int k = 0; k < kPsBins; ++k) { uint64_t w; memcpy(&w, &R.p[k], 8); printf(" %016llx", (unsigned long long)w); }
    printf("\n");
    if (!spill(std::string(argv[5]) + ".pairs.stat", R.stat) || !spill(std::string(argv[5]) + ".scaling.tsv", R.scaling)) { fprintf(stderr, "cannot write\n"); return 2; }
    return 0;
}
