// pairsquery_host.cpp -- stand-alone driver of the host and shared half of the region queries (microcket_amd/csrc/mkt_px2query.h): the
// region grammar, the index kept by px2_parse, the block plan with its compact buffer, and the line filter the kernel runs, serially.
// Members are inflated with inf_member_serial (mkt_inflate.h), only those of the plan.  No GPU, no HIP header.
//
//   pairsquery_host [-a] <in.pairs.gz> <in.pairs.gz.px2> <regions.txt: one region per line>
//
// stdout: "members <k> <k> ...\n", "runs <n>\n", "candidates <n> unparsed <n>\n", then per region "region <i> <lines>\n" and its lines;
// or "refused arg <message>\n" / "refused format <message>\n" alone.  Exit status 0 either way; 2 for a file that cannot be read.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../microcket_amd/csrc/mkt_px2query.h"

using namespace mkt;

static bool slurp(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}
// member k of gz into out[0, isize): 0, or the reason
static uint32_t inflate_member(const std::vector<uint8_t>& gz, const InfBlock& b, uint8_t* out) {
    const uint32_t nspan = b.bsize - kInfHead - kInfFoot;
    std::vector<uint8_t> span(nspan + kInfSpanPad, 0);
    if (nspan) memcpy(span.data(), gz.data() + b.coff + kInfHead, nspan);
    uint64_t kinds[3] = {0, 0, 0};
    return inf_member_serial(span.data(), nspan, out, b.isize, kinds);
}

int main(int argc, char** argv) {
    bool autoflip = false;
    int a0 = 1;
    if (argc > 1 && !strcmp(argv[1], "-a")) { autoflip = true; a0 = 2; }
    if (argc - a0 != 3) return 2;
    std::vector<uint8_t> gz, px, rg;
    if (!slurp(argv[a0], gz) || !slurp(argv[a0 + 1], px) || !slurp(argv[a0 + 2], rg)) return 2;
    std::vector<std::string> regions;
    for (size_t p = 0; p < rg.size();) {
        size_t q = p;
        while (q < rg.size() && rg[q] != '\n') ++q;
        regions.emplace_back((const char*)rg.data() + p, q - p);
        p = q + 1;
    }
    std::vector<const char*> rp;
    for (const std::string& r : regions) rp.push_back(r.c_str());

    std::vector<InfBlock> blocks, xblocks;
    uint64_t bad = 0;
    bool has_eof = false;
    if (uint32_t r = inf_block_table(px.data(), px.size(), xblocks, &bad, &has_eof)) { printf("refused format the index: %s\n", inf_reason_key(r)); return 0; }
    std::vector<uint8_t> d(1);
    for (const InfBlock& b : xblocks) {
        const size_t at = d.size() - 1;
        d.resize(d.size() + b.isize);
        if (uint32_t r = inflate_member(px, b, d.data() + at)) { printf("refused format the index: %s\n", inf_reason_key(r)); return 0; }
    }
    Px2Index ix;
    std::string err;
    if (!px2_parse(d.data(), d.size() - 1, ix, err)) { printf("refused format %s\n", err.c_str()); return 0; }
    if (uint32_t r = inf_block_table(gz.data(), gz.size(), blocks, &bad, &has_eof)) { printf("refused format the file: %s\n", inf_reason_key(r)); return 0; }
    if (!q_index_belongs(ix, blocks, gz.size())) { printf("refused format the index does not belong to this file\n"); return 0; }

    QPlan P;
    const int rc = q_plan(ix, blocks, gz.size(), rp.data(), (uint32_t)rp.size(), autoflip, P, err);
    if (rc) { printf("refused %s %s\n", rc == 1 ? "arg" : "format", err.c_str()); return 0; }
    q_layout(P, blocks, false);
    std::vector<uint8_t> text(P.compact_bytes);           // an exact size: a read outside a span is the sanitizer's to find
    for (size_t j = 0; j < P.members.size(); ++j)
        if (uint32_t r = inflate_member(gz, blocks[P.members[j]], text.data() + P.tbase[j])) { printf("refused format the file: %s\n", inf_reason_key(r)); return 0; }

    std::vector<std::string> answers(regions.size());
    std::vector<uint64_t> counts(regions.size(), 0);
    uint64_t cand = 0, unparsed = 0;
    for (const QSpan& s : P.spans) {
        const QSub& q = P.subs[s.sub];
        const uint8_t* A = (const uint8_t*)ix.names.data() + q.a_off;
        const uint8_t* B = (const uint8_t*)ix.names.data() + q.b_off;
        for (uint64_t p = s.lo; p < s.hi;) {
            uint64_t e = p;
            while (e < s.hi && text[e] != '\n') ++e;
            ++cand;
            const uint32_t m = q_match_line(text.data() + p, e - p, A, q.a_len, B, q.b_len, q.b1, q.e1, q.b2, q.e2);
            unparsed += m == 2;
            if (m == 1) { answers[q.region].append((const char*)text.data() + p, e - p); answers[q.region] += '\n'; ++counts[q.region]; }
            p = e + 1;
        }
    }
    printf("members");
    for (uint32_t k : P.members) printf(" %u", k);
    printf("\nruns %llu\ncandidates %llu unparsed %llu\n", (unsigned long long)P.runs, (unsigned long long)cand, (unsigned long long)unparsed);
    for (size_t r = 0; r < regions.size(); ++r) {
        printf("region %zu %llu\n", r, (unsigned long long)counts[r]);
        fwrite(answers[r].data(), 1, answers[r].size(), stdout);
    }
    return 0;
}
