// pairsquery_main.cpp -- the `pairix file.pairs.gz REGION ...` of this project: region queries on a BGZF .pairs.gz through its .px2 on
// the GPU (mkt_bgzf_query of include/mkt.h has the definition).
//
//   pairsquery [-a] [-L] [-l] [-n] <in.pairs.gz> [region ...]
//
// Reads in.pairs.gz and in.pairs.gz.px2.  A region is 'chrA:b-e|chrB:b-e'; a side may lack its range or be '*'.  -a answers a pair that
// is absent while its flip is present flipped; -L takes files that list one region per line instead of regions; -l prints the pairs of
// the index, -n its line count.  Stdout for regions is pairix's, byte for byte.  Exit status 0, also when a pair is absent; 1 for
// usage or a refused region (the message names its index in the batch); 3 for a file or an index that is refused, with the reason
// and the block's offset.  Only the blocks the index points to are inflated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mkt.h"

static int usage(const char* a0) {
    fprintf(stderr, "\nUsage: %s [-a] [-L] [-l] [-n] <in.pairs.gz> [region ...]\n\nAnswers regions 'chrA:b-e|chrB:b-e' (a side may lack its range or be '*') from in.pairs.gz and\n"
                    "in.pairs.gz.px2 on the GPU, as pairix prints them.\n  -a  autoflip: answer an absent pair whose flip is present flipped\n  -L  the arguments are files that list one region per line\n"
                    "  -l  list the pairs of the index\n  -n  print the line count of the index\n\n", a0);
    return 1;
}
static bool slurp(const char* path, std::vector<char>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::vector<char> buf((size_t)8 << 20);
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), f)) > 0) out.insert(out.end(), buf.begin(), buf.begin() + (ptrdiff_t)got);
    fclose(f);
    return true;
}

int main(int argc, char* argv[]) {
    bool autoflip = false, lists = false, names = false, count = false;
    int a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1]; ++a) {
        for (const char* c = argv[a] + 1; *c; ++c) {
            if (*c == 'a') autoflip = true;
            else if (*c == 'L') lists = true;
            else if (*c == 'l') names = true;
            else if (*c == 'n') count = true;
            else return usage(argv[0]);
        }
    }
    if (a >= argc) return usage(argv[0]);
    const std::string in = argv[a++];
    std::vector<std::string> regions;
    for (; a < argc; ++a) {
        if (!lists) { regions.push_back(argv[a]); continue; }
        std::vector<char> t;
        if (!slurp(argv[a], t)) { fprintf(stderr, "Error: cannot read %s\n", argv[a]); return 1; }
        for (size_t p = 0; p < t.size();) {
            size_t q = p;
            while (q < t.size() && t[q] != '\n') ++q;
            if (q > p) regions.emplace_back(t.data() + p, q - p);
            p = q + 1;
        }
    }
    std::vector<char> gz, px;
    if (!slurp(in.c_str(), gz)) { fprintf(stderr, "Error: cannot read %s\n", in.c_str()); return 10; }
    if (!slurp((in + ".px2").c_str(), px)) { fprintf(stderr, "Error: cannot read %s.px2\n", in.c_str()); return 10; }
    const char* e = getenv("MKT_DEVICE");
    mkt_bgzf* p = nullptr;
    int rc = mkt_bgzf_create(e ? atoi(e) : 0, &p);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU query: %s\n", mkt_strerror(rc)); return 20; }
    auto fail = [&](const char* what) {
        fprintf(stderr, "Error: %s: %s: %s\n", what, mkt_strerror(rc), mkt_bgzf_error(p));
        const int status = rc == MKT_E_FORMAT ? 3 : rc == MKT_E_ARG ? 1 : 21;
        mkt_bgzf_destroy(p);
        return status;
    };
    if ((rc = mkt_bgzf_load_index(p, px.data(), px.size())) != MKT_OK) return fail((in + ".px2").c_str());
    if (count) {
        uint64_t n = 0;
        if ((rc = mkt_bgzf_count(p, &n)) != MKT_OK) return fail("count");
        printf("%llu\n", (unsigned long long)n);
    }
    if (names) {
        uint64_t total = 0;
        if ((rc = mkt_bgzf_names(p, 0, nullptr, 0, &total)) != MKT_OK) return fail("names");
        std::vector<char> nm(total + 1);
        if ((rc = mkt_bgzf_names(p, 0, nm.data(), total, nullptr)) != MKT_OK) return fail("names");
        for (uint64_t k = 0; k < total; ++k) putchar(nm[k] ? nm[k] : '\n');
    }
    if (!regions.empty()) {
        if ((rc = mkt_bgzf_add(p, gz.data(), gz.size())) != MKT_OK) return fail(in.c_str());
        std::vector<const char*> rp;
        for (const std::string& r : regions) rp.push_back(r.c_str());
        mkt_bgzf_query_opts o;
        memset(&o, 0, sizeof o);
        o.autoflip = autoflip ? 1u : 0u;
        mkt_bgzf_query_info info;
        if ((rc = mkt_bgzf_query(p, rp.data(), (uint32_t)rp.size(), &o, &info)) != MKT_OK) return fail(in.c_str());
        std::vector<char> buf((size_t)32 << 20);
        for (uint64_t off = 0; off < info.answer_bytes; off += buf.size()) {
            const size_t n = info.answer_bytes - off < buf.size() ? (size_t)(info.answer_bytes - off) : buf.size();
            if ((rc = mkt_bgzf_fetch_query(p, off, buf.data(), n)) != MKT_OK) return fail("fetch");
            if (fwrite(buf.data(), 1, n, stdout) != n) { fprintf(stderr, "Error: cannot write the output\n"); mkt_bgzf_destroy(p); return 11; }
        }
        fprintf(stderr, "pairsquery: %llu regions, %llu sub-queries, %llu chunks, %llu blocks (%llu bytes) inflated, %llu of %llu candidate lines answered%s\n", (unsigned long long)info.regions,
                (unsigned long long)info.subqueries, (unsigned long long)info.chunks, (unsigned long long)info.blocks_inflated, (unsigned long long)info.bytes_inflated, (unsigned long long)info.lines,
                (unsigned long long)info.candidate_lines, info.unparsed ? "; some lines unparsed" : "");
    }
    if (fflush(stdout)) { fprintf(stderr, "Error: cannot write the output\n"); mkt_bgzf_destroy(p); return 11; }
    mkt_bgzf_destroy(p);
    return 0;
}
