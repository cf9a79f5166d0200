// pairscmp_main.cpp -- the reference's benchmarking/check.consistency.pl on the GPU: joins two .pairs files by read name and counts
// the reads that both placed at the same two loci within a distance (mkt_paircmp_* of include/mkt.h has the definition).
//
//   pairscmp <a.pairs> <b.pairs> [dist=200] [inconsistent]        ("-" reads one side from stdin)
//
// stdout is the script's, byte for byte; with a fourth argument the discordant, B-only and A-only records go to that file.  The
// script's pigz / gzip pipes for names ending in .gz are not offered: the project has no GPU inflate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_chunked_file.h"

static bool ends_gz(const char* s) { const size_t n = strlen(s); return n >= 3 && !strcmp(s + n - 3, ".gz"); }

int main(int argc, char* argv[]) {
    if (argc < 3) {
        fprintf(stderr, "\nUsage: %s <a.pairs> <b.pairs> [dist=200] [inconsistent]\n\nNOTE: Numbers are reported in millions.\nBoth files are held in GPU memory; '-' reads one of them from stdin.\n\n", argv[0]);
        return 2;
    }
    for (int k : {1, 2, 4}) if (k < argc && ends_gz(argv[k])) {
        fprintf(stderr, "Error: %s: .gz files are not read or written (this project has no GPU inflate); decompress first.\n", argv[k]);
        return 3;
    }
    if (!strcmp(argv[1], "-") && !strcmp(argv[2], "-")) { fprintf(stderr, "Error: only one side can come from stdin.\n"); return 3; }
    uint32_t dist = 0;                                   // 0: the default, as the script's `$ARGV[2] || 200`
    if (argc > 3 && argv[3][0]) {
        char* end = nullptr;
        const unsigned long long v = strtoull(argv[3], &end, 10);
        if (*end || argv[3][0] == '-' || argv[3][0] == '+' || v > 0xFFFFFFFFull) { fprintf(stderr, "Error: dist '%s' is not a non-negative integer.\n", argv[3]); return 3; }
        dist = (uint32_t)v;
    }
    const char* e = getenv("MKT_DEVICE");
    mkt_paircmp* p = nullptr;
    int rc = mkt_paircmp_create(e ? atoi(e) : 0, &p);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU pair comparison: %s\n", mkt_strerror(rc)); return 20; }
    std::vector<char> buf((size_t)32 << 20);
    for (int s = 0; s < 2; ++s) {
        const char* fn = argv[1 + s];
        FILE* f = strcmp(fn, "-") ? fopen(fn, "rb") : stdin;
        if (!f) { fprintf(stderr, "Error: cannot read %s\n", fn); return 10; }
        size_t k;
        while ((k = fread(buf.data(), 1, buf.size(), f)) > 0)
            if ((rc = mkt_paircmp_add(p, s, buf.data(), k)) != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_paircmp_error(p)); return 21; }
        if (f != stdin) fclose(f);
    }
    mkt_paircmp_opts o;
    mkt_paircmp_opts_default(&o);
    o.max_dist = dist;
    o.want_lines = argc > 4 ? 1 : 0;
    mkt_paircmp_info info;
    rc = mkt_paircmp_run(p, &o, &info);
    if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_paircmp_error(p)); return 21; }
    if (argc > 4) {
        mkt::ChunkedFile out(argv[4]);
        for (uint64_t off = 0; off < info.lines_bytes; off += buf.size()) {
            const size_t k = info.lines_bytes - off < buf.size() ? (size_t)(info.lines_bytes - off) : buf.size();
            if (mkt_paircmp_fetch_lines(p, off, buf.data(), k) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_paircmp_error(p)); return 21; }
            if (!out.append(buf.data(), k)) break;
        }
        if (!out.finish()) { fprintf(stderr, "Error: cannot write %s\n", argv[4]); return 11; }
    }
    std::vector<char> rep(4096 + strlen(argv[1]) + strlen(argv[2]));
    const long n = mkt_paircmp_report(&info, dist, argv[1], argv[2], rep.data(), rep.size());
    if (n < 0 || fwrite(rep.data(), 1, (size_t)n, stdout) != (size_t)n) { fprintf(stderr, "Error: write output failed!\n"); return 22; }
    mkt_paircmp_destroy(p);
    return 0;
}
