// pairsbgz_main.cpp -- the driver's `bgzip -c final.pairs > final.pairs.gz; pairix final.pairs.gz` on the GPU: writes the BGZF file
// and its pairix index <out>.px2 (mkt_pairsgz_* of include/mkt.h has the definition).
//
//   pairsbgz [-l LEVEL] [-f] <final.pairs | -> <out.pairs.gz>
//
// -l 0 stored, 1 the fixed code (default), 2 a code per block.  An index that exists is not overwritten without -f, as with pairix.
// Nothing is written when the text is refused (unsorted, a pair that reappears, a malformed line): the message names the line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_chunked_file.h"

static int usage(const char* a0) {
    fprintf(stderr, "\nUsage: %s [-l LEVEL] [-f] <final.pairs | -> <out.pairs.gz>\n\nWrites out.pairs.gz (BGZF) and out.pairs.gz.px2 (the pairix index, preset pairs).\n"
                    "  -l LEVEL  0 stored, 1 fixed code (default), 2 a code per block\n  -f        overwrite an index that exists\nThe text is held in GPU memory; .gz input is not read.\n\n", a0);
    return 2;
}
static bool ends_gz(const char* s) { const size_t n = strlen(s); return n >= 3 && !strcmp(s + n - 3, ".gz"); }

int main(int argc, char* argv[]) {
    int level = 1, k = 1;
    bool force = false;
    for (; k < argc && argv[k][0] == '-' && argv[k][1]; ++k) {
        if (!strcmp(argv[k], "-f")) force = true;
        else if (!strcmp(argv[k], "-l") && k + 1 < argc) {
            char* end = nullptr;
            const long v = strtol(argv[++k], &end, 10);
            if (*end || end == argv[k] || v < 0 || v > 2) { fprintf(stderr, "Error: level '%s': 0, 1 or 2.\n", argv[k]); return 3; }
            level = (int)v;
        } else return usage(argv[0]);
    }
    if (argc - k != 2) return usage(argv[0]);
    const char* in = argv[k];
    const std::string out = argv[k + 1], outx = out + ".px2";
    if (ends_gz(in)) { fprintf(stderr, "Error: %s: .gz files are not read (this project has no GPU inflate); decompress first.\n", in); return 3; }
    if (!force) {
        if (FILE* f = fopen(outx.c_str(), "rb")) { fclose(f); fprintf(stderr, "Error: the index %s exists; use -f to overwrite it.\n", outx.c_str()); return 4; }
    }
    const char* e = getenv("MKT_DEVICE");
    mkt_pairsgz* p = nullptr;
    int rc = mkt_pairsgz_create(e ? atoi(e) : 0, &p);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU pairs.gz writer: %s\n", mkt_strerror(rc)); return 20; }
    std::vector<char> buf((size_t)32 << 20);
    FILE* f = strcmp(in, "-") ? fopen(in, "rb") : stdin;
    if (!f) { fprintf(stderr, "Error: cannot read %s\n", in); return 10; }
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), f)) > 0)
        if ((rc = mkt_pairsgz_add(p, buf.data(), got)) != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_pairsgz_error(p)); return 21; }
    if (f != stdin) fclose(f);
    mkt_pairsgz_opts o;
    mkt_pairsgz_opts_default(&o);
    o.level = level;
    mkt_pairsgz_info info;
    rc = mkt_pairsgz_run(p, &o, &info);
    if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_pairsgz_error(p)); mkt_pairsgz_destroy(p); return 21; }
    for (int which = 0; which < 2; ++which) {
        const std::string& fn = which ? outx : out;
        const uint64_t total = which ? info.px2_bytes : info.gz_bytes;
        mkt::ChunkedFile w(fn.c_str());
        for (uint64_t off = 0; off < total; off += buf.size()) {
            const size_t n = total - off < buf.size() ? (size_t)(total - off) : buf.size();
            rc = which ? mkt_pairsgz_fetch_px2(p, off, buf.data(), n) : mkt_pairsgz_fetch_gz(p, off, buf.data(), n);
            if (rc != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_pairsgz_error(p)); return 21; }
            if (!w.append(buf.data(), n)) break;
        }
        if (!w.finish()) { fprintf(stderr, "Error: cannot write %s\n", fn.c_str()); return 11; }
    }
    fprintf(stderr, "pairsbgz: %llu lines, %llu records, %llu pairs, %llu chunks; %llu blocks, %llu + %llu bytes\n", (unsigned long long)info.lines, (unsigned long long)info.records,
            (unsigned long long)info.names, (unsigned long long)info.chunks, (unsigned long long)info.blocks, (unsigned long long)info.gz_bytes, (unsigned long long)info.px2_bytes);
    mkt_pairsgz_destroy(p);
    return 0;
}
