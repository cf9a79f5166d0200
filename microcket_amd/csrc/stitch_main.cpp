// stitch_main.cpp -- bin/stitch: drop-in for the driver's read stitching step (microcket:405-408, 430-438, and the probe at 371-373)
//     flash -q --interleaved-input -m 10 -M 150 -t T -To -c - | perl deal.flash.pl - PREFIX
// ->  stitch -o PREFIX -
// Interleaved FASTQ in (a file or "-"); out PREFIX.ext.fq, PREFIX.cut.read1.fq, PREFIX.cut.read2.fq and PREFIX.stitch.stat, or with
// --tab FLASH's tab-delimited lines on stdout; always "Percent combined: <pct>%" on stderr.  Everything is in input order.  The
// stitching runs on the GPU behind mkt_stitch_* (include/mkt.h); this file only moves bytes.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>
#include "../../include/mkt.h"

static void usage(const char* prg) {
    fprintf(stderr, "\nUsage: %s [-m 10] [-M 150] [-x 0.25] [-p 33] [--cut-tail 10] [--min-size 36] -o PREFIX [--tab] <interleaved.fq | ->\n"
                    "\nRead stitching on the GPU (MI355X build): FLASH's innie combination (-m min overlap, -M max overlap, -x max mismatch\n"
                    "density, -p phred offset) and deal.flash.pl's split of the result into PREFIX.ext.fq, PREFIX.cut.read1.fq,\n"
                    "PREFIX.cut.read2.fq and PREFIX.stitch.stat.  --tab: FLASH's tab-delimited lines on stdout instead (-o not needed).\n\n", prg);
    exit(2);
}
static bool write_all(int fd, const char* p, size_t n) {
    while (n) {
        const ssize_t k = write(fd, p, n);
        if (k < 0) { if (errno == EINTR) continue; return false; }
        p += k; n -= (size_t)k;
    }
    return true;
}
static bool number(const char* a, double* v) {
    char* end = nullptr;
    errno = 0;
    *v = strtod(a, &end);
    return end != a && *end == 0 && errno == 0;
}

int main(int argc, char* argv[]) {
    double m = 10, M = 150, x = 0.25, phred = 33, cut = 10, minsz = 36;
    const char* prefix = nullptr;
    int tab = 0;
    static const option longopts[] = {{"cut-tail", required_argument, nullptr, 1}, {"min-size", required_argument, nullptr, 2}, {"tab", no_argument, nullptr, 3},
                                      {nullptr, 0, nullptr, 0}};
    int opt;
    while ((opt = getopt_long(argc, argv, "m:M:x:p:o:", longopts, nullptr)) != -1) {
        double* dst = nullptr;
        switch (opt) {
        case 'm': dst = &m; break;
        case 'M': dst = &M; break;
        case 'x': dst = &x; break;
        case 'p': dst = &phred; break;
        case 1: dst = &cut; break;
        case 2: dst = &minsz; break;
        case 3: tab = 1; break;
        case 'o': prefix = optarg; break;
        default: usage(argv[0]);
        }
        if (dst && !number(optarg, dst)) { fprintf(stderr, "Error: '%s' is not a number\n", optarg); return 1; }
    }
    if (optind + 1 != argc || (!prefix && !tab)) usage(argv[0]);
    const char* in = argv[optind];
    auto whole = [](double v) { return v >= 0 && v <= 4294967295.0 && v == (double)(uint32_t)v; };
    if (!whole(m) || !whole(M) || !whole(phred) || !whole(cut) || !whole(minsz)) { fprintf(stderr, "Error: -m, -M, -p, --cut-tail and --min-size take whole numbers\n"); return 1; }
    char msg[256];
    if (mkt_stitch_check((uint32_t)m, (uint32_t)M, x, (uint32_t)phred, (uint32_t)cut, (uint32_t)minsz, msg, sizeof msg) != MKT_OK) { fprintf(stderr, "Error: %s\n", msg); return 1; }
    FILE* fin = fopen((in[0] == '-' && in[1] == '\0') ? "/dev/stdin" : in, "rb");
    if (!fin) { fprintf(stderr, "Error: read fastq failed!\n"); return 10; }
    FILE* fo[4] = {nullptr, nullptr, nullptr, nullptr};
    if (!tab) {
        static const char* const ext[4] = {"", ".ext.fq", ".cut.read1.fq", ".cut.read2.fq"};
        for (int k = 1; k < 4; ++k) {
            fo[k] = fopen((std::string(prefix) + ext[k]).c_str(), "wb");
            if (!fo[k]) { fprintf(stderr, "Error: open output files failed!\n"); return 11; }
        }
    }
    const char* e = getenv("MKT_DEVICE");
    mkt_stitch* s = nullptr;
    int rc = mkt_stitch_create(e ? atoi(e) : 0, &s);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU context: %s\n", mkt_strerror(rc)); return 20; }
    rc = mkt_stitch_begin(s, (uint32_t)m, (uint32_t)M, x, (uint32_t)phred, (uint32_t)cut, (uint32_t)minsz);
    if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_stitch_error(s)); return 21; }
    std::vector<char> buf((size_t)64 << 20);
    uint64_t ob[4];
    auto drain = [&]() -> bool {                                    // what the last push left in the streams
        for (int which = tab ? 0 : 1; which < (tab ? 1 : 4); ++which) {
            const int fd = tab ? 1 : fileno(fo[which]);
            for (uint64_t off = 0; off < ob[which]; off += buf.size()) {
                const size_t n = ob[which] - off < buf.size() ? (size_t)(ob[which] - off) : buf.size();
                if (mkt_stitch_fetch(s, which, off, buf.data(), n) != MKT_OK || !write_all(fd, buf.data(), n)) return false;
            }
        }
        return true;
    };
    // a regular file is read in 64 MiB pieces; a pipe in pieces of at most 4 MiB of what has arrived
    const int ifd = fileno(fin);
    size_t piece = (size_t)4 << 20;
    { struct stat sb; if (fstat(ifd, &sb) == 0 && S_ISREG(sb.st_mode)) piece = buf.size(); }
    for (;;) {
        size_t k = 0;
        while (k < piece) {
            const ssize_t g = read(ifd, buf.data() + k, piece - k);
            if (g < 0) { if (errno == EINTR) continue; fprintf(stderr, "Error: read fastq failed!\n"); return 10; }
            if (g == 0) break;
            k += (size_t)g;
        }
        rc = mkt_stitch_push(s, buf.data(), k, k == 0 ? 1 : 0, ob);
        if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_stitch_error(s)); return 21; }
        if ((ob[0] | ob[1] | ob[2] | ob[3]) && !drain()) { fprintf(stderr, "Error: write output failed!\n"); return 22; }
        if (k == 0) break;
    }
    fclose(fin);
    for (int k = 1; k < 4; ++k) if (fo[k] && fclose(fo[k]) != 0) { fprintf(stderr, "Error: write output failed!\n"); return 22; }
    uint64_t total = 0, comb = 0, unc = 0, pass = 0;
    mkt_stitch_stats(s, &total, &comb, &unc, &pass);
    if (!tab) {
        FILE* fs = fopen((std::string(prefix) + ".stitch.stat").c_str(), "wb");
        if (!fs) { fprintf(stderr, "Error: write stat failed!\n"); return 11; }
        fprintf(fs, "Combined\t%llu\tUncombined\t%llu\tPass\t%llu\n", (unsigned long long)comb, (unsigned long long)unc, (unsigned long long)pass);
        if (fclose(fs) != 0) { fprintf(stderr, "Error: write stat failed!\n"); return 22; }
    }
    fprintf(stderr, "Percent combined: %.2f%%\n", total ? 100.0 * (double)comb / (double)total : 0.0);
    mkt_stitch_destroy(s);
    return 0;
}
