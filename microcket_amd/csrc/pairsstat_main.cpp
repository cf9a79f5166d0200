// pairsstat -- pair-level QC of a .pairs file on the GPU: totals, distance thresholds, the reference's cis0 / cis1K / cis10K / trans,
// chromosome-pair counts, distance by strand orientation and the contact-probability curve P(s) (include/mkt.h has the definition).
//
//   pairsstat -g <chrom.sizes> [-o PREFIX] [--tol N] [--min-count N] <final.pairs | final.pairs.gz | ->      ($MKT_DEVICE: GPU ordinal)
//
// With -o: PREFIX.pairs.stat and PREFIX.scaling.tsv are written; without it the statistics go to stdout.  An input that begins with
// the gzip magic bytes is read as BGZF, inflated on the device (mkt_bgzf_*) and handed over there; plain text is streamed in pieces, so
// stdin and files larger than the device memory work.
// Exit codes: 0; 2 usage; 10 an input cannot be read; 11 an output cannot be written; 12 refused input (the table, a line, a BGZF
// block); 20 no GPU; 21 any other failure of the library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/mkt.h"

static int usage() {
    fprintf(stderr, "Usage: pairsstat -g <chrom.sizes> [-o PREFIX] [--tol PERMILLE] [--min-count N] <final.pairs | final.pairs.gz | ->\n");
    return 2;
}
static bool slurp(const char* fn, std::string& out) {
    FILE* f = fopen(fn, "rb");
    if (!f) return false;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    const bool ok = !ferror(f);
    fclose(f);
    return ok;
}
static bool number(const char* s, unsigned long long& v) {
    if (!s || !*s) return false;
    char* end = nullptr;
    v = strtoull(s, &end, 10);
    return *end == 0 && s[0] >= '0' && s[0] <= '9';
}
struct Stat {                                         // owns the two library objects and the input
    mkt_pairstat* p = nullptr;
    mkt_bgzf* z = nullptr;
    FILE* f = nullptr;
    ~Stat() {
        if (p) mkt_pairstat_destroy(p);
        if (z) mkt_bgzf_destroy(z);
        if (f && f != stdin) fclose(f);
    }
};
static int lib_fail(const Stat& S, int rc, const char* what) {
    fprintf(stderr, "Error: %s: %s: %s\n", what, mkt_strerror(rc), mkt_pairstat_error(S.p));
    return rc == MKT_E_FORMAT || rc == MKT_E_ARG || rc == MKT_E_RANGE ? 12 : 21;
}
static int write_text(Stat& S, int which, const std::string& fn) {
    const long n = mkt_pairstat_text(S.p, which, nullptr, 0);
    if (n < 0) return lib_fail(S, (int)n, "GPU statistics");
    std::string s((size_t)n, '\0');
    if (n && mkt_pairstat_text(S.p, which, &s[0], s.size()) != n) return lib_fail(S, MKT_E_STATE, "GPU statistics");
    FILE* o = fn.empty() ? stdout : fopen(fn.c_str(), "wb");
    if (!o) { fprintf(stderr, "Error: cannot write %s\n", fn.c_str()); return 11; }
    const bool ok = fwrite(s.data(), 1, s.size(), o) == s.size() && fflush(o) == 0;
    if (o != stdout) fclose(o);
    if (!ok) { fprintf(stderr, "Error: cannot write %s\n", fn.empty() ? "stdout" : fn.c_str()); return 11; }
    return 0;
}

int main(int argc, char* argv[]) {
    const char *table = nullptr, *prefix = nullptr, *in = nullptr;
    mkt_pairstat_opts o;
    mkt_pairstat_opts_default(&o);
    for (int k = 1; k < argc; ++k) {
        const std::string a = argv[k];
        unsigned long long v = 0;
        if (a == "-g" && k + 1 < argc) table = argv[++k];
        else if (a == "-o" && k + 1 < argc) prefix = argv[++k];
        else if (a == "--tol" && k + 1 < argc) { if (!number(argv[++k], v) || v > 0xFFFFFFFFull) return usage(); o.tol_permille = (uint32_t)v; }
        else if (a == "--min-count" && k + 1 < argc) { if (!number(argv[++k], v)) return usage(); o.min_count = v; }
        else if (a == "-" || a[0] != '-') { if (in) return usage(); in = argv[k]; }
        else return usage();
    }
    if (!table || !in) return usage();
    std::string ttxt;
    if (!slurp(table, ttxt)) { fprintf(stderr, "Error: cannot read %s\n", table); return 10; }
    Stat S;
    S.f = strcmp(in, "-") ? fopen(in, "rb") : stdin;
    if (!S.f) { fprintf(stderr, "Error: cannot read %s\n", in); return 10; }
    const char* e = getenv("MKT_DEVICE");
    const int dev = e ? atoi(e) : 0;
    int rc = mkt_pairstat_create(dev, ttxt.data(), ttxt.size(), &S.p);
    if (rc == MKT_E_NO_DEVICE) { fprintf(stderr, "Error: GPU statistics: %s\n", mkt_strerror(rc)); return 20; }
    if (rc) return lib_fail(S, rc, "GPU statistics");
    std::vector<char> buf((size_t)64 << 20);
    bool first = true, gz = false;
    for (;; first = false) {
        const size_t k = fread(buf.data(), 1, buf.size(), S.f);
        if (k == 0) break;
        if (first && k >= 4 && (unsigned char)buf[0] == 0x1f && (unsigned char)buf[1] == 0x8b) {
            gz = true;
            if ((rc = mkt_bgzf_create(dev, &S.z))) { fprintf(stderr, "Error: GPU inflate: %s\n", mkt_strerror(rc)); return rc == MKT_E_NO_DEVICE ? 20 : 21; }
        }
        if (gz) {
            if ((rc = mkt_bgzf_add(S.z, buf.data(), k))) { fprintf(stderr, "Error: GPU inflate: %s: %s\n", mkt_strerror(rc), mkt_bgzf_error(S.z)); return 21; }
        } else if ((rc = mkt_pairstat_add(S.p, buf.data(), k))) return lib_fail(S, rc, "GPU statistics");
    }
    if (ferror(S.f)) { fprintf(stderr, "Error: cannot read %s\n", in); return 10; }
    if (gz) {
        const void* d = nullptr;
        uint64_t n = 0;
        if ((rc = mkt_bgzf_run(S.z, nullptr, nullptr)) || (rc = mkt_bgzf_device_text(S.z, &d, &n))) {
            fprintf(stderr, "Error: GPU inflate: %s: %s\n", mkt_strerror(rc), mkt_bgzf_error(S.z));
            return rc == MKT_E_FORMAT ? 12 : 21;
        }
        if (n && (rc = mkt_pairstat_add_device(S.p, d, (size_t)n))) return lib_fail(S, rc, "GPU statistics");
    }
    mkt_pairstat_info info;
    if ((rc = mkt_pairstat_run(S.p, &o, &info))) return lib_fail(S, rc, "GPU statistics");
    if (!prefix) return write_text(S, 0, "");
    if (int x = write_text(S, 0, std::string(prefix) + ".pairs.stat")) return x;
    return write_text(S, 1, std::string(prefix) + ".scaling.tsv");
}
