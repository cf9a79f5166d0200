// tests/host/trim_host.cpp -- TEST TOOL, never shipped or loaded by the product.
//
// Drives the host half of adapter and quality trimming (microcket_amd/csrc/mkt_trim.h: the argument check with the adapter table, the
// limit table, the record check, the tail rule) without a GPU, so that tests/test_ktrim_host.py can hold it against tests/ktrimdef.py;
// built plain and with the address and undefined-behaviour sanitizers.
//
//   trim_host limits M                   limit[0] .. limit[64] for mismatch M
//   trim_host check [key=value ...]      "ok <adapter 1> <adapter 2>" or "refused: <message>"
//   trim_host pairs [key=value ...]      per stdin line "h1 \t s1 \t p1 \t q1 \t h2 \t s2 \t p2 \t q2": "bad <code>" or "<kept> <class> <dimer>",
//                                        decided with mkt_trim.h's pieces in plain loops (quality window, seeds in ascending order, tail)
// keys: kit adapter1 adapter2 min_size phred min_qual window mismatch
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../microcket_amd/csrc/mkt_trim.h"

static std::vector<std::string> g_keep;      // the strings the options point to
static bool options(int argc, char** argv, int from, mkt_trim_opts* o) {
    o->adapter1 = o->adapter2 = o->kit = nullptr;
    o->min_size = 36; o->phred = 33; o->min_qual = 20; o->window = 5; o->mismatch = 0.125; o->interleaved_input = 0;
    g_keep.reserve((size_t)argc);
    for (int k = from; k < argc; ++k) {
        const char* eq = strchr(argv[k], '=');
        if (!eq) return false;
        const std::string key(argv[k], eq - argv[k]);
        g_keep.emplace_back(eq + 1);
        const char* v = g_keep.back().c_str();
        if (key == "kit") o->kit = v;
        else if (key == "adapter1") o->adapter1 = v;
        else if (key == "adapter2") o->adapter2 = v;
        else if (key == "min_size") o->min_size = (uint32_t)strtoul(v, nullptr, 10);
        else if (key == "phred") o->phred = (uint32_t)strtoul(v, nullptr, 10);
        else if (key == "min_qual") o->min_qual = (uint32_t)strtoul(v, nullptr, 10);
        else if (key == "window") o->window = (uint32_t)strtoul(v, nullptr, 10);
        else if (key == "mismatch") o->mismatch = strtod(v, nullptr);
        else return false;
    }
    return true;
}

static void decide(const mkt::TrParams& P, const std::vector<std::string>& f) {
    using namespace mkt;
    const uint8_t *s1 = (const uint8_t*)f[1].data(), *q1 = (const uint8_t*)f[3].data(), *s2 = (const uint8_t*)f[5].data(), *q2 = (const uint8_t*)f[7].data();
    uint32_t bad = trim_record_shape(f[0].empty() ? 0 : (uint8_t)f[0][0], (uint32_t)f[0].size(), f[2].empty() ? 0 : (uint8_t)f[2][0], (uint32_t)f[1].size(), (uint32_t)f[3].size());
    if (!bad) bad = trim_record_shape(f[4].empty() ? 0 : (uint8_t)f[4][0], (uint32_t)f[4].size(), f[6].empty() ? 0 : (uint8_t)f[6][0], (uint32_t)f[5].size(), (uint32_t)f[7].size());
    if (!bad) for (unsigned char c : f[3] + f[7]) if (!trim_qual_ok(c, P.phred)) bad = TR_BAD_QUAL;
    if (bad) { printf("bad %u\n", bad); return; }
    const uint32_t n = (uint32_t)(f[1].size() < f[5].size() ? f[1].size() : f[5].size());
    uint32_t k = 0, run = 0;
    for (uint32_t i = 0; i < n; ++i) {
        run = (q1[i] >= P.thr && q2[i] >= P.thr) ? run + 1 : 0;
        if (run >= P.window && i + 1 >= P.min_size) k = i + 1;
    }
    if (!k) { printf("0 %d 0\n", (int)TR_DROP_QUALITY); return; }
    for (uint32_t p = 0; p + TR_SEED <= k; ++p) {
        if (memcmp(s1 + p, P.a1, TR_SEED) != 0 && memcmp(s2 + p, P.a2, TR_SEED) != 0) continue;
        const uint32_t L = k - p < P.alen ? k - p : P.alen;
        uint32_t c1 = 0, c2 = 0;
        for (uint32_t j = 0; j < L; ++j) { c1 += s1[p + j] != P.a1[j]; c2 += s2[p + j] != P.a2[j]; }
        if (c1 <= P.limit[L] && c2 <= P.limit[L]) { printf("%u %d %d\n", p, (int)TR_ADAPTER, p <= TR_DIMER ? 1 : 0); return; }
    }
    const uint32_t k2 = trim_tail(s1, s2, k, P.a1, P.a2);
    printf("%u %d 0\n", k2, k2 != k ? (int)TR_TAILHIT : (int)TR_PASS);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s limits M | check [key=value ...] | pairs [key=value ...]\n", argv[0]); return 2; }
    const std::string cmd = argv[1];
    if (cmd == "limits" && argc == 3) {
        uint8_t lim[MKT_TRIM_MAX_ADAPTER + 1];
        mkt::trim_limits(strtod(argv[2], nullptr), lim);
        for (int L = 0; L <= MKT_TRIM_MAX_ADAPTER; ++L) printf("%u%c", (unsigned)lim[L], L < MKT_TRIM_MAX_ADAPTER ? ' ' : '\n');
        return 0;
    }
    mkt_trim_opts o;
    if ((cmd != "check" && cmd != "pairs") || !options(argc, argv, 2, &o)) { fprintf(stderr, "bad arguments\n"); return 2; }
    mkt::TrParams P;
    char msg[256];
    const int rc = mkt::trim_resolve(&o, &P, msg, sizeof msg);
    if (cmd == "check") {
        if (rc != MKT_OK) printf("refused: %s\n", msg);
        else printf("ok %.*s %.*s\n", (int)P.alen, (const char*)P.a1, (int)P.alen, (const char*)P.a2);
        return 0;
    }
    if (rc != MKT_OK) { fprintf(stderr, "refused: %s\n", msg); return 2; }
    std::string line;
    for (int c; (c = getchar()) != EOF;) {
        if (c != '\n') { line += (char)c; continue; }
        std::vector<std::string> f(1);
        for (char ch : line) { if (ch == '\t') f.emplace_back(); else f.back() += ch; }
        line.clear();
        if (f.size() != 8) { fprintf(stderr, "a line of %zu fields\n", f.size()); return 2; }
        decide(P, f);
    }
    return 0;
}
