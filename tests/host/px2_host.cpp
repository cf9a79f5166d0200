// px2_host.cpp -- stand-alone driver of the host half of the pairs.gz index (microcket_amd/csrc/mkt_px2.h): the fixed part of the
// index's header and the check of the name table for a pair that reappears.  No GPU, no HIP header.
//
// stdin:  "<lines> <runs>\n", then per run "<0-based line of its first record> <name>\n" in file order.
// stdout: "reappears <1-based line>\n" if a name stands in the table twice; else "ok <names>\n" and one line of hex: the header, the
//         name table, and per name an empty bin table and an empty linear index.
#include <cstdio>
#include <string>
#include <vector>

#include "../../microcket_amd/csrc/mkt_px2.h"

int main() {
    unsigned long long n_lines = 0, n_runs = 0;
    if (scanf("%llu %llu", &n_lines, &n_runs) != 2) return 2;
    std::vector<unsigned long long> line(n_runs);
    std::string table;
    for (unsigned long long k = 0; k < n_runs; ++k) {
        char name[4096];
        if (scanf("%llu %4095s", &line[k], name) != 2) return 2;
        table += name;
        table.push_back('\0');
    }
    const int64_t re = mkt::px_first_reappearing(table.data(), table.size(), n_runs);
    if (re != mkt::kPxNoName) { printf("reappears %llu\n", line[(size_t)re] + 1); return 0; }
    std::string out = mkt::px_head((uint32_t)n_runs, n_lines, (uint32_t)table.size());
    if (out.size() != mkt::kPxHeadBytes) return 3;
    out += table;
    for (unsigned long long k = 0; k < n_runs; ++k) { mkt::px_put32(out, 0); mkt::px_put32(out, 0); }
    printf("ok %llu\n", n_runs);
    for (unsigned char c : out) printf("%02x", c);
    printf("\n");
    // the window of a position at the edges the kernel shares with this half
    if (mkt::px_window(0) != 0 || mkt::px_window(1) != 0 || mkt::px_window(32768) != 0 || mkt::px_window(32769) != 1 || mkt::px_window(mkt::kPxPosMax) != 65535) return 4;
    return 0;
}
