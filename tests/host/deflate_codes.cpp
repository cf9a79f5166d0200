// tests/host/deflate_codes.cpp -- TEST TOOL, never shipped or loaded by the product.
//
// Runs the code construction of the BGZF deflate kernel (microcket_amd/csrc/mkt_deflate_codes.h: the very functions
// k_bgzf_deflate calls) on the CPU, so that tests/test_deflate_codes_host.py can check it against a heap-based Huffman and
// the tables of RFC 1951 without a GPU.
//
//   deflate_codes tables        prints "L len sym eb ev" for len 3..258 and "D dist sym eb ev" for dist 1..32768
//   deflate_codes codes         reads histograms from stdin, one per line: "maxbits nsym c[0] ... c[nsym-1]"; for each prints
//                               one line of nsym table entries "length:code" (the code as stored: bit-reversed)
// The used symbols are handed over the way the kernel does it: ascending by count, ties by symbol.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../microcket_amd/csrc/mkt_deflate_codes.h"

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "tables")) {
        uint32_t sy, eb, ev;
        for (uint32_t l = 3; l <= 258; ++l) { mkt::len_code(l, sy, eb, ev); printf("L %u %u %u %u\n", l, sy, eb, ev); }
        for (uint32_t d = 1; d <= 32768; ++d) { mkt::dist_code(d, sy, eb, ev); printf("D %u %u %u %u\n", d, sy, eb, ev); }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "codes")) {
        int maxbits, nsym;
        while (scanf("%d %d", &maxbits, &nsym) == 2) {
            if (maxbits < 1 || maxbits > 15 || nsym < 1 || nsym > 288) { fprintf(stderr, "bad histogram head\n"); return 2; }
            std::vector<uint32_t> cnt(nsym);
            for (int s = 0; s < nsym; ++s) if (scanf("%u", &cnt[s]) != 1) { fprintf(stderr, "short histogram\n"); return 2; }
            std::vector<int> used;
            for (int s = 0; s < nsym; ++s) if (cnt[s]) used.push_back(s);
            std::stable_sort(used.begin(), used.end(), [&](int a, int b) { return cnt[a] < cnt[b]; });
            std::vector<uint32_t> skey(used.size() + 1), table(nsym);
            std::vector<uint16_t> ssym(used.size() + 1);
            for (size_t i = 0; i < used.size(); ++i) { skey[i] = cnt[used[i]]; ssym[i] = (uint16_t)used[i]; }
            mkt::huff_codes(skey.data(), ssym.data(), (int)used.size(), maxbits, table.data(), nsym);
            for (int s = 0; s < nsym; ++s) printf("%u:%u%c", table[s] >> 16, table[s] & 0xFFFFu, s + 1 < nsym ? ' ' : '\n');
        }
        return 0;
    }
    fprintf(stderr, "usage: deflate_codes tables | codes < histograms\n");
    return 2;
}
