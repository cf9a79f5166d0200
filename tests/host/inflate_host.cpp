// inflate_host.cpp -- stand-alone driver of the shared half of the BGZF reader (microcket_amd/csrc/mkt_inflate.h): the block table and,
// member by member, the same header parse, table build and token decode the kernel runs, serially.  No GPU, no HIP header.
//
//   inflate_host <in.gz> <out.txt>
//
// stdout: "ok <blocks> <text bytes> <stored> <fixed> <dynamic> <has_eof>\n" and the text in out.txt, or "refused <reason key> <file
// offset of the block>\n" and no out.txt.  Exit status 0 either way; 2 for a file that cannot be read or written.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../microcket_amd/csrc/mkt_inflate.h"

static uint32_t crc32_of(const uint8_t* d, size_t n) {
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            tab[i] = c;
        }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = tab[(c ^ d[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> gz;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) gz.insert(gz.end(), buf, buf + got);
    fclose(f);
    std::vector<mkt::InfBlock> blocks;
    uint64_t bad = 0, kinds[3] = {0, 0, 0};
    bool has_eof = false;
    uint32_t r = mkt::inf_block_table(gz.data(), gz.size(), blocks, &bad, &has_eof);
    std::vector<uint8_t> text;
    for (size_t k = 0; !r && k < blocks.size(); ++k) {
        const mkt::InfBlock& b = blocks[k];
        const uint32_t nspan = b.bsize - mkt::kInfHead - mkt::kInfFoot;
        std::vector<uint8_t> span(nspan + mkt::kInfSpanPad, 0);             // an exact copy: a read past the pad is the sanitizer's to find
        if (nspan) memcpy(span.data(), gz.data() + b.coff + mkt::kInfHead, nspan);
        std::vector<uint8_t> out(b.isize);
        r = mkt::inf_member_serial(span.data(), nspan, out.data(), b.isize, kinds);
        if (!r && crc32_of(out.data(), out.size()) != b.crc) r = mkt::INF_CRC;
        if (r) bad = b.coff;
        text.insert(text.end(), out.begin(), out.end());
    }
    if (r) { printf("refused %s %llu\n", mkt::inf_reason_key(r), (unsigned long long)bad); return 0; }
    FILE* o = fopen(argv[2], "wb");
    if (!o || (text.size() && fwrite(text.data(), 1, text.size(), o) != text.size()) || fclose(o)) return 2;
    printf("ok %zu %zu %llu %llu %llu %d\n", blocks.size(), text.size(), (unsigned long long)kinds[0], (unsigned long long)kinds[1], (unsigned long long)kinds[2], has_eof ? 1 : 0);
    return 0;
}
