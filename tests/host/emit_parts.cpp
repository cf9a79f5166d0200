// tests/host/emit_parts.cpp -- TEST TOOL, never shipped or loaded by the product.
//
// fast_emit_part (microcket_amd/csrc/mkt_fast.h) on the CPU: a FastState filled by hand with emitting groups, every .pairs line
// written piece by piece into a buffer between sentinel bytes, and the buffer compared byte by byte with fast_pair_byte, the
// per-byte definition of the same output.  For parts in {1, 2, 3, 4, 8}; pieces and lines once last to first and once first to
// last, so that a piece which writes a dword it shares with a neighbour (the piece beside it, or the line beside its line)
// destroys bytes that are already there, whichever side the neighbour is on.
//
// The tiles cover, and the program checks that they did: every destination alignment with every line length mod 4; the 14-byte
// line (fewer dwords than pieces); each of the four run boundaries e0 .. e3 exactly on an interior piece boundary and one byte to
// either side of it, for every parts > 1; 10-digit positions; a QNAME of 62 bytes (the longest the parser admits) and one of 123
// (with two 1-byte names all the 128-byte head row holds).
// Exit status 0 and a line "emit_parts ok ..." when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../microcket_amd/csrc/mkt_host.h"
#include "../../microcket_amd/csrc/mkt_fast.h"

using namespace mkt;

typedef FastCfg<kLeanTile, kLeanHB, kLeanHF, kLeanLCAP> FC;
static const uint32_t kParts[5] = {1, 2, 3, 4, 8};

struct Line { std::string q, ca, pa, cb, pb; char sa, sb; };

static std::string digits(uint32_t n, uint32_t salt) {             // n decimal digits, no leading zero
    std::string s;
    for (uint32_t k = 0; k < n; ++k) s.push_back((char)('0' + (k == 0 ? 1 + (salt + k) % 9 : (salt * 7 + k * 3) % 10)));
    return s;
}
static std::string name(uint32_t n, uint32_t salt, char first) {   // n bytes, none of them <= 0x20
    std::string s;
    for (uint32_t k = 0; k < n; ++k) s.push_back(k == 0 ? first : (char)('a' + (salt + 5 * k) % 26));
    return s;
}
static Line make(uint32_t ql, uint32_t cal, uint32_t pal, uint32_t cbl, uint32_t pbl, uint32_t salt) {
    Line l;
    l.q = name(ql, salt, 'Q'); l.ca = name(cal, salt + 1, 'c'); l.pa = digits(pal, salt); l.cb = name(cbl, salt + 2, 'C'); l.pb = digits(pbl, salt + 3);
    l.sa = salt & 1 ? '-' : '+'; l.sb = salt & 2 ? '-' : '+';
    return l;
}

struct Coverage {
    bool align[4][4] = {};                  // [dst & 3][plen & 3]
    bool shortest[5] = {};                  // per parts: a 14-byte line (nd < parts for parts = 8; the fewest dwords for the others)
    bool edge[5][4][3] = {};                // [parts][run boundary e0 .. e3][boundary - piece boundary + 1]
    bool pos10 = false, q62 = false, q123 = false;
    uint64_t lines = 0, bytes = 0;
};

static int failures = 0;
static void fail(const char* what, uint32_t parts, uint32_t a0, uint32_t at, int order) {
    if (failures++ < 20) fprintf(stderr, "emit_parts: %s (parts %u, base alignment %u, byte %u, order %d)\n", what, parts, a0, at, order);
}

// one tile: the lines one behind the other, as the kernel's offsets x_pair lay them out; the tile's output starts at alignment a0
static void run_tile(FastState<FC>& st, const std::vector<Line>& lines, uint32_t a0, Coverage& cov) {
    if (lines.size() > (size_t)FC::GCAP || 2 * lines.size() + 1 > (size_t)FC::LCAP) { fprintf(stderr, "emit_parts: tile too large\n"); exit(2); }
    memset(&st, 0, sizeof st);
    auto& g = st.u.g;
    uint32_t total = 0;
    for (size_t e = 0; e < lines.size(); ++e) {
        const Line& l = lines[e];
        const uint32_t i = 2u * (uint32_t)e + 1u, slot = (uint32_t)e;          // (line index, slot and ordinal all differ)
        // the three text runs in head row i, each with the tab behind it, at an offset that changes from line to line
        uint32_t w = i * (uint32_t)FC::HSTRIDE + (l.q.size() + l.ca.size() + l.cb.size() + 3u + (e % 5u) <= (uint32_t)FC::HEADB ? (uint32_t)(e % 5u) : 0u);
        if (l.q.size() + l.ca.size() + l.cb.size() + 3u > (size_t)FC::HEADB) { fprintf(stderr, "emit_parts: line longer than a head row\n"); exit(2); }
        auto put = [&](const std::string& s) { const uint32_t at = w; memcpy(st.win + w, s.data(), s.size()); st.win[w + s.size()] = '\t'; w += (uint32_t)s.size() + 1u; return at; };
        g.l_qa[slot] = (uint16_t)put(l.q); g.l_ca[slot] = (uint16_t)put(l.ca); g.l_cb[slot] = (uint16_t)put(l.cb);
        const std::string la = l.pa + "\t", lb = l.pb + "\t" + l.sa + "\t" + l.sb + "\n";
        if (la.size() > 16 || lb.size() > 16) { fprintf(stderr, "emit_parts: literal too long\n"); exit(2); }
        memset(&g.l_litA[slot][0], 0xA5, 16); memset(&g.l_litB[slot][0], 0x5A, 16);      // (what lies behind a literal is no zero)
        memcpy(&g.l_litA[slot][0], la.data(), la.size()); memcpy(&g.l_litB[slot][0], lb.data(), lb.size());
        const uint32_t e0 = (uint32_t)l.q.size() + 1u, e1 = e0 + (uint32_t)l.ca.size() + 1u, e2 = e1 + (uint32_t)la.size(), e3 = e2 + (uint32_t)l.cb.size() + 1u;
        const uint32_t plen = e3 + (uint32_t)lb.size();
        g.l_e0[slot] = (uint16_t)e0; g.l_e1[slot] = (uint16_t)e1; g.l_e2[slot] = (uint16_t)e2; g.l_e3[slot] = (uint16_t)e3;
        g.g_slot[i] = (uint8_t)slot; g.g_plen[i] = (uint16_t)plen; g.x_pair[i] = (uint16_t)total; g.em_idx[e] = (uint8_t)i;
        // what this line covers
        const uint32_t a = (a0 + total) & 3u, nd = (a + plen + 3u) >> 2;
        const uint32_t ee[4] = {e0, e1, e2, e3};
        cov.align[a][plen & 3u] = true;
        cov.pos10 = cov.pos10 || (l.pa.size() == 10 && l.pb.size() == 10);
        cov.q62 = cov.q62 || l.q.size() == 62; cov.q123 = cov.q123 || l.q.size() == 123;
        for (int pi = 0; pi < 5; ++pi) {
            const uint32_t parts = kParts[pi], q = (nd + parts - 1u) / parts;
            if (plen == 14u) cov.shortest[pi] = true;
            for (uint32_t p = 1; p < parts && p * q < nd; ++p)
                for (int r = 0; r < 4; ++r) {
                    const int dlt = (int)ee[r] - (int)(4u * p * q - a);
                    if (dlt >= -1 && dlt <= 1) cov.edge[pi][r][dlt + 1] = true;
                }
        }
        total += plen;
        ++cov.lines; cov.bytes += plen;
    }
    st.sums.emitted = (uint32_t)lines.size(); st.sums.pair_bytes = total;
    // the destination: 64 sentinel bytes on either side of the tile's output
    std::vector<uint32_t> store((total + 160u) / 4u + 2u);
    uint8_t* const buf = reinterpret_cast<uint8_t*>(store.data());
    uint8_t* const o = buf + 64 + a0;
    const size_t nbuf = 64 + a0 + total + 64;
    for (int pi = 0; pi < 5; ++pi)
        for (int order = 0; order < 2; ++order) {
            const uint32_t parts = kParts[pi];
            memset(buf, 0xEE, nbuf);
            const uint32_t E = (uint32_t)lines.size();
            for (uint32_t k = 0; k < E; ++k) {
                const uint32_t e = order ? k : E - 1u - k, i = g.em_idx[e];
                for (uint32_t pk = 0; pk < parts; ++pk)
                    fast_emit_part(st, g.g_slot[i], g.g_plen[i], o + g.x_pair[i], order ? pk : parts - 1u - pk, parts);
            }
            for (uint32_t k = 0; k < total; ++k) if (o[k] != fast_pair_byte(st, k)) { fail("output byte differs from fast_pair_byte", parts, a0, k, order); break; }
            for (size_t k = 0; k < nbuf; ++k) if ((k < 64 + a0 || k >= 64 + a0 + total) && buf[k] != 0xEE) { fail("byte outside the tile's output written", parts, a0, (uint32_t)k, order); break; }
        }
    // fast_emit_line is all parts of a line by one caller
    memset(buf, 0xEE, nbuf);
    for (uint32_t e = (uint32_t)lines.size(); e-- > 0;) { const uint32_t i = g.em_idx[e]; fast_emit_line(st, g.g_slot[i], g.g_plen[i], o + g.x_pair[i]); }
    for (uint32_t k = 0; k < total; ++k) if (o[k] != fast_pair_byte(st, k)) { fail("fast_emit_line differs from fast_pair_byte", 1, a0, k, 0); break; }
    // and the text is what the fields say (fast_pair_byte itself is pinned by the oracle parity tests; here against the hand-made lines)
    std::string want;
    for (const Line& l : lines) want += l.q + "\t" + l.ca + "\t" + l.pa + "\t" + l.cb + "\t" + l.pb + "\t" + l.sa + "\t" + l.sb + "\n";
    if (want.size() != total || memcmp(want.data(), o, total) != 0) fail("output differs from the lines' text", 1, a0, 0, 0);
}

int main() {
    std::unique_ptr<FastState<FC>> stp(new FastState<FC>);
    Coverage cov;
    uint32_t salt = 1;
    for (uint32_t a0 = 0; a0 < 4; ++a0) {
        // the shortest line, alone and among its like (every alignment: 14 = 2 mod 4)
        run_tile(*stp, {make(1, 1, 1, 1, 1, salt++)}, a0, cov);
        run_tile(*stp, std::vector<Line>(9, make(1, 1, 1, 1, 1, salt++)), a0, cov);
        // every QNAME length 1 .. 70 with names of 1, 4 and 5 bytes and positions of 1 .. 10 digits: the run boundaries pass over
        // every piece boundary of every parts
        for (uint32_t cal = 1; cal <= 6; ++cal) {
            std::vector<Line> t;
            for (uint32_t ql = 1; ql <= 70; ++ql) t.push_back(make(ql, cal, 1 + (ql + cal) % 10, 1 + (ql * 3 + cal) % 6, 1 + (ql * 7 + cal) % 10, salt++));
            run_tile(*stp, t, a0, cov);
        }
        for (uint32_t pal = 1; pal <= 10; ++pal) {
            std::vector<Line> t;
            for (uint32_t ql = 1; ql <= 40; ++ql) t.push_back(make(ql, 1 + ql % 5, pal, 1 + (ql / 5) % 5, 1 + (pal + ql) % 10, salt++));
            run_tile(*stp, t, a0, cov);
        }
        // 10-digit positions, the longest QNAMEs
        run_tile(*stp, {make(12, 5, 10, 5, 10, salt++), make(62, 5, 10, 5, 10, salt++), make(123, 1, 10, 1, 10, salt++), make(123, 1, 1, 1, 1, salt++), make(1, 1, 1, 1, 1, salt++)}, a0, cov);
    }
    bool all = cov.pos10 && cov.q62 && cov.q123;
    for (int a = 0; a < 4; ++a) for (int m = 0; m < 4; ++m) if (!cov.align[a][m]) { fprintf(stderr, "emit_parts: no line at alignment %d with length %d mod 4\n", a, m); all = false; }
    for (int pi = 0; pi < 5; ++pi) {
        if (!cov.shortest[pi]) all = false;
        if (kParts[pi] > 1)
            for (int r = 0; r < 4; ++r) for (int d = 0; d < 3; ++d)
                if (!cov.edge[pi][r][d]) { fprintf(stderr, "emit_parts: parts %u: run boundary e%d never %+d from a piece boundary\n", kParts[pi], r, d - 1); all = false; }
    }
    if (!all) { fprintf(stderr, "emit_parts: the cases do not cover what they are there for\n"); return 3; }
    if (failures) { fprintf(stderr, "emit_parts: %d failures\n", failures); return 1; }
    printf("emit_parts ok lines %llu bytes %llu\n", (unsigned long long)cov.lines, (unsigned long long)cov.bytes);
    return 0;
}
