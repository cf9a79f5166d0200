// tests/host/parse_chain.cpp -- TEST TOOL, never shipped or loaded by the product.
//
// What the lean kernel's heads phase leaves for its parser, and the parser's QNAME compare (microcket_amd/csrc/mkt_fast.h), on
// the CPU:
//   (a) fast_head_line through fast_head_chunk_ref: the line start (off16, goff) and the "second newline in the row's first
//       vector" verdict (bits) against a byte loop, for the newline in front of the line at every byte of its vector, alone
//       and with a second newline at every other byte, and for the line that opens the block;
//   (b) lean_eq against memcmp: every length 1 .. 101, both offsets at every byte of a dword, no difference and one differing
//       byte at every position of the range.  The twelve bytes behind either range always differ between the two sides, and
//       must not matter.  One side ends 11 bytes before the end of its allocation: the sanitized build of this program fails
//       on a read past the 11 bytes the compare is allowed.  Both sides take that place in turn;
//   (c) the separator words fast_head_ws hands the parser against the row's 128 mask bits shifted down by the line start,
//       for every start 0 .. 16 and random rows.
// Exit status 0 and a line "parse_chain ok ..." when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "../../microcket_amd/csrc/mkt_host.h"
#include "../../microcket_amd/csrc/mkt_fast.h"

using namespace mkt;

typedef FastCfg<kLeanTile, kLeanHB, kLeanHF, kLeanLCAP> FC;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "parse_chain: " __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// ---- (a) -------------------------------------------------------------------------------------------------
// A block of text whose vector V holds a newline at byte p (and one at q when q < 16); table entry `line` points at it.
static uint64_t row_start_cases(FastState<FC>& st) {
    uint64_t cases = 0;
    const uint32_t V = 3, n = 16u * 16u;
    std::vector<uint8_t> text(n);
    for (uint32_t first = 0; first < 2; ++first)                    // 1: the entry is the line that opens the block
        for (uint32_t line = first ? 0u : 1u; line < (first ? 1u : 3u); ++line)
            for (uint32_t p = 0; p < 16; ++p)
                for (uint32_t q = 0; q <= 16; ++q) {                // q == 16: no second newline
                    if (q == p) continue;
                    for (uint32_t k = 0; k < n; ++k) text[k] = (uint8_t)('A' + (k * 7u + p) % 26u);
                    const uint32_t v = first ? 0u : V + line;
                    text[16u * v + p] = '\n';
                    if (q < 16) text[16u * v + q] = '\n';
                    text[16u * (v + 1u) + 5u] = '\n';                 // the line ends: a complete line of one token is no record and no reason to defer
                    TileGeom G;
                    G.w0 = first ? 0u : 32u; G.t0 = G.w0; G.t1 = n; G.w1 = n;       // window-relative vector v - w0 / 16
                    memset(&st.u, 0, sizeof st.u);
                    memset(st.win, 0, sizeof st.win);
                    const uint32_t hv = v - G.w0 / 16u;
                    st.hv16[line] = (uint16_t)hv;
                    st.bits[line] = 0xFF; st.off16[line] = 0xFFFF; st.goff[line] = 0xFFFF;
                    for (uint32_t c = 0; c < (uint32_t)FC::HCH; ++c) fast_head_chunk_ref(st, text.data(), n, G, line, c);
                    // the reference: a byte loop over the vector
                    uint32_t soff = 0, count = 0;
                    if (!first) for (uint32_t b = 16; b-- > 0;) if (text[16u * v + b] == '\n') { soff = b + 1u; ++count; }
                    const bool multi = count > 1u;
                    CHECK(st.goff[line] == 16u * hv + soff, "goff: line %u p %u q %u first %u: %u, expected %u", line, p, q, first, st.goff[line], 16u * hv + soff);
                    CHECK(st.off16[line] == line * (uint32_t)FC::HSTRIDE + soff, "off16: line %u p %u q %u first %u: %u, expected %u", line, p, q, first, st.off16[line], line * (uint32_t)FC::HSTRIDE + soff);
                    CHECK((st.bits[line] != 0) == multi, "short-line verdict: line %u p %u q %u first %u: bits %u, expected %d", line, p, q, first, st.bits[line], (int)multi);
                    // ... and the parser reports it, and nothing else
                    {
                        st.NL = line + 1u; st.abn = 0;
                        if (line) { st.off16[line - 1u] = (uint16_t)((line - 1u) * (uint32_t)FC::HSTRIDE + 1u); }
                        Params P = {MODE_UNC, 0.5f, 10, 0};
                        const TextView tv = fast_view(st, text.data(), n, G);
                        fast_parse(st, tv, P, G, line);
                        CHECK(st.abn == (multi ? (uint32_t)AB_SHORT_LINE : 0u), "parser: line %u p %u q %u first %u: abn %u", line, p, q, first, st.abn);
                    }
                    ++cases;
                }
    return cases;
}

// ---- (b) -------------------------------------------------------------------------------------------------
static uint64_t lean_eq_cases() {
    uint64_t cases = 0;
    for (uint32_t len = 1; len <= 101; ++len)
        for (uint32_t sa = 0; sa < 4; ++sa)
            for (uint32_t sb = 0; sb < 4; ++sb)
                for (uint32_t order = 0; order < 2; ++order) {
                    // [front: 16 + s0 bytes][range 0: len][12 bytes][pad to a dword + s1][range 1: len][11 bytes] end of the allocation
                    const uint32_t s0 = order ? sb : sa, s1 = order ? sa : sb;
                    const uint32_t o0 = 16u + s0;
                    const uint32_t o1 = ((o0 + len + 12u + 3u) & ~3u) + 4u + s1;
                    const size_t size = (size_t)o1 + len + 11u;
                    uint8_t* win = (uint8_t*)malloc(size);
                    if (!win) { fprintf(stderr, "parse_chain: out of memory\n"); exit(2); }
                    for (size_t k = 0; k < size; ++k) win[k] = (uint8_t)(rnd() >> 32);
                    for (uint32_t k = 0; k < len; ++k) win[o1 + k] = win[o0 + k];
                    for (uint32_t k = 0; k < 11u; ++k) win[o1 + len + k] = (uint8_t)~win[o0 + len + k];      // behind the ranges: every byte differs
                    TextView tv;
                    tv.g = nullptr; tv.n = 0; tv.win = win; tv.w0 = 0; tv.wlen = (uint32_t)size; tv.nlm = nullptr; tv.wsm = nullptr;
                    const uint32_t a = order ? o1 : o0, b = order ? o0 : o1;     // (a & 3, b & 3) = (sa, sb)
                    CHECK((a & 3u) == sa && (b & 3u) == sb, "layout");
                    CHECK(lean_eq(tv, a, b, len), "equal ranges reported different: len %u sa %u sb %u order %u", len, sa, sb, order);
                    ++cases;
                    for (uint32_t d = 0; d < len; ++d)
                        for (uint32_t side = 0; side < 2; ++side) {
                            uint8_t& x = win[(side ? o1 : o0) + d];
                            const uint8_t keep = x;
                            x ^= (uint8_t)(1u << ((d + len + side) & 7u));
                            const bool want = memcmp(win + a, win + b, len) == 0;                             // false
                            CHECK(lean_eq(tv, a, b, len) == want, "differing byte %u of %u missed: sa %u sb %u order %u side %u", d, len, sa, sb, order, side);
                            x = keep;
                            ++cases;
                        }
                    free(win);
                }
    return cases;
}

// ---- (c) -------------------------------------------------------------------------------------------------
static uint64_t head_ws_cases(FastState<FC>& st) {
    uint64_t cases = 0;
    const uint32_t n = 16u * 16u;
    std::vector<uint8_t> text(n, (uint8_t)'x');
    for (uint32_t sh = 0; sh <= 16; ++sh)
        for (uint32_t round = 0; round < 64; ++round) {
            const uint32_t line = sh ? 1u + (round & 1u) : 0u;
            TileGeom G;
            G.w0 = sh ? 16u : 0u; G.t0 = G.w0; G.t1 = n; G.w1 = n;
            memset(st.win, 'x', sizeof st.win);
            if (sh) st.win[line * (uint32_t)FC::HSTRIDE + sh - 1u] = '\n';
            st.hv16[line] = (uint16_t)(2u + line);
            uint64_t A = rnd(), B = rnd();
            if (round == 0) { A = ~0ull; B = ~0ull; }
            if (round == 1) { A = 0; B = 1ull << 63; }
            memcpy(&st.u.m.hmask[line][0], &A, 8); memcpy(&st.u.m.hmask[line][4], &B, 8);
            fast_head_line(st, G, line);
            uint64_t ws0, ws1;
            fast_head_ws(st, line, ws0, ws1);
            // the 128 bits B:A shifted down by sh, bit by bit
            uint64_t e0 = 0, e1 = 0;
            for (uint32_t k = 0; k + sh < 128u; ++k) {
                const uint32_t s = k + sh;
                const uint64_t bit = s < 64u ? (A >> s) & 1ull : (B >> (s - 64u)) & 1ull;
                if (k < 64u) e0 |= bit << k; else e1 |= bit << (k - 64u);
            }
            CHECK(ws0 == e0 && ws1 == e1, "separator words: shift %u round %u: %016llx %016llx, expected %016llx %016llx", sh, round,
                  (unsigned long long)ws0, (unsigned long long)ws1, (unsigned long long)e0, (unsigned long long)e1);
            CHECK(st.off16[line] == line * (uint32_t)FC::HSTRIDE + sh, "separator words: shift %u: line start %u", sh, st.off16[line]);
            ++cases;
        }
    return cases;
}

int main() {
    std::unique_ptr<FastState<FC>> stp(new FastState<FC>);
    memset(stp.get(), 0, sizeof(FastState<FC>));
    const uint64_t na = row_start_cases(*stp);
    const uint64_t nb = lean_eq_cases();
    const uint64_t nc = head_ws_cases(*stp);
    if (fails) { fprintf(stderr, "parse_chain: %d checks failed\n", fails); return 1; }
    printf("parse_chain ok row starts %llu compares %llu separator words %llu\n", (unsigned long long)na, (unsigned long long)nb, (unsigned long long)nc);
    return 0;
}
