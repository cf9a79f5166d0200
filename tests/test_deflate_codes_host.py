"""The code construction of the BGZF deflate kernel (microcket_amd/csrc/mkt_deflate_codes.h: len_code, dist_code, mk_lengths,
huff_codes with its Kraft-sum length limiter, bitrev), run on the CPU through tests/host/deflate_codes.cpp and checked against a
heap-based Huffman written here and the tables of RFC 1951 3.2.5 written out below.  No GPU: the functions are the very ones
k_bgzf_deflate calls, compiled for the host.

The limiter only works when an unrestricted Huffman code is deeper than 15 bits (7 for the code-length code); the histograms
below contain such cases, and that precondition is asserted from the Python heap, never from the code under test."""
import random
import subprocess

import pytest

import util
from inflatedef import heap_huffman

# (alphabet size of the table, most symbols the kernel can use in it, maxbits)
ALPHABETS = {"litlen": (288, 286, 15), "dist": (32, 30, 15), "codelen": (19, 19, 7)}


_cache = {}


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def spread(values, nsym, nmax, rng):
    """the counts put on a seeded choice of the first nmax symbols of an alphabet of nsym, in a seeded order"""
    h = [0] * nsym
    for s, v in zip(rng.sample(range(nmax), len(values)), values):
        h[s] = v
    return h


def histograms():
    """[(name, alphabet, counts)], made once"""
    if "h" not in _cache:
        _cache["h"] = _histograms()
    return _cache["h"]


def _histograms():
    rng = random.Random(1951)
    out = []
    for alpha, (nsym, nmax, maxbits) in ALPHABETS.items():
        sizes = sorted(set([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 19, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 285, 286, nmax - 1, nmax]))
        sizes = [k for k in sizes if 1 <= k <= nmax]
        for k in sizes:
            out.append((f"{alpha}-equal-{k}", alpha, spread([3] * k, nsym, nmax, rng)))
            out.append((f"{alpha}-one-huge-{k}", alpha, spread([60000] + [1] * (k - 1), nsym, nmax, rng)))
            if k <= 31:
                out.append((f"{alpha}-pow2-{k}", alpha, spread([1 << i for i in range(k)], nsym, nmax, rng)))
        for k in range(1, min(nmax, 44) + 1):                                 # 44 exact Fibonacci counts still sum below 2^32
            t = fib(k)
            out.append((f"{alpha}-fib-{k}", alpha, spread(t, nsym, nmax, rng)))
            out.append((f"{alpha}-fib-ordered-{k}", alpha, t + [0] * (nsym - k)))
            out.append((f"{alpha}-fib-reversed-{k}", alpha, t[::-1] + [0] * (nsym - k)))
            ties = [v for v in t for _ in (0, 1)][:k]                         # 1 1 1 1 2 2 3 3 5 5 ...
            out.append((f"{alpha}-fib-ties-{k}", alpha, spread(ties, nsym, nmax, rng)))
            out.append((f"{alpha}-fib-plus-ones-{k}", alpha, spread((t + [1] * nmax)[:min(nmax, 2 * k)], nsym, nmax, rng)))
        for i in range(1500):
            k = rng.randrange(1, nmax + 1)
            kind = i % 5
            if kind == 0:
                v = [rng.randrange(1, 65000) for _ in range(k)]
            elif kind == 1:
                v = [rng.randrange(1, 4) for _ in range(k)]
            elif kind == 2:                                                   # geometric: deep codes
                r = rng.choice([1.3, 1.5, 1.62, 1.7, 2.0, 2.5])
                v = [max(1, int(r ** min(j, 40)) + rng.randrange(0, 2)) for j in range(k)]
            elif kind == 3:                                                   # Fibonacci with noise
                v = [max(1, x + rng.randrange(-1, 2)) for x in (fib(44) * 7)[:k]]
            else:                                                             # a few big, many small
                v = [rng.randrange(1, 3) for _ in range(k)]
                for j in rng.sample(range(k), min(k, rng.randrange(1, 6))):
                    v[j] = rng.randrange(1000, 65000)
            v = [min(x, (1 << 32) // (k + 1)) for x in v]                     # the code under test adds counts in 32 bits
            out.append((f"{alpha}-random-{i}", alpha, spread(v, nsym, nmax, rng)))
    return out


def tables():
    """the driver's answer for every histogram, computed once: [(name, alphabet, counts, lengths, stored codes)]"""
    if "t" not in _cache:
        util.ensure_built()
        hs = histograms()
        text = "".join(f"{ALPHABETS[a][2]} {len(c)} " + " ".join(map(str, c)) + "\n" for _, a, c in hs)
        r = subprocess.run([util.DEFLATE_CODES_EXE, "codes"], input=text.encode(), stdout=subprocess.PIPE, check=True)
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(hs)
        res = []
        for (name, a, c), ln in zip(hs, lines):
            ent = [tuple(map(int, e.split(":"))) for e in ln.split()]
            assert len(ent) == len(c)
            res.append((name, a, c, [e[0] for e in ent], [e[1] for e in ent]))
        _cache["t"] = res
    return _cache["t"]


def unreverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


def test_histogram_set_reaches_the_limiter():
    """the precondition, from the heap alone: unrestricted depths of 16 or more (15-bit codes) and 8 or more (7-bit code)"""
    deep = {a: 0 for a in ALPHABETS}
    exact = {a: False for a in ALPHABETS}
    for name, a, c in histograms():
        d = max(heap_huffman(c).values())
        if d > ALPHABETS[a][2]:
            deep[a] += 1
        if "-fib-ordered-" in name:
            k = sum(1 for x in c if x)
            assert d == max(k - 1, 1), name                      # exact Fibonacci counts: depth n - 1
            if d > ALPHABETS[a][2]:
                exact[a] = True
    assert all(v >= 50 for v in deep.values()), deep
    assert all(exact.values()), exact
    for a, k in (("litlen", 18), ("dist", 18), ("codelen", 10)):              # the smallest exact Fibonacci cases named in DESIGN.md
        c = fib(k)
        assert max(heap_huffman(c).values()) == k - 1 > ALPHABETS[a][2]
        assert any(n == f"{a}-fib-ordered-{k}" for n, _, _ in histograms())


def test_lengths_kraft_and_cost():
    n_limited = 0
    for name, a, c, lens, codes in tables():
        maxbits = ALPHABETS[a][2]
        used = [s for s, x in enumerate(c) if x]
        for s, x in enumerate(c):
            if x:
                assert 1 <= lens[s] <= maxbits, (name, s, lens[s])
            else:
                assert lens[s] == 0 and codes[s] == 0, (name, s)
        kraft = sum(1 << (maxbits - lens[s]) for s in used)
        if len(used) >= 2:
            assert kraft == 1 << maxbits, (name, kraft)                       # complete and not over-subscribed
        else:
            assert lens[used[0]] == 1, name
        shortest_rarer, prev = maxbits + 1, None                              # a more frequent symbol never has a longer code
        group = []
        for s in sorted(used, key=lambda s: c[s]) + [None]:
            if s is None or c[s] != prev:
                if group:
                    assert max(group) <= shortest_rarer, (name, prev)
                    shortest_rarer = min(shortest_rarer, min(group))
                group = []
                prev = None if s is None else c[s]
            if s is not None:
                group.append(lens[s])
        ref = heap_huffman(c)
        cost = sum(c[s] * lens[s] for s in used)
        ref_cost = sum(c[s] * ref[s] for s in used)
        if max(ref.values()) <= maxbits:
            assert cost == ref_cost, (name, cost, ref_cost)
        else:
            n_limited += 1
            assert cost >= ref_cost, (name, cost, ref_cost)
    assert n_limited >= 300


def test_codes_are_canonical_and_prefix_free():
    for name, a, c, lens, codes in tables():
        maxbits = ALPHABETS[a][2]
        # RFC 1951 3.2.2: the canonical code of these lengths
        bl_count = [0] * (maxbits + 2)
        for l in lens:
            if l:
                bl_count[l] += 1
        next_code, code = [0] * (maxbits + 2), 0
        for bits in range(1, maxbits + 1):
            code = (code + bl_count[bits - 1]) << 1
            next_code[bits] = code
        words = []
        for s, l in enumerate(lens):
            if l:
                assert codes[s] < 1 << l, (name, s)
                got = unreverse(codes[s], l)
                assert got == next_code[l], (name, s, got, next_code[l])
                next_code[l] += 1
                words.append(format(got, "0%db" % l))
        words.sort()
        for x, y in zip(words, words[1:]):
            assert not y.startswith(x), (name, x, y)


# RFC 1951 3.2.5, written out: (symbol, extra bits, first length) and (symbol, extra bits, first distance)
LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10), (265, 1, 11), (266, 1, 13),
                (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31), (273, 3, 35), (274, 3, 43), (275, 3, 51),
                (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115), (281, 5, 131), (282, 5, 163), (283, 5, 195), (284, 5, 227),
                (285, 0, 258)]
DIST_TABLE = [(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 0, 4), (4, 1, 5), (5, 1, 7), (6, 2, 9), (7, 2, 13), (8, 3, 17), (9, 3, 25), (10, 4, 33), (11, 4, 49),
              (12, 5, 65), (13, 5, 97), (14, 6, 129), (15, 6, 193), (16, 7, 257), (17, 7, 385), (18, 8, 513), (19, 8, 769), (20, 9, 1025),
              (21, 9, 1537), (22, 10, 2049), (23, 10, 3073), (24, 11, 4097), (25, 11, 6145), (26, 12, 8193), (27, 12, 12289), (28, 13, 16385),
              (29, 13, 24577)]


def rfc_symbol(table, v):
    """(symbol, extra bits, extra value) of a length or distance by the RFC's table: the last row whose base is <= v"""
    row = [r for r in table if r[2] <= v][-1]
    assert v - row[2] < 1 << row[1]
    return row[0], row[1], v - row[2]


def test_length_and_distance_symbols():
    util.ensure_built()
    out = subprocess.run([util.DEFLATE_CODES_EXE, "tables"], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    got = {"L": {}, "D": {}}
    for ln in out:
        k, v, sy, eb, ev = ln.split()
        got[k][int(v)] = (int(sy), int(eb), int(ev))
    assert sorted(got["L"]) == list(range(3, 259)) and sorted(got["D"]) == list(range(1, 32769))
    for l in range(3, 259):
        assert got["L"][l] == rfc_symbol(LENGTH_TABLE, l), l
    for d in range(1, 32769):
        assert got["D"][d] == rfc_symbol(DIST_TABLE, d), d


@pytest.mark.parametrize("v,n,want", [(0, 1, 0), (1, 1, 1), (1, 2, 2), (0b110, 3, 0b011), (0x30, 8, 0x0C), (1, 15, 1 << 14), (0x5555, 15, 0x5555), (0x1234, 16, 0x2C48)])
def test_unreverse_helper(v, n, want):
    assert unreverse(v, n) == want
