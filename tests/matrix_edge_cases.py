"""Inputs for contact-matrix binning that sit on the steps of the kernels' own constants, each with what the definition
(tests/matrixdef.py) says about it.  No GPU and nothing of the package is needed here: test_matrix_edges_host.py runs every builder
on its own, test_gpu_matrix_edges.py feeds what they return to microcket_amd.Matrix.

A builder asserts, before it returns, what the definition alone says about its input: the exact skipped count, the number of
cells, and the property the case exists for.  A case therefore cannot pass because most of it was skipped, or because the step
it aims at moved.

The constants and rules of the code under test are restated below, in the manner of test_gpu_dedup_keys.py; each names the line
it restates by the name of the constant or function (all under microcket_amd/csrc)."""
import functools
from collections import namedtuple

import numpy as np

import matrixdef as md

MXWG = 256                    # MXWG in mkt_matrix.hip          threads per workgroup, and the sub-tile of the head passes
MX_TILE = 8 * MXWG            # MX_TILE in mkt_matrix.hip       sorted keys per workgroup in the two head passes (2048)
MX_CPW = 4 * MXWG             # MX_CPW in mkt_matrix.hip        cells per workgroup in the two text passes (1024)
DS_T = 8192                   # DS_T in mkt_kernels.hip         records per tile of a radix pass
DS_D = 7                      # DS_D in mkt_kernels.hip         bits per radix digit
K_CHR_SLOTS = 8192            # kChrSlots in mkt_core.h         names a table may hold
K_MX_SLOTS = 2 * K_CHR_SLOTS  # kMxSlots in mkt_matrix_obj.h    slots of the name table (16384)
NAME_MAX = 63                 # MxTab::name in mkt_matrix_obj.h bytes of a name ([63] holds the length)
assert (MX_TILE, MX_CPW, K_MX_SLOTS) == (2048, 1024, 16384)
M64 = (1 << 64) - 1

Case = namedtuple("Case", "table res text want pairs skipped nbins facts")   # want: {r: (cells, skipped)}; facts: what the builder found


# ---- the rules restated ---------------------------------------------------------------------------------------------------------
def key_bits(nbins):
    """MxRes::B as mkt_matrix_create sets it (mkt_matrix.hip): the bits of nbins itself, at most 32"""
    B = 0
    while B < 32 and (1 << B) <= nbins:
        B += 1
    return B


def radix_shifts(B):
    """the shifts of launch_radix64(.., 0, 2 * B, ..) (mkt_kernels.hip): one pass per started 7-bit digit"""
    return list(range(0, 2 * B, DS_D))


def cell_key(b1, b2, nbins):
    """k_mx_keys (mkt_matrix.hip): the key of a binned pair"""
    return (min(b1, b2) << key_bits(nbins)) | max(b1, b2)


def unbinned_key(nbins):
    """k_mx_keys (mkt_matrix.hip): what is not binned sorts behind every cell"""
    return (nbins << key_bits(nbins)) | nbins


def mx_fnv(name: bytes):
    """mx_fnv (mkt_matrix.hip): FNV-1a, 0 is kept for "empty" """
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) & M64
    return h or 1


def home_slot(name: bytes):
    """the first slot of a name: find in k_mx_parse and the fill loop of mkt_matrix_create (mkt_matrix.hip)"""
    return (mx_fnv(name) >> 17) & (K_MX_SLOTS - 1)


def build_slots(names):
    """the table as mkt_matrix_create fills it (hostTab in mkt_matrix.hip): names in table order, linear probing with wrap-around"""
    slots = [None] * K_MX_SLOTS
    for i, nm in enumerate(names):
        s = home_slot(nm)
        while slots[s] is not None:
            s = (s + 1) & (K_MX_SLOTS - 1)
        slots[s] = i
    return slots


def probe(slots, names, q: bytes):
    """(table index or -1, the slots looked at) for a name of the text, as find walks them (the lambda in k_mx_parse, mkt_matrix.hip)"""
    seen = []
    if not 1 <= len(q) <= NAME_MAX:
        return -1, seen
    s = home_slot(q)
    for _ in range(K_MX_SLOTS):
        seen.append(s)
        if slots[s] is None:
            return -1, seen
        if names[slots[s]] == q:
            return slots[s], seen
        s = (s + 1) & (K_MX_SLOTS - 1)
    return -1, seen


# ---- text and arrays side by side -------------------------------------------------------------------------------------------------
TAILS = {5: b"", 6: b"\t+", 7: b"\t+\t-", 12: b"\t+\t-\t60\t60\t150M\t150M\tNM:i:0"}
UNKNOWN = b"chrNotThere"


def table_text(table) -> bytes:
    return b"".join(b"%s\t%d\n" % (nm, L) for nm, L in table)


class Build:
    """lines of .pairs text next to the arrays the definition takes; ia / ib = -1 writes a name the table does not have"""

    def __init__(self, table):
        self.table = list(table)
        self.names = [nm for nm, _ in self.table]
        assert UNKNOWN not in self.names
        self.items = []

    def pair(self, ia, pa, ib, pb, cols=7):
        self.items.append((int(ia), int(pa), int(ib), int(pb), cols))

    def pairs(self, ia, pa, ib, pb, cols=7):
        self.items.extend((a, p, b, q, cols) for a, p, b, q in zip(np.asarray(ia).tolist(), np.asarray(pa).tolist(), np.asarray(ib).tolist(), np.asarray(pb).tolist()))

    def comment(self, text=b"#columns: readID chr1 pos1 chr2 pos2 strand1 strand2"):
        assert text.startswith(b"#") and b"\n" not in text
        self.items.append(text)

    def case(self, res, order=None, facts=None):
        items = self.items if order is None else [self.items[i] for i in order]
        names = self.names
        lines, rows = [], []
        for it in items:
            if isinstance(it, bytes):
                lines.append(it + b"\n")
                continue
            a, p, b, q, cols = it
            lines.append(b"r\t%s\t%d\t%s\t%d%s\n" % (names[a] if a >= 0 else UNKNOWN, p, names[b] if b >= 0 else UNKNOWN, q, TAILS[cols]))
            rows.append((a, p, b, q))
        arr = np.array(rows, dtype=np.int64).reshape(-1, 4)
        want = md.definition_arrays(self.table, res, arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])
        nbins = {r: md.bin_layout(self.table, r)[2] for r in res}
        return Case(table_text(self.table), list(res), b"".join(lines), want, len(rows), want[res[0]][1], nbins, facts or {})


def text_case(table, res, text, facts=None):
    """a case whose arrays come from the definition's own reading of the text (small inputs only)"""
    tt = table_text(table)
    want = md.definition(tt, res, text)
    return Case(tt, list(res), text, want, md.n_pairs(text), want[res[0]][1], {r: md.bin_layout(table, r)[2] for r in res}, facts or {})


def cell_set(cells):
    return {(int(a), int(b)) for a, b, _ in cells.tolist()}


def heads(cells):
    """where each run starts among the sorted binned keys: the exclusive prefix sums of the counts"""
    c = cells[:, 2].astype(np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]) if c.size else np.zeros(0, dtype=np.int64)


# ---- 1. key width ---------------------------------------------------------------------------------------------------------------
KEY_WIDTH_K = [1, 2, 3, 4, 7, 8, 10, 11, 14, 15, 16, 17, 21, 24, 25, 28, 31, 32]


def key_width_nbins(k):
    return [n for n in ((1 << k) - 1, 1 << k) if n < (1 << 32)]


@functools.lru_cache(maxsize=None)
def key_width_case(nbins):
    """one chromosome of nbins bases at r = 1: bin = position - 1, so any bin id costs nothing"""
    b = Build([(b"c", nbins)])
    rng = np.random.default_rng(nbins % 1000003)
    top = 1 << ((nbins - 1).bit_length() - 1) if nbins > 1 else 0
    last, prev = nbins - 1, max(nbins - 2, 0)
    required = [(0, 0), (0, last), (last, last), (prev, last)]
    xs = sorted({int(x) for x in rng.integers(0, max(top, 1), size=6)} | {0, max(top - 1, 0)})
    pool = {0, last, prev}
    twins = []                                                  # cells whose keys differ in exactly one bit
    for x in xs:
        for y in (x | top, x ^ 1):
            if y < nbins and y != x:
                pool |= {x, y}
                twins += [((x, last), (y, last)), ((0, x), (0, y))]
    for c in required:
        b.pair(0, c[0] + 1, 0, c[1] + 1)
    for c1, c2 in twins:
        for c in (c1, c2):
            b.pair(0, c[1] + 1, 0, c[0] + 1, cols=5)            # the larger bin first: the kernel orders them
    pl = np.array(sorted(pool), dtype=np.int64)
    n_rand = 3000
    b.pairs(np.zeros(n_rand, int), pl[rng.integers(0, pl.size, n_rand)] + 1, np.zeros(n_rand, int), pl[rng.integers(0, pl.size, n_rand)] + 1)
    b.pairs(np.zeros(500, int), rng.integers(0, nbins, 500) + 1, np.zeros(500, int), rng.integers(0, nbins, 500) + 1, cols=6)
    n_binned = len(b.items)
    for ia, pa, ib, pb in ((0, 0, 0, 1), (0, 1, 0, nbins + 1), (-1, 1, 0, 1), (0, nbins, -1, nbins), (0, nbins + 1, 0, nbins + 1), (0, 0, 0, 0), (-1, 1, -1, 1)):
        b.pair(ia, pa, ib, pb)
    b.comment(); b.comment(b"#")
    order = rng.permutation(len(b.items)).tolist()
    B = key_bits(nbins)
    case = b.case([1], order, facts={"B": B, "shifts": radix_shifts(B)})
    cells, skipped = case.want[1]
    # what the definition says, before any GPU is asked
    assert case.nbins[1] == nbins and skipped == 7 and case.pairs == n_binned + 7 and int(cells[:, 2].sum()) == n_binned
    have = cell_set(cells)
    assert set(required) <= have and len(have) == cells.shape[0] == len({(min(i[1], i[3]), max(i[1], i[3])) for i in b.items[:n_binned]})
    for c1, c2 in twins:
        k1, k2 = cell_key(*c1, nbins), cell_key(*c2, nbins)
        assert c1 in have and c2 in have and bin(k1 ^ k2).count("1") == 1
    if nbins >= 4:
        assert any((k1 ^ k2) == top << B for (c1, c2) in twins for k1, k2 in [(cell_key(*c1, nbins), cell_key(*c2, nbins))])   # the top bit of bin1
        assert any((k1 ^ k2) == 1 for (c1, c2) in twins for k1, k2 in [(cell_key(*c1, nbins), cell_key(*c2, nbins))])          # bit 0 of bin2
    # the key of what is not binned is behind the last cell, and every bit of both is inside the sorted 2B bits
    assert unbinned_key(nbins) > cell_key(last, last, nbins) and unbinned_key(nbins) < (1 << (2 * B)) <= (1 << 64)
    if nbins & (nbins + 1) == 0:                                # 2^k - 1: one bit of each half tells the two apart
        x = unbinned_key(nbins) ^ cell_key(last, last, nbins)
        assert bin(x >> B).count("1") == 1 and bin(x & ((1 << B) - 1)).count("1") == 1 and B == nbins.bit_length()
    else:
        assert nbins & (nbins - 1) == 0 and B == nbins.bit_length()
    assert len(radix_shifts(B)) == -(-2 * B // DS_D) and (B < 32 or radix_shifts(B)[-1] == 63)
    return case


# 16 resolutions over one record list; L_0 % r is 0, 1 and r - 1 among them
MANY_TABLE = [(b"first", 3_000_000), (b"second", 2_000_003)]
MANY_RES = [1, 2, 3, 7, 13, 100, 299, 1000, 4096, 65536, 1_000_000, 1_500_000, 2_999_999, 3_000_001, 2999, 4294967295]


@functools.lru_cache(maxsize=None)
def many_resolutions_case():
    b = Build(MANY_TABLE)
    rng = np.random.default_rng(16)
    L0, L1 = MANY_TABLE[0][1], MANY_TABLE[1][1]
    edge = [(0, 1), (0, L0), (0, L0 - 1), (1, 1), (1, 2), (1, L1), (1, L1 - 1)]
    for ca, pa in edge:
        for cb, pb in edge:
            b.pair(ca, pa, cb, pb)
    n = 4000
    ia, ib = rng.integers(0, 2, n), rng.integers(0, 2, n)
    Ls = np.array([L0, L1])
    b.pairs(ia, 1 + (rng.random(n) * Ls[ia]).astype(np.int64), ib, 1 + (rng.random(n) * Ls[ib]).astype(np.int64))
    n_binned = len(b.items)
    b.pair(0, L0 + 1, 1, 1); b.pair(1, L1 + 1, 0, 1); b.pair(-1, 5, 0, 5); b.comment()
    case = b.case(MANY_RES, rng.permutation(len(b.items)).tolist(), facts={"B": sorted({key_bits(md.bin_layout(MANY_TABLE, r)[2]) for r in MANY_RES})})
    assert len(MANY_RES) == 16 and len(set(MANY_RES)) == 16
    assert {"zero": any(L0 % r == 0 and r > 1 for r in MANY_RES), "one": any(L0 % r == 1 for r in MANY_RES), "r-1": any(L0 % r == r - 1 and r > 2 for r in MANY_RES)} == {"zero": True, "one": True, "r-1": True}
    assert len(case.facts["B"]) >= 8                                        # several key widths share the one record list
    for r in MANY_RES:
        cells, skipped = case.want[r]
        off1 = -(-L0 // r)                                                  # the first bin of the second chromosome
        assert skipped == 3 and int(cells[:, 2].sum()) == n_binned and md.bin_layout(MANY_TABLE, r)[0] == [0, off1]
        assert (off1 - 1, off1) in cell_set(cells)                          # first:L0 with second:1, on either side of the seam
    return case


# ---- 2. tiles -----------------------------------------------------------------------------------------------------------------------
TILE_NV = [1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16385]
TILE_EXTRA = [0, 1, 3000]
TILE_SHAPES = ["one", "distinct", "runs"]
TILE_TABLE = [(b"t", 1 << 20)]
TEXT_NNZ = [1023, 1024, 1025, 2048, 2049]


def run_lengths(nv):
    """sorted keys 0 .. nv: 2047 single keys; a run whose head is the last key of the first 2048-tile and whose other four keys open
    the second; 2044 keys to the end of that tile; one run over the third and fourth tile exactly; a single key that opens the
    fifth; then runs of 1, 2, 3, 1, 2, 3, ... keys.  Cut off at nv."""
    lens = [1] * (MX_TILE - 1) + [5, MX_TILE - 4, 2 * MX_TILE, 1]
    k, total = 0, sum(lens)
    while total < nv:
        lens.append(1 + k % 3)
        total += lens[-1]
        k += 1
    out, left = [], nv
    for x in lens:
        if left <= 0:
            break
        out.append(min(x, left))
        left -= out[-1]
    return out


def _extras(b, extra, sel, n_main, rng):
    """positions (in the final order) of `extra` lines that are not binned: skipped pairs and '#' lines, first, last and in between"""
    bad = [(0, 0, 0, 1), (0, 1, 0, (1 << 20) + 1), (-1, 1, 0, 1), (0, 7, -1, 7)]
    first, mid, last = [], [], []
    n_skip = 0
    for j in range(extra):
        where = (first, mid, last)[(j + sel // 2) % 3]
        if (j + sel) % 2:
            b.comment(b"#%d" % j)
        else:
            b.pair(*bad[(j // 2) % 4])
            n_skip += 1
        where.append(n_main + j)
    order = rng.permutation(n_main).tolist()
    for idx in mid:
        order.insert(int(rng.integers(1, max(len(order), 2))), idx)
    return first + order + last, n_skip


@functools.lru_cache(maxsize=None)
def tile_case(nv, extra, shape):
    b = Build(TILE_TABLE)
    sel = TILE_NV.index(nv) + TILE_SHAPES.index(shape)
    rng = np.random.default_rng(nv * 7 + extra + sel)
    if shape == "one":
        lens, cell = [nv], lambda s: (5, 9)
    elif shape == "distinct":
        lens, cell = [1] * nv, lambda s: (s, s + 1)
    else:
        lens, cell = run_lengths(nv), lambda s: (s, s + 1)
    b1 = np.repeat(np.array([cell(s)[0] for s in range(len(lens))], dtype=np.int64), lens)
    b2 = np.repeat(np.array([cell(s)[1] for s in range(len(lens))], dtype=np.int64), lens)
    swap = rng.random(nv) < 0.5                                             # the larger bin first in half of the lines
    b.pairs(np.zeros(nv, int), np.where(swap, b2, b1) + 1, np.zeros(nv, int), np.where(swap, b1, b2) + 1, cols=5 if nv % 2 else 7)
    order, n_skip = _extras(b, extra, sel, nv, rng)
    case = b.case([1, 64], order, facts={"n": nv + extra, "nv": nv})
    cells, skipped = case.want[1]
    assert len(b.items) == nv + extra and skipped == n_skip and case.pairs == nv + n_skip and int(cells[:, 2].sum()) == nv
    assert extra != 3000 or (n_skip == 1500 and case.text.startswith((b"#", b"r\t")) and case.text.count(b"\n#") + case.text.startswith(b"#") == 1500)
    assert cells.shape[0] == len(lens) and cells[:, 2].tolist() == lens     # nnz = 1, = nv, or the planned runs
    if shape == "runs":
        h = heads(cells).tolist()
        if nv >= MX_TILE + 4:
            assert MX_TILE - 1 in h and not set(range(MX_TILE, MX_TILE + 4)) & set(h)        # a head on the last key of a tile
        if nv >= 4 * MX_TILE + 1:
            assert 2 * MX_TILE in h and 4 * MX_TILE in h and not set(range(2 * MX_TILE + 1, 4 * MX_TILE)) & set(h)   # two whole tiles
            assert lens[h.index(4 * MX_TILE)] == 1                          # a single key opens a tile
    return case


@functools.lru_cache(maxsize=None)
def text_nnz_case(nnz):
    b = Build(TILE_TABLE)
    rng = np.random.default_rng(nnz)
    lens = [1 + s % 3 for s in range(nnz)]
    s = np.repeat(np.arange(nnz, dtype=np.int64), lens)
    b.pairs(np.zeros(s.size, int), s + 1, np.zeros(s.size, int), s + 8)
    b.pair(0, 0, 0, 1); b.pair(-1, 1, 0, 1); b.comment()
    case = b.case([1], rng.permutation(len(b.items)).tolist())
    cells, skipped = case.want[1]
    assert cells.shape[0] == nnz and skipped == 2 and cells[:, 2].tolist() == lens
    return case


# ---- 3. the name table ----------------------------------------------------------------------------------------------------------
NameCase = namedtuple("NameCase", "case names slots wrapped chain absent_occupied absent_in_chain")


@functools.lru_cache(maxsize=None)
def name_table_case():
    # (a) names whose home is one of the last two slots: the first two take them, the others wrap to slot 0 and on
    wrapped, i = [], 0
    while len(wrapped) < 6:
        nm = b"w%d" % i
        if home_slot(nm) >= K_MX_SLOTS - 2:
            wrapped.append(nm)
        i += 1
    # (b) exactly 8192 names, 1 .. 63 bytes, among them names that are prefixes and extensions of one another
    names = wrapped + [b"chr1", b"chr10", b"chr1_", b"chr1_random", b"chr", b"c", b"X", b"7", b"L" * NAME_MAX, b"L" * (NAME_MAX - 1)]
    k = 0
    while len(names) < K_CHR_SLOTS:
        stem = b"%d_" % k
        names.append(stem + b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ.-"[:max(1 + k % NAME_MAX - len(stem), 0)])
        k += 1
    assert len(names) == len(set(names)) == K_CHR_SLOTS and {len(n) for n in names} == set(range(1, NAME_MAX + 1))
    table = [(nm, 50 + i % 50) for i, nm in enumerate(names)]
    slots = build_slots(names)
    assert sum(s is not None for s in slots) == K_CHR_SLOTS
    # the searched properties, on the restatement: the homes, and a chain that crosses the end of the table
    assert all(home_slot(w) in (K_MX_SLOTS - 2, K_MX_SLOTS - 1) for w in wrapped)
    chain = list(range(min(home_slot(w) for w in wrapped), K_MX_SLOTS))
    while slots[(chain[-1] + 1) % K_MX_SLOTS] is not None:
        chain.append((chain[-1] + 1) % K_MX_SLOTS)
    assert all(slots[s] is not None for s in chain) and len(chain) >= 6
    over = [w for w in wrapped if slots.index(names.index(w)) < K_MX_SLOTS - 2]
    assert len(over) >= 4                                                   # these sit in slots 0, 1, ..: found only by wrapping
    for w in over:
        idx, seen = probe(slots, names, w)
        assert idx == names.index(w) and seen[0] >= K_MX_SLOTS - 2 and K_MX_SLOTS - 1 in seen and 0 in seen
    # two names of the table with one home slot
    homes = {}
    for nm in names:
        homes.setdefault(home_slot(nm), []).append(nm)
    shared = [v for v in homes.values() if len(v) > 1]
    assert shared
    # names the table does not have: (1) the home slot is taken, (2) the probe starts inside the chain that wraps, before and after the end
    have = set(names)
    absent_occupied, j = [], 0
    while len(absent_occupied) < 40:
        nm = b"abs%d" % j
        if nm not in have and slots[home_slot(nm)] is not None:
            absent_occupied.append(nm)
        j += 1
    absent_in_chain, j = [], 0
    want_before, want_after = 2, 2
    while want_before or want_after:
        nm = b"q%d" % j
        j += 1
        h = home_slot(nm)
        if nm in have or h not in chain:
            continue
        if h >= K_MX_SLOTS - 2 and want_before:
            want_before -= 1
            absent_in_chain.append(nm)
        elif h < K_MX_SLOTS - 2 and want_after:
            want_after -= 1
            absent_in_chain.append(nm)
    for nm in absent_occupied + absent_in_chain:
        idx, seen = probe(slots, names, nm)
        assert idx == -1 and len(seen) >= 2 and slots[seen[-1]] is None
    assert sum(1 for nm in absent_in_chain if probe(slots, names, nm)[1][0] >= K_MX_SLOTS - 2 and 0 in probe(slots, names, nm)[1]) == 2
    long63 = next(nm for nm in names if len(nm) == NAME_MAX and nm[:1] != b"L")
    cut = [nm[:-1] for nm in (names[100], names[2000], b"chr1_random", long63) if nm[:-1] not in have]
    assert len(cut) == 4
    # the pairs: every name on both sides; then what must be skipped, one line each, next to a name that is there
    lines = [b"r\t%s\t%d\t%s\t%d\t+\t-\n" % (names[i], 1 + i % 50, names[(i * 7 + 3) % K_CHR_SLOTS], 1 + (i * 3) % 50) for i in range(K_CHR_SLOTS)]
    assert {(i * 7 + 3) % K_CHR_SLOTS for i in range(K_CHR_SLOTS)} == set(range(K_CHR_SLOTS))
    for a in (b"chr1", b"chr10", b"chr1_", b"chr1_random", b"chr", b"c"):
        for c in (b"chr1", b"chr10", b"chr1_", b"chr"):
            lines.append(b"r\t%s\t50\t%s\t1\t+\t-\n" % (a, c))
    n_ok = len(lines)
    bad = absent_occupied + absent_in_chain + cut + [long63 + b"z", b"L" * 64, b"", b"chr1\x00", b"chr11", b"ch"]
    for k, nm in enumerate(bad):
        assert nm not in have
        lines.append(b"r\t%s\t1\tchr1\t1\t+\t-\n" % nm if k % 2 else b"r\tchr1\t1\t%s\t1\n" % nm)
    lines.append(b"r\t\t1\t\t1\n")
    rng = np.random.default_rng(3)
    text = b"".join(lines[i] for i in rng.permutation(len(lines)).tolist())
    case = text_case(table, [1, 37], text)
    cells, skipped = case.want[1]
    assert skipped == len(bad) + 1 and case.pairs == n_ok + skipped and int(cells[:, 2].sum()) == n_ok
    off = md.bin_layout(table, 1)[0]
    assert {names.index(b"chr1"), names.index(b"chr10"), names.index(b"chr1_"), names.index(b"chr")} == {6, 7, 8, 10}
    assert (off[6], off[7] + 49) in cell_set(cells) and (off[6], off[8] + 49) in cell_set(cells)    # chr10:50 / chr1_:50 with chr1:1
    return NameCase(case, names, slots, wrapped, chain, absent_occupied, absent_in_chain)


# ---- 4. positions and resolutions ---------------------------------------------------------------------------------------------------
U32 = (1 << 32) - 1
MOD64_ONE = (1 << 64) + 1                                       # 20 digits, 1 (mod 2^64): a 64-bit accumulator without a cap reads 1
MOD32_ONE = -(-10 ** 19 // (1 << 32)) * (1 << 32) + 1           # 20 digits, 1 (mod 2^32) and below 2^64: a 32-bit store of it reads 1
BIG25 = [b"1" + b"0" * 24, b"%d" % (100_000 * (1 << 64) + 1), b"9" * 25]
assert len(str(MOD64_ONE)) == 20 and MOD64_ONE % (1 << 64) == 1
assert len(str(MOD32_ONE)) == 20 and MOD32_ONE % (1 << 32) == 1 and MOD32_ONE < (1 << 64) and MOD32_ONE % (1 << 64) != 1
assert all(len(x) == 25 for x in BIG25) and int(BIG25[1]) % (1 << 64) == 1
POSITION_TABLES = {
    "one_long": ([(b"d", U32)], [1, U32, U32 - 1, 1000]),
    "three": ([(b"a", 1), (b"c", 1000), (b"d", U32)], [1000, 1001, 999, U32, 7, 2]),
    "short": ([(b"a", 1), (b"c", 1000)], [1, 1000, 1001, 999, U32, 1 << 20]),
}


@functools.lru_cache(maxsize=None)
def positions_case(which):
    table, res = POSITION_TABLES[which]
    sides = []                                                  # (name, the position as written, whether the side is inside)
    for nm, L in table:
        texts = [b"0", b"1", b"%d" % L, b"%d" % (L + 1), b"0000000001", b"%020d" % L, b"4294967295", b"4294967296", b"4294967297",
                 b"1099511627776", b"1099511627777", b"%d" % MOD64_ONE, b"%d" % MOD32_ONE] + BIG25
        if L > 2:
            texts += [b"%d" % (L - 1), b"2"]
        sides += [(nm, t, 1 <= int(t) <= L) for t in texts]
    lines = []
    for k, (na, ta, _) in enumerate(sides):
        for j, (nb, tb, _) in enumerate(sides):
            lines.append(b"r\t%s\t%s\t%s\t%s%s\n" % (na, ta, nb, tb, TAILS[(5, 6, 7)[(k + j) % 3]]))
    inside = sum(1 for s in sides if s[2])
    case = text_case(table, res, b"".join(lines))
    for r in res:
        cells, skipped = case.want[r]
        assert skipped == len(sides) ** 2 - inside ** 2 and 0 < inside < len(sides) and int(cells[:, 2].sum()) == inside ** 2
        assert int(cells[:, 1].max()) == case.nbins[r] - 1                  # position L of the last chromosome: the last bin
    big = [r for r in res if r >= max(L for _, L in table)]                 # r at or past every L_i: one bin per chromosome
    assert big and all(case.nbins[r] == len(table) for r in big) and U32 in res
    ca, pa, cb, pb = md.parse_pairs(b"r\tx\t%d\tx\t%s\n" % (MOD64_ONE, BIG25[2]))
    assert pa == [md.POS_SAT] and pb == [md.POS_SAT]                        # the definition's cap, as the kernel's
    return case


# ---- 5. line shapes and carry -------------------------------------------------------------------------------------------------------
LINES_TABLE = [(b"chrB", 1000), (b"chrA", 250), (b"chrC", 10)]


@functools.lru_cache(maxsize=None)
def line_shapes_text():
    """five-, six-, seven- and twelve-column lines, '#' lines between them, the last line without its newline"""
    rng = np.random.default_rng(55)
    out = [b"## pairs format v1.0\n", b"#\n"]
    for k in range(40):
        a, c = rng.integers(0, 3, 2)
        La, Lc = LINES_TABLE[a][1], LINES_TABLE[c][1]
        pa = (0 if k % 14 == 0 else La + 1) if k % 7 == 0 else int(rng.integers(1, La + 1))
        out.append(b"id%d\t%s\t%d\t%s\t%d%s\n" % (k, LINES_TABLE[a][0], pa, LINES_TABLE[c][0], int(rng.integers(1, Lc + 1)), TAILS[(5, 6, 7, 12)[k % 4]]))
        if k % 5 == 2:
            out.append(b"#a comment\twith\ttabs\tin\tit\tand\tmore\n")
    out.append(b"last\tchrC\t10\tchrA\t250")
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def line_shapes_case():
    text = line_shapes_text()
    case = text_case(LINES_TABLE, [100, 1], text)
    cells, skipped = case.want[100]
    assert case.pairs == 41 and skipped == 6 and int(cells[:, 2].sum()) == 41 - skipped and not text.endswith(b"\n")
    assert (12, 13) in cell_set(cells)                                      # the last line, which has no newline
    assert text.count(b"\n#") >= 8 and all(any(len(l.split(b"\t")) == c for l in text.split(b"\n") if not l.startswith(b"#")) for c in (5, 6, 7, 12))
    return case


def chunkings(text):
    """{name: pieces}: whole; cut on, before and after every newline; and with a piece that is a single '#'"""
    nl = [i for i, c in enumerate(text) if c == 10]
    cut = lambda at: [text[a:b] for a, b in zip([0] + at, at + [len(text)]) if b > a]
    sharp = text.index(b"\n#a comment") + 1
    out = {"whole": [text], "on": cut([i + 1 for i in nl]), "before": cut(nl), "after": cut([i + 2 for i in nl if i + 2 < len(text)]),
           "sharp": [text[:sharp], text[sharp:sharp + 1], text[sharp + 1:]], "bytes": [text[i:i + 1] for i in range(len(text))]}
    assert out["sharp"][1] == b"#" and all(b"".join(p) == text for p in out.values())
    assert all(p.endswith(b"\n") for p in out["on"][:-1]) and all(p.startswith(b"\n") for p in out["before"][1:]) and all(p[-2:-1] == b"\n" for p in out["after"][:-1])
    return out


# ---- 6. the digits of the COO text ------------------------------------------------------------------------------------------------
COO_TABLE = [(b"c", U32)]
COO_COUNTS = [1000000, 999999, 100000, 99999, 1000, 999, 100, 99, 10, 9]
COO_GROUPS = 4                                                  # whole workgroups of cells in front of the last, partial one


@functools.lru_cache(maxsize=None)
def coo_digits_case():
    """(case, the byte offset at which each workgroup of 1024 cells starts its text)"""
    special = []
    for d in range(1, 10):
        special += [(10 ** d - 1, 10 ** d - 1), (10 ** d - 1, 10 ** d), (10 ** d, 10 ** d)]
    special += [(0, U32 - 1), (U32 - 1, U32 - 1), (10 ** 9, U32 - 1), (9, 10 ** 9), (99999, 999999), (0, 0)]
    count = {c: (COO_COUNTS[k] if k < len(COO_COUNTS) else 1 + k % 3) for k, c in enumerate(special)}
    n_fill = COO_GROUPS * MX_CPW + 100 - len(special)
    for i in range(n_fill):                                     # filler cells; every 50th can go from 9 to 10 pairs: one byte more
        count[(20000 + 3 * i, 20000 + 3 * i + i % 5)] = 9 if i % 50 == 0 else 1
    cells = sorted(count)
    assert len(cells) == COO_GROUPS * MX_CPW + 100
    line_len = lambda c: len(b"%d\t%d\t%d\n" % (c[0], c[1], count[c]))
    for g in range(1, COO_GROUPS):                              # workgroup g is to start at g (mod 4)
        start = sum(line_len(c) for c in cells[:g * MX_CPW])
        need = (g - start) % 4
        spare = [c for c in cells[(g - 1) * MX_CPW:g * MX_CPW] if count[c] == 9 and c not in special]
        assert len(spare) >= 3
        for c in spare[:need]:
            count[c] = 10
    # the input: every cell's pairs as repeated short five-column lines, the expected cells from arrays
    text = b"".join((b".\tc\t%d\tc\t%d\n" % ((c[1] + 1, c[0] + 1) if k % 2 else (c[0] + 1, c[1] + 1))) * count[c] for k, c in enumerate(cells))
    text += b"#end\n.\tc\t0\tc\t1\n.\tc\t4294967296\tc\t1\n"
    cnt = np.array([count[c] for c in cells], dtype=np.int64)
    b1 = np.repeat(np.array([c[0] for c in cells], dtype=np.int64), cnt)
    b2 = np.repeat(np.array([c[1] for c in cells], dtype=np.int64), cnt)
    z = np.zeros(b1.size + 2, dtype=np.int64)
    want = md.definition_arrays(COO_TABLE, [1], z, np.concatenate([b1 + 1, [0, 1 << 32]]), z, np.concatenate([b2 + 1, [1, 1]]))
    case = Case(table_text(COO_TABLE), [1], text, want, int(cnt.sum()) + 2, 2, {1: U32}, {})
    got, skipped = want[1]
    assert skipped == 2 and got.tolist() == [[c[0], c[1], count[c]] for c in cells] and text.count(b"\n") == case.pairs + 1
    assert set(COO_COUNTS) <= set(got[:, 2].tolist()) and 10 ** 6 == int(got[:, 2].max())
    ids = set(got[:, 0].tolist()) | set(got[:, 1].tolist())
    assert all({10 ** d - 1, 10 ** d} <= ids for d in range(1, 10)) and U32 - 1 in ids
    coo = md.coo_text(got)
    starts = [len(md.coo_text(got[:g * MX_CPW])) for g in range(COO_GROUPS + 1)]
    assert [s % 4 for s in starts[:COO_GROUPS]] == [0, 1, 2, 3] and starts[COO_GROUPS] < len(coo)   # on the definition's own text
    return case, starts


# ---- 7. a table that lacks some of a context's chromosomes ----------------------------------------------------------------------------
def partial_table(full_rows, pairs_text):
    """full_rows without the two names the pairs use second and third most, and with the most used one at half its length"""
    use = {}
    for line in pairs_text.split(b"\n"):
        f = line.split(b"\t")
        if len(f) >= 5 and not line.startswith(b"#"):
            use[f[1]] = use.get(f[1], 0) + 1
            use[f[3]] = use.get(f[3], 0) + 1
    by_use = sorted(use, key=lambda k: (-use[k], k))
    halved, gone = by_use[0], set(by_use[1:3])
    rows = [(nm, L // 2 if nm == halved else L) for nm, L in full_rows if nm not in gone]
    assert len(rows) == len(full_rows) - 2 and any(nm == halved for nm, _ in rows)
    return rows, halved, gone
