"""Inputs of the .hic tests (tests/test_hic_host.py, tests/test_gpu_hic.py): small chromosome tables and pair lists that put cells on
every edge the container has.  A case is a table, bin sizes, pairs as (chrA, posA, chrB, posB, copies), weights and options; its cells
are binned here by the definition of include/mkt.h, its .pairs text is what the GPU is given."""
import random

import hicdef as hd


class Case:
    def __init__(self, chroms, resolutions, pairs=(), opts=None, weights=None, cells=None):
        self.chroms, self.resolutions, self.pairs, self.opts, self.weights = chroms, list(resolutions), list(pairs), dict(opts or {}), weights
        self._cells = cells

    @property
    def table(self):
        return b"".join(n + b"\t%d\n" % L for n, L in self.chroms)

    @property
    def cells(self):
        if self._cells is None:
            lens = [L for _, L in self.chroms]
            self._cells = []
            for r in self.resolutions:
                off, _ = hd.offsets(lens, r)
                acc = {}
                for ca, pa, cb, pb, n in self.pairs:
                    a, b = off[ca] + (pa - 1) // r, off[cb] + (pb - 1) // r
                    key = (min(a, b), max(a, b))
                    acc[key] = acc.get(key, 0) + n
                self._cells.append(sorted((a, b, c) for (a, b), c in acc.items()))
        return self._cells

    def text(self):
        out = [b"## pairs format v1.0\n"]
        for ca, pa, cb, pb, n in self.pairs:
            out.append((b"r\t%s\t%d\t%s\t%d\t+\t-\n" % (self.chroms[ca][0], pa, self.chroms[cb][0], pb)) * n)
        return b"".join(out)


def chrom_of(case, r, b):
    off, nb = hd.offsets([L for _, L in case.chroms], r)
    return max(c for c in range(len(off)) if off[c] <= b and (off[c + 1] if c + 1 < len(off) else nb) > b)


GEO_CHROMS = [(b"chrA", 130), (b"chrB", 70), (b"chrNone", 50), (b"chrC", 110)]     # 13 / 6, 7 / 3, 5 / 2, 11 / 5 bins at 10 / 25 bp: no multiple of 4


def geometry():
    """blocks of 4 bins at 10 and 25 bp: cells on the first and the last bin of every block and in the partial last block row and
    column, a trans pair, a pair without cells (chrB x chrC), a chromosome without pairs (chrNone)"""
    edge = [0, 3, 4, 7, 8, 11, 12]
    pairs = []
    k = 0
    for x in edge:
        for y in edge:
            if x <= y:
                k += 1
                pairs.append((0, 10 * x + 1 + k % 10, 0, 10 * y + 10 - k % 7, 1 + k % 3))
    for x in [0, 3, 4, 12]:
        for y in [0, 3, 4, 6]:
            pairs.append((1, 10 * y + 5, 0, 10 * x + 2, 2))                        # (the second side is the earlier chromosome)
    for x in [0, 6]:
        for y in [0, 3, 4, 7, 8, 10]:
            pairs.append((0, 10 * x + 1, 3, 10 * y + 10, 1))
    pairs += [(3, 110, 3, 110, 4), (3, 1, 3, 110, 1), (1, 70, 1, 70, 1)]
    return Case(GEO_CHROMS, [10, 25], pairs, dict(block_bins=4, genome_id=b"toy1"))


def geometry_direct():
    """the same, with cells given per resolution so that chrB x chrC has cells at 25 bp only (an object cannot make that: its
    resolutions bin the same pairs)"""
    c = geometry()
    cells = [list(v) for v in c.cells]
    off, _ = hd.offsets([L for _, L in GEO_CHROMS], 25)
    cells[1] = sorted(cells[1] + [(off[1] + 2, off[3] + 4, 9)])
    w = [[1.0 + 0.25 * i if i % 5 else float("nan") for i in range(hd.offsets([L for _, L in GEO_CHROMS], 10)[1])], None]
    return Case(GEO_CHROMS, [10, 25], (), dict(block_bins=4, genome_id=b"toy1", norm_label=b"KR"), w, cells)


def _rows(width, target):
    """cells (x, y) row by row, `width` a row, until rows + records is `target`"""
    out, y = [], 0
    while target > 0:
        k = min(width, target - 1)
        out += [(x, y) for x in range(k)]
        target -= k + 1
        y += 1
    return out


TRANS = [(b"p", 200000), (b"q", 200000)]


def payload_of(n_rows_plus_records):
    """one short block of a trans pair at 1 kb whose payload is 16 + 4 * (rows + records) bytes"""
    return Case(TRANS, [1000], [(0, 1000 * x + 1, 1, 1000 * y + 1, 1) for x, y in _rows(150, n_rows_plus_records)], dict(block_bins=1000))


def triangle():
    """one chromosome of 256 bins, every upper-triangle cell: 32896 records in 256 rows, 132624 bytes, three pieces"""
    return Case([(b"t", 256000)], [1000], [(0, 1000 * x + 1, 0, 1000 * y + 1, 1) for x in range(256) for y in range(x, 256)], dict(block_bins=256))


def noisy():
    """a multi-piece payload that codes badly: 17000 records of a trans block whose counts come from a fixed-seed generator, 1 .. 255
    (more would take hundreds of millions of pairs: a count is that many lines)"""
    rng = random.Random(20250611)
    return Case(TRANS, [1000], [(0, 1000 * x + 1, 1, 1000 * y + 1, rng.randint(1, 255)) for x, y in _rows(150, 17114)], dict(block_bins=1000))


def widths():
    """two neighbouring blocks of 4 bins: one holds a cell of exactly 32768 pairs (float), the other one of exactly 32767 (short)"""
    return Case([(b"w", 160)], [10], [(0, 15, 0, 25, 32768), (0, 5, 0, 5, 3), (0, 45, 0, 55, 32767), (0, 65, 0, 75, 2)], dict(block_bins=4))


HOST_CASES = dict(geometry=geometry_direct, pairs=geometry, exact=lambda: payload_of(16316), four_more=lambda: payload_of(16317), widths=widths)
