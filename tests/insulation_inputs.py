"""Inputs of the insulation tests, made once and shared (the callers leave them unchanged).  Imports nothing from the package under
test: the cells come from the matrix definition."""
import functools

import numpy as np

import expected_inputs as xi
import loops_inputs as li
import matrixdef as md

R = 1000
# planted domains, per chromosome, in bins: dense inside, sparse between
DOMAINS = ([12, 30, 10, 17, 25, 14, 21], [16, 11, 28])
BAND_BINS, BAND_DIST = [3, 300, 70], 140


def _cells_of(ttext, text):
    return md.definition(ttext, [R], text)[R][0]


@functools.lru_cache(maxsize=None)
def planted():
    """Block-diagonal chromosomes: 240 // size contacts on every cell inside a domain (every bin then has about the same total, so
    that balancing leaves the picture as it is), and one contact on a third of the cells up to distance 12 between domains.
    -> (table text, .pairs text, offsets, nbins, cells (k, 3), edges): edges = the first bin of every domain that does not start its
    chromosome."""
    rows, ttext, trows = li.table_of([sum(d) for d in DOMAINS], R)
    off, nb = xi.offsets(R, trows)
    b1, b2, cnt, edges = [], [], [], []
    for c, sizes in enumerate(DOMAINS):
        dom, inside = np.repeat(np.arange(len(sizes)), sizes), np.repeat(240 // np.asarray(sizes), sizes)
        edges += [off[c] + int(e) for e in np.cumsum(sizes)[:-1]]
        for x in range(dom.size):
            for y in range(x, dom.size):
                d = y - x
                n = int(inside[x]) if dom[x] == dom[y] else int(d <= 12 and (x + y) % 3 == 0)
                if n:
                    b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(n)
    text = li.text_of(rows, R, off, b1, b2, cnt)
    return ttext, text, off, nb, _cells_of(ttext, text), edges


def boundaries_are_the_planted(boundary, edges):
    """the rule of the planted input: a boundary within one bin of every planted edge, and no boundary further than one bin from one"""
    found = np.flatnonzero(boundary).tolist()
    return all(any(abs(b - e) <= 1 for b in found) for e in edges) and all(any(abs(b - e) <= 1 for e in edges) for b in found)


@functools.lru_cache(maxsize=None)
def band():
    """A chromosome of 300 bins with every cell up to distance 140 stored (1 .. 4 contacts), between one of 3 bins and one of 70 bins
    (all cells stored).  -> (table text, .pairs text, offsets, nbins, cells)"""
    rows, ttext, trows = li.table_of(BAND_BINS, R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(17)
    b1, b2, cnt = [], [], []
    for c, n in enumerate(BAND_BINS):
        for x in range(n):
            for y in range(x, min(n, x + BAND_DIST + 1)):
                b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(int(rng.integers(1, 5)))
    text = li.text_of(rows, R, off, b1, b2, cnt)
    return ttext, text, off, nb, _cells_of(ttext, text)
