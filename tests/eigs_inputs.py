"""Inputs of the compartment-eigenvector tests, made once and shared (the callers leave them unchanged).  Imports nothing from the
package under test: the cells come from the matrix definition.

A planted matrix: distance decay times 1 + a1 s1 s1^T + a2 s2 s2^T + a3 s3 s3^T with three mutually orthogonal +-1 patterns (Hadamard
rows under one random permutation and sign change, so that their autocorrelation along the chromosome is small and E[d] stays the decay) and a depth of tens of contacts per near-diagonal cell, so that cis is dense: at 40 contacts the
plain noise eigenvalues crowd lambda_3 of weaker patterns, at 3 they swamp everything."""
import functools

import numpy as np

import expected_inputs as xi
import loops_inputs as li
import matrixdef as md

R = 1000
STRENGTHS = (0.45, 0.27, 0.16)                           # their sum stays below 1: every mean is positive
PLANT_BINS = [64, 6, 128]                                  # the 6-bin chromosome is below min_good: skipped
PLANT_DEPTH = 90.0


def patterns(n, rng):
    """three mutually orthogonal +-1 patterns of length n (a power of two): rows of the Sylvester Hadamard matrix, columns permuted and
    signs changed by one random draw"""
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n
    return (H[[3, 5, 6]] * rng.choice(np.array([-1.0, 1.0]), n))[:, rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def planted(seed=11):
    """-> (table text, .pairs text, offsets, nbins, cells (k, 3), phasing track [nbins])"""
    rows, ttext, trows = li.table_of(PLANT_BINS, R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(seed)
    b1, b2, cnt = [], [], []
    track = np.full(nb, np.nan)
    for c, n in enumerate(PLANT_BINS):
        if n < 9:
            for x in range(n):
                for y in range(x, n):
                    b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(int(rng.poisson(20)) + 1)
            continue
        s = patterns(n, rng)
        track[off[c]:off[c] + n] = s[0] - 0.6 * s[1] + 0.5 * s[2] + 0.3 * rng.standard_normal(n)
        track[off[c] + 5] = np.nan                                         # a bin without a value
        i, j = np.triu_indices(n)
        decay = PLANT_DEPTH / (1.0 + (j - i) / 12.0)
        mean = decay * (1.0 + sum(a * s[k][i] * s[k][j] for k, a in enumerate(STRENGTHS)))
        draw = rng.poisson(mean)
        for x, y, q in zip(i.tolist(), j.tolist(), draw.tolist()):
            if q:
                b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(q)
    text = li.text_of(rows, R, off, b1, b2, cnt)
    cells = md.definition(ttext, [R], text)[R][0]
    return ttext, text, off, nb, cells, track


SHAPE_BINS = [256, 257, 1300, 30]                          # the reduction chunk, one bin more, long rows, and a small one


@functools.lru_cache(maxsize=None)
def shapes():
    """A sparse band matrix over chromosomes of exactly the reduction chunk (256 bins) and one bin more, and a 1 300-bin chromosome in
    which three bins touch nearly every other bin (row plus column above 1 024 cells: the long-row path) next to ordinary rows.
    -> (table text, .pairs text, offsets, nbins, cells)"""
    rows, ttext, trows = li.table_of(SHAPE_BINS, R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(3)
    cell = {}
    for c, n in enumerate(SHAPE_BINS):
        for x in range(n):
            for y in range(x, min(n, x + 5)):
                if rng.random() < 0.8:
                    cell[(off[c] + x, off[c] + y)] = int(rng.integers(1, 4))
    for h in (0, 640, 1299):                                               # first, middle and last bin of the long chromosome
        for y in range(SHAPE_BINS[2]):
            if rng.random() < 0.9:
                a, b = sorted((off[2] + h, off[2] + y))
                cell[(a, b)] = int(rng.integers(1, 4))
    keys = sorted(cell)
    text = li.text_of(rows, R, off, [k[0] for k in keys], [k[1] for k in keys], [cell[k] for k in keys])
    cells = md.definition(ttext, [R], text)[R][0]
    return ttext, text, off, nb, cells
