"""Inputs of the saddle tests, made once and shared (the callers leave them unchanged).  Imports nothing from the package under test:
the cells come from the matrix definition.  Every builder asserts what it is there for before it returns."""
import functools

import numpy as np

import expected_inputs as xi
import loops_inputs as li
import matrixdef as md
import saddledef as sd

R = li.R_EDGE
CHUNK_BINS = [100, 100]
CHUNK_MIN_DIAG = 2
# the chunk matrices and the number of chunks that must hold used cells: (cis, trans).  The last stored cell is a trans cell and the
# one before it a cis cell, so at 4097 and 8193 cells the trans entries reach into the chunk of one cell and the cis entries do not.
CHUNK_CASES = {1: (0, 1), 4095: (1, 1), 4096: (1, 1), 4097: (1, 2), 8192: (2, 2), 8193: (2, 3)}


def brute_positions(g, off, nbins, Q, contact, min_diag, max_diag):
    """step 4 by a double loop over the pairs of bins: the yardstick of the prefix-count versions"""
    chrom = sd.chrom_of(off, nbins)
    n = np.zeros((Q, Q), dtype=np.uint64)
    for i in range(nbins):
        if g[i] == sd.NONE:
            continue
        for j in range(i, nbins):
            if g[j] == sd.NONE:
                continue
            if contact == "cis":
                d = j - i
                ok = chrom[i] == chrom[j] and d >= min_diag and (not max_diag or d <= max_diag)
            else:
                ok = chrom[i] != chrom[j]
            if ok:
                a, b = min(g[i], g[j]), max(g[i], g[j])
                n[a][b] += 1
    return n


@functools.lru_cache(maxsize=None)
def chunk_matrix(ncells):
    """Two chromosomes of 100 bins with exactly ncells stored cells, all in the rows of the first chromosome, so that cis and trans cells
    alternate along the cell order and the cells that one contact does not use keep slots in every chunk.
    -> (table text, .pairs text, offsets, nbins, cells (k, 3), track [nbins])"""
    rows, ttext, trows = li.table_of(CHUNK_BINS, R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(17)
    i, j = np.meshgrid(np.arange(100), np.arange(200), indexing="ij")
    cis_last, trans_last = 97 * 200 + 99, 97 * 200 + 199                       # the two last cells: (97, 99), cis at distance 2, then (97, 199), trans
    universe = np.flatnonzero((j >= i).ravel())                                # cell index i * 200 + j: ascending = the stored order
    universe = universe[universe < cis_last]
    last = np.array([cis_last, trans_last][max(0, 2 - ncells):], dtype=np.int64)
    pick = np.sort(np.concatenate([rng.choice(universe, ncells - last.size, replace=False), last]))
    b1, b2 = pick // 200, pick % 200
    cnt = rng.integers(1, 4, ncells)
    text = li.text_of(rows, R, off, b1, b2, cnt)
    cells = md.definition(ttext, [R], text)[R][0]
    assert cells.shape[0] == ncells and (cells[:, 0] == b1).all() and (cells[:, 1] == b2).all()
    track = rng.standard_normal(nb)
    cis = (b2 < 100) & (b2 - b1 >= CHUNK_MIN_DIAG)
    trans = b2 >= 100
    chunk = np.arange(ncells) // sd.CHUNK
    got = (np.unique(chunk[cis]).size, np.unique(chunk[trans]).size)
    assert got == CHUNK_CASES[ncells], (ncells, got)
    if ncells > 1:
        assert not cis[-1] and trans[-1] and b2[-2] < 100                      # unused cells keep slots: the last cis cell is not the last cell
    return ttext, text, off, nb, cells, track


def chunk_entry_spans(cells, g, off, nb, contact, Q):
    """per unordered entry the number of chunks that hold used cells of it: the most any entry spans"""
    used, a, b = sd.used_cells(cells[:, 0], cells[:, 1], g, sd.chrom_of(off, nb), contact, CHUNK_MIN_DIAG, 0)
    chunk = np.arange(cells.shape[0]) // sd.CHUNK
    e = (a * Q + b)[used]
    return max((np.unique(chunk[used][e == x]).size for x in np.unique(e)), default=0)


@functools.lru_cache(maxsize=None)
def group_tracks():
    """tracks over the bins of loops_inputs.edge_matrix (183 bins) -> {name: track}"""
    nb = li.edge_matrix(False)[3]
    rng = np.random.default_rng(23)
    few = np.full(nb, np.nan)
    few[rng.choice(nb, 40, replace=False)] = rng.standard_normal(40)
    zeros = np.where(np.arange(nb) % 2 == 0, -0.0, 0.0)
    zeros[5], zeros[77], zeros[150] = -np.inf, np.inf, 1.0
    full = rng.standard_normal(nb)
    full[[3, 20]] = np.nan
    out = dict(full=full, few=few, nan=np.full(nb, np.nan), constant=np.full(nb, 2.5), zeros=zeros)
    assert np.isfinite(few).sum() == 40 < 50 and np.signbit(zeros).sum() > 80 and (zeros == 0).sum() == nb - 3
    return out


def empty_groups(track, valid, Q, trim_lo, trim_hi):
    """the groups without a bin"""
    return int((sd.groups(track, valid, Q, trim_lo, trim_hi)[1] == 0).sum())


@functools.lru_cache(maxsize=None)
def flat(k=3):
    """loops_inputs.flat_matrix: one chromosome of 30 bins, every cell stored with k contacts; a track without ties"""
    ttext, text, off, nb, cells = li.flat_matrix(k)
    assert cells.shape[0] == 30 * 31 // 2 and (cells[:, 2] == k).all()
    return ttext, text, off, nb, cells, np.random.default_rng(2).standard_normal(nb)
