"""Feature lists of the pileup tests, made once and shared (the callers leave them unchanged).  Imports nothing from the package under
test.  The matrices are those of the loop and insulation tests: loops_inputs.edge_matrix, band_matrix and planted,
insulation_inputs.planted."""
import functools

import numpy as np

import loops_inputs as li

# one chromosome of 6 bins, the cells of the hand-computed cases
HAND = [(0, 0, 5), (0, 1, 2), (0, 2, 9), (1, 1, 4), (1, 2, 3), (2, 3, 1), (3, 3, 7), (3, 4, 2), (4, 5, 6)]
BAND_MIN_DIST = 3            # the band features closer than this are DIST: the ones that keep a slot without contributing


def _arrays(pairs):
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


@functools.lru_cache(maxsize=None)
def edge_features(masked):
    """edge_matrix(masked): every stored cis cell, every (i, i) and the stored trans cells (a few, TRANS) -> (bin1, bin2)"""
    _, _, off, nb, cells, _ = li.edge_matrix(masked)
    offa = np.asarray(off)
    b1, b2 = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
    cis = np.searchsorted(offa, b1, side="right") == np.searchsorted(offa, b2, side="right")
    assert 3 <= (~cis).sum() <= 40
    diag = np.arange(nb)
    return np.concatenate([b1[cis], diag, b1[~cis]]), np.concatenate([b2[cis], diag, b2[~cis]])


@functools.lru_cache(maxsize=None)
def band_base():
    """band_matrix(): 97 features at distances 0 .. 12 along the band, none near an end -> (bin1, bin2); those closer than BAND_MIN_DIST
    are DIST with min_dist = BAND_MIN_DIST"""
    a = 40 + 3 * np.arange(97)
    return a, a + (5 * np.arange(97)) % 13


def band_features(n, holes=True, empty_chunk=False):
    """the base list repeated to n features.  holes: DIST features (distance 0) at slots 0, 255, 256 and 100 (as far as n reaches);
    empty_chunk: every feature of chunk 1 is one."""
    a, b = band_base()
    a, b = np.resize(a, n).copy(), np.resize(b, n).copy()
    if holes:
        for s in (0, 100, 255, 256):
            if s < n:
                b[s] = a[s]
    if empty_chunk:
        b[256:512] = a[256:512]
    return a, b


def without(a, b, status, used=1):
    """the same list with the features that are not used taken out"""
    keep = np.asarray(status) == used
    return np.asarray(a)[keep], np.asarray(b)[keep]


@functools.lru_cache(maxsize=None)
def mirror_features():
    """band_matrix(): (on-diagonal (i, i), off-diagonal with 1 <= b - a < 5) -> two (bin1, bin2)"""
    i = np.arange(30, 370, 7)
    a = np.arange(31, 360, 5)
    return (i, i.copy()), (a, a + 1 + np.arange(a.size) % 4)


@functools.lru_cache(maxsize=None)
def planted_features():
    """the planted pixels of loops_inputs.planted() at 250 kb -> (bin1, bin2)"""
    return _arrays(li.planted()[2][250000])
