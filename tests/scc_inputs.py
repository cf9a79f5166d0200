"""Inputs of the replicate-comparison tests, made once and shared (the callers leave them unchanged).  Imports nothing from the package
under test: the cells come from the matrix definition, the expectations from tests/sccdef.py.  Every builder asserts what it is there
for before it returns.  A pair of replicates is Rep(ttext, text_a, text_b, off, nb, cells_a, cells_b)."""
import collections
import functools

import numpy as np

import expected_inputs as xi
import loops_inputs as li
import matrixdef as md
import sccdef as sd

R = li.R_EDGE
Rep = collections.namedtuple("Rep", "ttext text_a text_b off nb cells_a cells_b")
CHUNK_BINS = (1, 2, 255, 256, 257, 512, 513)
CHUNK_H, CHUNK_MAX_DIAG = 1, 3
WINDOW_BINS = (40, 7)
WINDOW_HS = (0, 1, 2, 5)
WINDOW_MAX_DIAG = 12
SLAB_BINS = 600


def _cells(ttext, text):
    return md.definition(ttext, [R], text)[R][0]


def _draw(rng, bins, width, lam, skip=()):
    """per chromosome a band of `width` diagonals with Poisson counts that fall with the distance; no cell touches a bin of `skip`"""
    off = np.concatenate([[0], np.cumsum(bins)])[:-1]
    b1, b2, cnt = [], [], []
    for c, n in enumerate(bins):
        for x in range(n):
            for y in range(x, min(n, x + width)):
                k = int(rng.poisson(lam / (1.0 + (y - x))))
                if k and not ({int(off[c]) + x, int(off[c]) + y} & set(skip)):
                    b1.append(int(off[c]) + x); b2.append(int(off[c]) + y); cnt.append(k)
    return b1, b2, cnt


def _rep(bins, seed, width=8, lam=4.0, skip_a=(), skip_b=(), extra_a=(), extra_b=()):
    rows, ttext, trows = li.table_of(list(bins), R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(seed)
    texts, cells = [], []
    for skip, extra in ((skip_a, extra_a), (skip_b, extra_b)):
        b1, b2, cnt = _draw(rng, bins, width, lam, skip)
        for x, y, k in extra:
            b1.append(x); b2.append(y); cnt.append(k)
        texts.append(li.text_of(rows, R, off, b1, b2, cnt))
        cells.append(_cells(ttext, texts[-1]))
    return Rep(ttext, texts[0], texts[1], off, nb, cells[0], cells[1])


def want(rep, cells_a=None, cells_b=None, **opts):
    """the definition on the builder's own cells (the tests feed it the GPU's)"""
    ca = rep.cells_a if cells_a is None else cells_a
    cb = rep.cells_b if cells_b is None else cells_b
    return sd.scc(tuple(ca[:, k] for k in range(3)), tuple(cb[:, k] for k in range(3)), rep.nb, rep.off, **opts)


@functools.lru_cache(maxsize=None)
def chunk_edges(nc):
    """one chromosome of nc bins: with max_diag 3 the stratum lengths nc - d cross 256 and 512 from both sides over CHUNK_BINS"""
    rep = _rep((nc,), 100 + nc, width=6)
    lengths = {n - d for n in CHUNK_BINS for d in range(CHUNK_MAX_DIAG + 1)}
    assert {255, 256, 257, 511, 512, 513} <= lengths and {1, 0, -1} & lengths
    assert rep.cells_a.shape[0] >= 1 and rep.cells_b.shape[0] >= 1 and (nc < 255 or rep.cells_a.tobytes() != rep.cells_b.tobytes())
    return rep


@functools.lru_cache(maxsize=None)
def window_edges():
    """chromosomes of 40 and 7 bins, the second shorter than the window (h = 5) and than the band (max_diag 12), with heavy trans cells
    and dense neighbours: -> (the replicates, the same with only the first chromosome's cis cells, the same with only the second's)"""
    heavy = [(3, 41, 500), (39, 40, 700), (20, 46, 900), (0, 45, 300)]          # trans cells next to the chromosome edge and far from it
    full = _rep(WINDOW_BINS, 7, width=20, lam=6.0, extra_a=heavy, extra_b=[(x, y, 2 * k) for x, y, k in heavy])
    rows, ttext, trows = li.table_of(list(WINDOW_BINS), R)
    only = []
    for c in (0, 1):
        lo, hi = full.off[c], full.off[c] + WINDOW_BINS[c]
        parts = []
        for cells in (full.cells_a, full.cells_b):
            keep = cells[(cells[:, 0] >= lo) & (cells[:, 1] < hi)].astype(np.int64)
            parts.append(li.text_of(rows, R, full.off, keep[:, 0], keep[:, 1], keep[:, 2]))
        only.append(Rep(ttext, parts[0], parts[1], full.off, full.nb, _cells(ttext, parts[0]), _cells(ttext, parts[1])))
    for cells in (full.cells_a, full.cells_b):
        trans = (cells[:, 0] < 40) & (cells[:, 1] >= 40)
        assert trans.sum() == 4 and cells[trans, 2].min() >= 300                # heavy trans cells ...
        assert ((cells[:, 0] >= 40).sum() >= 15) and ((cells[:, 1] < 40).sum() >= 300)      # ... and cells of the neighbour chromosome
    assert WINDOW_BINS[1] < 2 * max(WINDOW_HS) + 1 and WINDOW_BINS[1] < WINDOW_MAX_DIAG
    assert only[0].cells_a.shape[0] < full.cells_a.shape[0] and (only[0].cells_a[:, 1] < 40).all() and (only[1].cells_a[:, 0] >= 40).all()
    return full, only[0], only[1]


MASK_BINS = (60, 30)
MASK_A, MASK_B, MASK_BOTH = (0, 17, 59, 75), (5, 6, 89), (30, 31, 60)              # global bins without a contact


@functools.lru_cache(maxsize=None)
def masked():
    """bins without a contact only in A, only in B and in both (first, last and interior bins of a chromosome among them): after
    balancing they are the masked bins"""
    rep = _rep(MASK_BINS, 19, width=12, lam=5.0, skip_a=MASK_A + MASK_BOTH, skip_b=MASK_B + MASK_BOTH)
    bare = [set(range(rep.nb)) - set(c[:, 0].tolist()) - set(c[:, 1].tolist()) for c in (rep.cells_a, rep.cells_b)]
    assert bare[0] == set(MASK_A + MASK_BOTH) and bare[1] == set(MASK_B + MASK_BOTH)
    only_a, only_b, both = bare[0] - bare[1], bare[1] - bare[0], bare[0] & bare[1]
    assert only_a and only_b and both                                           # each kind occurs
    valid = np.ones(rep.nb, dtype=bool)
    valid[sorted(bare[0] | bare[1])] = False
    h = 3
    P = np.concatenate([[0], np.cumsum(valid[:60])])
    k = np.arange(60)
    nv = P[np.minimum(k + h, 59) + 1] - P[np.maximum(k - h, 0)]
    clipped = np.minimum(k + h, 59) - np.maximum(k - h, 0) + 1
    assert (nv[valid[:60]] < clipped[valid[:60]]).any() and (nv[valid[:60]] == clipped[valid[:60]]).any()      # a window with fewer valid bins than its clipped length
    return rep, sorted(bare[0]), sorted(bare[1])


USED_OPTS = dict(h=0, min_diag=0, max_diag=3, min_n=3)


@functools.lru_cache(maxsize=None)
def used_and_scored():
    """one chromosome of 30 bins at h = 0 (x is the cell itself).  Diagonal 0: varied counts, some positions empty in both maps
    (0 < n < n_cand, scored).  Diagonal 1: every cell of A holds 2 (x is constant: rho NaN, w 0).  Diagonal 2: two used positions
    (n < min_n).  Diagonal 3: varied in both (scored)."""
    rows, ttext, trows = li.table_of([30], R)
    off, nb = xi.offsets(R, trows)
    rng = np.random.default_rng(3)
    texts, cells = [], []
    for side in range(2):
        b1, b2, cnt = [], [], []
        for i in range(30):
            if i % 5 != 4:                                                      # bins 4, 9, .. are empty on the diagonal of both maps
                b1.append(i); b2.append(i); cnt.append(int(rng.integers(1, 9)))
        for i in range(29):
            b1.append(i); b2.append(i + 1); cnt.append(2 if side == 0 else int(rng.integers(1, 6)))
        for i in (3, 11):
            b1.append(i); b2.append(i + 2); cnt.append(1 + side + i)
        for i in range(27):
            b1.append(i); b2.append(i + 3); cnt.append(int(rng.integers(1, 7)))
        texts.append(li.text_of(rows, R, off, b1, b2, cnt))
        cells.append(_cells(ttext, texts[-1]))
    rep = Rep(ttext, texts[0], texts[1], off, nb, cells[0], cells[1])
    w = want(rep, **USED_OPTS)
    assert 0 < w.n[0] < w.n_cand[0] and w.n[0] == 24 and not np.isnan(w.rho[0]) and w.w[0] == 24.0
    assert w.n[1] == 29 and np.isnan(w.rho[1]) and w.w[1] == 0.0                # constant x
    assert w.n[2] == 2 and np.isnan(w.rho[2]) and w.w[2] == 0.0                 # n < min_n
    assert not np.isnan(w.rho[3]) and w.info["scored"] == 2
    return rep


@functools.lru_cache(maxsize=None)
def slabs():
    """one chromosome of 600 bins (three chunks, so slabs of 256 rows, of 512 rows and one slab differ) and a short second one"""
    rep = _rep((SLAB_BINS, 9), 23, width=10, lam=3.0)
    assert -(-SLAB_BINS // sd.CHUNK) == 3
    return rep
