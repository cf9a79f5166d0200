"""The replicate comparison's definition (tests/sccdef.py, restating mkt_matrix_scc of include/mkt.h) against a brute-force walk of
every position and its window, and the properties the definition promises.  No GPU."""
import math

import numpy as np
import pytest

import scc_inputs as si
import sccdef as sd


def _brute(cells_a, cells_b, nbins, off, h, min_diag, max_diag, wa=None, wb=None, min_n=3, weighting=0):
    """position by window, plain Python: the same additions in the same order, written as loops"""
    valid = [True] * nbins if wa is None else [not (math.isnan(wa[k]) or math.isnan(wb[k])) for k in range(nbins)]
    nchr = len(off)
    ncs = [(off[c + 1] if c + 1 < nchr else nbins) - off[c] for c in range(nchr)]
    rows = []
    for c in range(nchr):
        lo, nc = off[c], ncs[c]
        F = []
        for cells, w in ((cells_a, wa), (cells_b, wb)):
            f = {}
            for a, b, k in cells:
                a, b, k = int(a), int(b), int(k)
                if lo <= a and b < lo + nc and valid[a] and valid[b]:
                    v = float(k) if w is None else (float(k) * float(w[a])) * float(w[b])
                    f[(a - lo, b - lo)] = f[(b - lo, a - lo)] = v
            F.append(f)

        def smooth(f, i, j):
            W = None
            for ii in range(i - h, i + h + 1):
                r = None
                for jj in range(j - h, j + h + 1):
                    t = f.get((ii, jj), 0.0) if 0 <= ii < nc and 0 <= jj < nc else 0.0
                    r = t if r is None else r + t
                W = r if W is None else W + r
            nv = lambda a, b: sum(valid[lo + k] for k in range(max(a, 0), min(b, nc - 1) + 1))
            return W / float(nv(i - h, i + h) * nv(j - h, j + h))

        for d in range(min_diag, max_diag + 1):
            slots = [[0.0] * 5 for _ in range(max(nc - d, 0))]
            n = ncand = 0
            for i in range(max(nc - d, 0)):
                if valid[lo + i] and valid[lo + i + d]:
                    ncand += 1
                    x, y = smooth(F[0], i, i + d), smooth(F[1], i, i + d)
                    if x != 0 or y != 0:
                        n += 1
                        slots[i] = [x, y, x * x, y * y, x * y]
            sums = []
            for k in range(5):
                tot = None
                for q in range(0, len(slots), 256):
                    s = [slots[q + t][k] if q + t < len(slots) else 0.0 for t in range(256)]
                    half = 128
                    while half:
                        for t in range(half):
                            s[t] = s[t] + s[t + half]
                        half //= 2
                    tot = s[0] if tot is None else tot + s[0]
                sums.append(0.0 if tot is None else tot)
            rows.append((ncand, n, *sums, *sd.score(n, *sums, weighting, min_n)[:2]))
    return rows


def _inputs(mask):
    rng = np.random.default_rng(5)
    off, nb = [0, 12], 17
    cells = []
    for _ in range(2):
        c = [(a, b, int(rng.integers(1, 9))) for a in range(nb) for b in range(a, nb) if rng.random() < 0.6]
        c.append((2, 14, 50))                                                    # a trans cell
        cells.append(np.array(sorted(c), dtype=np.int64))
    wa = wb = None
    if mask:
        wa, wb = rng.uniform(0.5, 1.5, nb), rng.uniform(0.5, 1.5, nb)
        wa[[0, 5]] = np.nan
        wb[[5, 11, 14]] = np.nan
    return cells, off, nb, wa, wb


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("h", [0, 1, 3])
def test_definition_equals_brute_force(h, mask):
    cells, off, nb, wa, wb = _inputs(mask)
    got = sd.scc(tuple(cells[0].T), tuple(cells[1].T), nb, off, h=h, min_diag=0, max_diag=0, weights_a=wa, weights_b=wb)
    rows = _brute(cells[0], cells[1], nb, off, h, 0, 11, wa, wb)
    assert got.info["strata"] == 12 and len(rows) == 24
    for k, row in enumerate(rows):
        for f, v in zip(sd.STRATA, row):
            a = getattr(got, f)[k]
            assert np.array(a).tobytes() == np.array(v, dtype=a.dtype).tobytes(), (k, f, a, v)
    assert got.info["scored"] > 4 and got.n[12 + 5:24].sum() == 0                # strata with d >= n_c are empty
    if mask:
        assert got.info["candidates"] < sd.scc(tuple(cells[0].T), tuple(cells[1].T), nb, off, h=h).info["candidates"]


@pytest.mark.parametrize("weighting", ["n", "var"])
def test_exchange_is_byte_exact(weighting):
    rep = si.window_edges()[0]
    ab = si.want(rep, h=2, max_diag=12, weighting=weighting)
    ba = si.want(rep, cells_a=rep.cells_b, cells_b=rep.cells_a, h=2, max_diag=12, weighting=weighting)
    swapped = si.want(rep, h=2, max_diag=12, weighting=weighting, swap=True)
    for f in sd.FIELDS:
        assert getattr(ba, f).tobytes() == getattr(swapped, f).tobytes(), f
    for f, g in (("sx", "sy"), ("sxx", "syy"), ("sxy", "sxy"), ("rho", "rho"), ("w", "w"), ("n", "n"), ("scc", "scc"), ("num", "num"), ("den", "den")):
        assert getattr(ab, f).tobytes() == getattr(ba, g).tobytes(), f
    assert ab.info["count_a"] == ba.info["count_b"] and np.array(ab.info["scc"]).tobytes() == np.array(ba.info["scc"]).tobytes()


def test_self_comparison_is_one():
    for rep, o in ((si.window_edges()[0], dict(h=1, max_diag=12)), (si.used_and_scored(), si.USED_OPTS), (si.chunk_edges(257), dict(h=1, max_diag=3, weighting="var"))):
        r = si.want(rep, cells_b=rep.cells_a, **o)
        assert r.info["scored"] > 0 and abs(r.info["scc"] - 1.0) < 1e-12
        ok = ~np.isnan(r.rho)
        assert ok.sum() == r.info["scored"] and (np.abs(r.rho[ok] - 1.0) < 1e-12).all()
        assert (np.abs(r.scc[r.n_scored > 0] - 1.0) < 1e-12).all() and np.isnan(r.scc[r.n_scored == 0]).all()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700])
def test_chunk_tree_is_a_plain_sum_on_integers(n):
    v = np.random.default_rng(n).integers(0, 1000, n).astype(np.float64)
    assert sd.chunk_tree(v) == float(v.sum()) == float(sum(int(x) for x in v))


def test_builders_hold_what_they_promise():
    for nc in si.CHUNK_BINS:
        si.chunk_edges(nc)
    si.masked()
    si.slabs()
    rep = si.used_and_scored()
    w = si.want(rep, **si.USED_OPTS)
    assert w.info["strata"] == 4 and w.info["candidates"] == 30 + 29 + 28 + 27
