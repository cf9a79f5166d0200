"""The loop-calling checker itself (tests/loopsdef.py), without a GPU: the vectorised cell pass against a position-by-position
version on a 40-bin matrix, the edge table, the threshold recurrence, the clustering; and the binding lists the new entry points."""
import math

import numpy as np

import expecteddef as ed
import loopsdef as ld


def _small(seed, masked=()):
    rng = np.random.default_rng(seed)
    off, nb = [0, 40, 47], 60
    dense = np.zeros((nb, nb), dtype=np.int64)
    for lo, hi in ((0, 40), (40, 47), (47, 60)):
        for x in range(lo, hi):
            for y in range(x, hi):
                if rng.random() < 0.7:
                    dense[x, y] = dense[y, x] = int(rng.integers(1, 6))
    dense[3, 45] = dense[45, 3] = 2                                          # a trans cell
    for k in masked:
        dense[k, :] = 0
        dense[:, k] = 0
    b1, b2 = np.nonzero(np.triu(dense))
    cnt = dense[b1, b2]
    w = None
    if masked:
        w = np.random.default_rng(seed + 1).uniform(0.5, 2.0, nb)
        w[list(masked)] = np.nan
    return dense, b1, b2, cnt, off, nb, w


def test_cell_pass_against_brute_force():
    seen, statuses = set(), set()
    for seed, masked, opts in ((1, (), dict(min_dist=0, window=3, window_max=6, peak=1, min_ll_count=30)), (2, (0, 17, 39, 41), dict(min_dist=2, window=4, window_max=9, min_ll_count=25)),
                               (3, (), dict())):
        dense, b1, b2, cnt, off, nb, w = _small(seed, masked)
        E = ed.expected(b1, b2, cnt, nb, off, weights=w).genome.expected_smooth
        got = ld.cells_pass(b1, b2, cnt, nb, off, E, weights=w, **opts)
        o = ld.options(**opts)
        ww = np.ones(nb) if w is None else w
        valid = ~np.isnan(ww)
        bounds = off + [nb]
        for s in range(b1.size):
            i, j = int(b1[s]), int(b2[s])
            c = max(k for k in range(3) if off[k] <= i)
            cand = j < bounds[c + 1] and valid[i] and valid[j] and j - i >= o["min_dist"]
            assert (got.status[s] != ld.NONE) == bool(cand)
            if not cand:
                assert got.window[s] == 0 and (got.chunk[s] == ld.NOCHUNK).all() and np.isnan(got.r[s]).all()
                continue
            win, cs, bs, es, kp = ld.brute_cell(dense, valid, bounds[c], bounds[c + 1], E, ww, i, j, **opts)
            assert (got.window[s], int(got.csum_ll[s]), got.kept[s].tolist()) == (win, cs, kp)
            seen.add(win)
            for R in range(4):
                assert math.isclose(got.bsum[s, R], bs[R], rel_tol=1e-13, abs_tol=0) and math.isclose(got.esum[s, R], es[R], rel_tol=1e-13, abs_tol=0)
                if kp[R] and es[R] != 0.0:
                    r = (bs[R] / es[R]) * E[j - i] / (ww[i] * ww[j])
                    assert math.isclose(got.r[s, R], r, rel_tol=1e-12, abs_tol=0)
                    k = min(k for k in range(ld.NCHUNK) if r <= ld.EDGES[k]) if r <= 512 else ld.NOCHUNK
                    assert got.chunk[s, R] == k or abs(r / ld.EDGES[min(k, 27) - (got.chunk[s, R] < k)] - 1) < 1e-12
                else:
                    assert np.isnan(got.r[s, R]) and got.chunk[s, R] == ld.NOCHUNK
            undef = any(not (kp[R] and es[R] != 0.0) for R in range(4))
            assert (got.status[s] == ld.UNDEFINED) == undef
        statuses |= set(got.status.tolist())
    assert statuses >= {ld.NONE, ld.TESTED, ld.UNDEFINED}
    assert len(seen) >= 5, seen                                               # the window did grow, and did not always


def test_region_shapes():
    D, LL, H, V = ld.region_offsets(5, 2)
    assert len(D) == 11 * 11 - 25 - 2 * (11 - 5) - 0 and (1, -1) not in LL and (3, -1) in LL and (1, -3) in LL and len(LL) == 25 - 4
    assert len(H) == 3 * 6 and len(V) == 3 * 6 and set(LL) <= set(D) and all(a != 0 and b != 0 for a, b in D)
    for R in (D, LL, H, V):
        assert R == sorted(R)


def test_edge_table():
    assert ld.EDGES.size == 28 and (np.diff(ld.EDGES) > 0).all() and ld.EDGES[0] == 1.0 and ld.EDGES[27] == 512.0
    assert ld.EDGES[3] == 2.0 and ld.EDGES[4] == 2 * 1.2599210498948732 and abs(ld.EDGES[1] ** 3 - 2.0) < 1e-15


def test_threshold_recurrence():
    Q = ld.tail_table(0)                                                      # lambda = 1
    assert Q[0] == 1.0 and Q[1] == 1.0 - math.exp(-1.0) and abs(Q[2] - (1.0 - 2.0 * math.exp(-1.0))) < 1e-15
    assert all(a >= b for a, b in zip(Q, Q[1:])) and Q[-1] == 0.0 and len(Q) == 2049
    H = np.zeros((4, 28, 2048), dtype=np.uint64)
    rng = np.random.default_rng(9)
    lam = float(ld.EDGES[6])                                                  # 4: Poisson counts and 40 outliers
    x = np.concatenate([rng.poisson(lam, 5000), np.full(40, 30)])
    np.add.at(H[1, 6], x, 1)
    H[2, 9, 2047] = 3                                                         # only the last column
    T = ld.thresholds(H, 0.1)
    assert T.shape == (4, 28) and T[0, 0] == 2048 and T[1, 5] == 2048
    t = int(T[1, 6])
    O = lambda v: int((x >= v).sum())
    Q6 = ld.tail_table(6)
    assert 1 <= t <= 30 and 5040 * Q6[t] <= 0.1 * O(t) and not (O(t - 1) > 0 and 5040 * Q6[t - 1] <= 0.1 * O(t - 1)) or t == 1
    assert T[2, 9] <= 2047                                                    # 3 cells far in the tail: the first x whose tail holds them all
    en = ld.enriched(np.array([ld.TESTED, ld.TESTED, ld.OVER]), np.array([[0, 6, 0, 0], [0, 6, 0, 0], [0, 6, 0, 0]]), np.array([t, t - 1, 4000]), np.where(T == 2048, 0, T))
    assert en.tolist() == [True, False, False]


def test_clustering():
    b1 = np.array([10, 11, 12, 20, 38, 40])
    b2 = np.array([30, 31, 33, 50, 60, 62])
    cnt = np.array([5, 9, 9, 4, 7, 7])
    r = np.arange(24, dtype=np.float64).reshape(6, 4)
    got = ld.loops(b1, b2, cnt, [0, 39], np.ones(6, dtype=bool), np.full(6, 5), r, cluster_radius=2)
    # 0-1-2 chain; 3 alone; 4 and 5 are close but in different chromosomes (bin 38 | bin 40)
    assert [(L.cell, L.n_cells, L.box) for L in got] == [(1, 3, (10, 12, 30, 33)), (3, 1, (20, 20, 50, 50)), (4, 1, (38, 38, 60, 60)), (5, 1, (40, 40, 62, 62))]
    assert got[0].count == 9 and got[0].r == (4.0, 5.0, 6.0, 7.0)


def test_binding_lists_the_entry_points():
    from microcket_amd import capi
    for name in ("mkt_loops_opts_default", "mkt_matrix_loops", "mkt_matrix_fetch_loop_cells", "mkt_matrix_fetch_loop_hist", "mkt_matrix_fetch_loop_thresholds",
                 "mkt_matrix_fetch_loops", "mkt_matrix_loops_timing"):
        assert name in capi.EXPORTS
    assert [f for f, _ in capi.LoopsOpts._fields_] == ["peak", "window", "window_max", "min_ll_count", "min_dist", "max_dist", "fdr", "cluster_radius", "reserved"]
