"""Insulation scores and boundaries (mkt_matrix_insulation, pairs2matrix --insulation): what can be checked without a GPU.  The
definition restated in tests/insuldef.py against hand-computed cases and a planted block-diagonal input, and the executable's
argument handling."""
import math
import os
import subprocess

import numpy as np

import balancedef as bd
import insuldef as idf
import insulation_inputs as ii
import matrixdef as md
import microcket_amd as m
import util

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
NAN = float("nan")


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


# one chromosome of 6 bins
HAND = [(0, 0, 5), (0, 1, 2), (0, 2, 9), (1, 1, 4), (1, 2, 3), (2, 3, 1), (3, 3, 7), (3, 4, 2), (4, 5, 6)]


def test_sums_and_scores_by_hand():
    b1, b2, c = zip(*HAND)
    # window 2, ignore_diags 0: rows i - 1, i and columns i, i + 1
    S = idf.sums(b1, b2, c, 6, [0], [2], None, 0)
    assert S.n_valid[0].tolist() == [2, 4, 4, 4, 4, 2]
    assert S.csum[0].tolist() == [5 + 2, 2 + 9 + 4 + 3, 3 + 0 + 0 + 1, 1 + 0 + 7 + 2, 2 + 0 + 0 + 6, 6 + 0]
    assert S.bsum[0].tolist() == [7.0, 18.0, 4.0, 10.0, 8.0, 6.0] and S.stored[0].tolist() == [2, 4, 2, 3, 2, 1]
    assert idf.n_full(2, 0) == 4
    assert _same(idf.score(S.n_valid, S.bsum, [2], 0, 0.66)[0], [NAN, 4.5, 1.0, 2.5, 2.0, NAN])      # 2 of 4 positions < 0.66 x 4
    assert _same(idf.score(S.n_valid, S.bsum, [2], 0, 0.0)[0], [3.5, 4.5, 1.0, 2.5, 2.0, 3.0])
    assert _same(idf.score(S.n_valid, S.bsum, [2], 0, 0.5)[0], [3.5, 4.5, 1.0, 2.5, 2.0, 3.0])       # 2 >= 0.5 x 4
    # windows 1 and 2 with ignore_diags 2: window 1 has no position at all, window 2 only (i - 1, i + 1)
    assert idf.n_full(1, 2) == 0 and idf.n_full(2, 2) == 1 and idf.n_full(5, 2) == 22 and idf.n_full(3, 7) == 0
    S = idf.sums(b1, b2, c, 6, [0], [1, 2], None, 2)
    assert S.n_valid.tolist() == [[0] * 6, [0, 1, 1, 1, 1, 0]] and S.csum.tolist() == [[0] * 6, [0, 9, 0, 0, 0, 0]]
    sc = idf.score(S.n_valid, S.bsum, [1, 2], 2, 0.66)
    assert _same(sc, [[NAN] * 6, [NAN, 9.0, 0.0, 0.0, 0.0, NAN]])
    L = idf.normalise(sc[1], [0], 6)
    assert _same(L, [NAN, 0.0, NAN, NAN, NAN, NAN])                           # a score of 0 has no logarithm; the mean is 9
    assert _same(idf.normalise(sc[0], [0], 6), [NAN] * 6)                     # no score in the chromosome
    # a masked bin: positions lose its row and its column (bin 2 itself keeps (1, 3)); v = (count * w[bin1]) * w[bin2]
    w = np.array([1.0, 0.5, NAN, 2.0, 1.0, 1.0])
    S = idf.sums(b1, b2, c, 6, [0], [2], w, 0)
    assert S.n_valid[0].tolist() == [2, 2, 1, 2, 4, 2] and S.csum[0].tolist() == [7, 2 + 4, 0, 7 + 2, 2 + 6, 6]
    assert S.bsum[0].tolist() == [5.0 + 2 * 0.5, 2 * 0.5 + 4 * 0.25, 0.0, 7 * 4.0 + 2 * 2.0, 2 * 2.0 + 6.0, 6.0]
    assert _same(idf.score(S.n_valid, S.bsum, [2], 0, 0.5)[0], [3.0, 1.0, NAN, 16.0, 2.5, 3.0])
    # a chromosome of one bin, then one of five: the lone bin has the position (0, 0) with ignore_diags 0 and none with 2
    S = idf.sums([0, 1, 1], [0, 1, 3], [3, 1, 2], 6, [0, 1], [2], None, 0)
    assert S.n_valid[0].tolist() == [1, 2, 4, 4, 4, 2] and S.csum[0].tolist() == [3, 1, 2, 0, 0, 0]     # no diamond reaches across the ranges
    S = idf.sums([0, 1, 1], [0, 1, 3], [3, 1, 2], 6, [0, 1], [2], None, 2)
    assert S.n_valid[0].tolist() == [0, 0, 1, 1, 1, 0] and S.csum[0].tolist() == [0, 0, 2, 0, 0, 0]
    r = idf.insulation([0, 1, 1], [0, 1, 3], [3, 1, 2], 6, [0, 1], [2], ignore_diags=0, min_frac_valid=0.0)
    assert _same(r.log2_score[0][:1], [0.0]) and not r.minima.any()           # its own mean; a segment of one bin has no minimum


def test_minima_and_strengths_by_hand():
    # 8 bins, mean 4: a plateau minimum, two plain ones
    sc = np.array([4.0, 1.0, 1.0, 4.0, 2.0, 8.0, 4.0, 8.0])
    L = idf.normalise(sc, [0], 8)
    assert L.tolist() == [0.0, -2.0, -2.0, 0.0, -1.0, 1.0, 0.0, 1.0]
    st, bnd, mn = idf.call(L, [0], 8, 1.5)
    assert np.flatnonzero(mn).tolist() == [1, 4, 6]                           # the plateau [1, 2] is reported at 1
    assert _same(st, [NAN, 2.0, NAN, NAN, 1.0, NAN, 1.0, NAN])               # min(0, 1) + 2; min(0, 1) + 1; min(1, 1) - 0
    assert bnd.tolist() == [False, True] + [False] * 6
    assert idf.call(L, [0], 8, 1.0)[1].tolist() == [False, True, False, False, True, False, True, False]      # strength >= min_strength
    # the same track as two chromosomes of 4 bins: bin 4 has lost its left neighbour
    st, bnd, mn = idf.call(L, [0, 4], 8, 0.2)
    assert np.flatnonzero(mn).tolist() == [1, 6] and _same(st[[1, 6]], [2.0, 1.0])
    # next to a gap: bins 1 and 3 are lower than their one neighbour, but the other one is not in the segment
    L = np.array([1.0, -1.0, NAN, -1.0, 1.0, 0.0, 1.0])
    st, bnd, mn = idf.call(L, [0], 7, 0.2)
    assert np.flatnonzero(mn).tolist() == [5] and st[5] == 1.0 and bnd[5]     # the walk left stops at bin 3 (-1 < 0)
    # a plateau at the end of a segment, a monotone track and a flat one have no minimum
    for L in ([1.0, 0.0, 0.0], [3.0, 2.0, 1.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0]):
        assert not idf.call(np.array(L), [0], len(L), 0.0)[2].any()
    # NaN, 0 and a chromosome without a positive score
    assert _same(idf.normalise(np.array([4.0, 0.0, NAN, 4.0, 0.0, NAN]), [0, 4], 6), [0.0, NAN, NAN, 0.0, NAN, NAN])
    assert math.isnan(idf.normalise(np.array([0.0]), [0], 1)[0])


def test_planted_domains_are_found():
    ttext, text, off, nb, cells, edges = ii.planted()
    assert nb == sum(map(sum, ii.DOMAINS)) and len(edges) == sum(len(d) - 1 for d in ii.DOMAINS) == 8
    b1, b2, c = (cells[:, k].astype(np.int64) for k in range(3))
    r = idf.insulation(b1, b2, c, nb, off, [5])
    assert r.boundary[0].sum() >= len(edges) and ii.boundaries_are_the_planted(r.boundary[0], edges), np.flatnonzero(r.boundary[0]).tolist()
    assert np.isnan(r.score[0][[0, 2, off[1] - 3, off[1] - 1, off[1], nb - 1]]).all() and not np.isnan(r.score[0][3:off[1] - 3]).any()     # 12 of 22 positions three bins from an end, 17 four bins from it
    # and from balanced values: the weights of the balancing definition with no bin masked
    w = bd.balance(b1, b2, c, nb, off, min_nnz=1, mad_max=0).weights
    assert not np.isnan(w).any()
    rw = idf.insulation(b1, b2, c, nb, off, [5], weights=w)
    assert ii.boundaries_are_the_planted(rw.boundary[0], edges), np.flatnonzero(rw.boundary[0]).tolist()


def test_pairs2matrix_insulation_arguments_without_gpu(tmp_path):
    from microcket_amd import build
    build.build_lib()
    build.build_pairs2matrix()
    table = tmp_path / "g.sizes"
    table.write_bytes(md.HAND_TABLE)
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(md.HAND_PAIRS)
    out = tmp_path / "out" / "o"
    os.makedirs(out.parent)
    run = lambda *a: subprocess.run([EXE, "-g", str(table), "-o", str(out), *a, str(pairs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    for sub in (("--ins-ignore-diags", "1"), ("--ins-min-frac-valid", "0.5"), ("--ins-min-strength", "0.1")):
        r = run("-r", "100", *sub)                                            # a sub-option without --insulation
        assert r.returncode == 2 and b"needs --insulation" in r.stderr and b"Usage" in r.stderr, sub
    for rl, wl in (("100", "250"), ("100,30", "200"), ("100", "200,250"), ("100", "0"), ("100", "abc"), ("100", "200,"), ("100", "200,200"), ("100", "300,200"),
                   ("100", "100,200,300,400,500"), ("100", "-200"), ("100", "102500"), ("100", "2e2")):
        r = run("-r", rl, "--insulation", wl)
        assert r.returncode == 12, (rl, wl, r.stderr)
    for sub in (("--ins-ignore-diags", "-1"), ("--ins-ignore-diags", "x"), ("--ins-min-frac-valid", "1.5"), ("--ins-min-frac-valid", "nan"), ("--ins-min-strength", "-0.1")):
        assert run("-r", "100", "--insulation", "200", *sub).returncode == 12, sub
    assert os.listdir(out.parent) == []                                       # refused before anything is written
    if m.device_count() == 0:
        r = run("-r", "100,50", "--insulation", "200,500,51200", "--ins-ignore-diags", "3", "--ins-min-frac-valid", "0.5", "--ins-min-strength", "0.1")
        assert r.returncode == 20 and r.stdout == b"" and os.listdir(out.parent) == []
