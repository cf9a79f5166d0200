"""Saddle tables and compartment strength (mkt_matrix_saddle, pairs2matrix --saddle): what can be checked without a GPU.  The definition
restated in tests/saddledef.py against hand-computed groups, brute-force positions, an order that changes the bits and a hand-written
4 x 4 table, and the executable's argument handling."""
import math
import os
import subprocess

import numpy as np
import pytest

import eigs_inputs as gi
import expecteddef as ed
import matrixdef as md
import microcket_amd as m
import saddle_inputs as si
import saddledef as sd
import util
from microcket_amd import capi

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
NAN, INF = float("nan"), float("inf")


def _same(x, want):
    return np.asarray(x, dtype=np.float64).tobytes() == np.asarray(want, dtype=np.float64).tobytes()


def test_groups_by_hand():
    t = np.array([3.0, 1.0, 1.0, NAN, -0.0, 0.0, INF, -INF])
    ok = np.ones(8, dtype=bool)
    # ascending: -inf (7), -0.0 (4), 0.0 (5) a tie kept in bin order, 1.0 (1), 1.0 (2) likewise, 3.0 (0), inf (6); g = r * 2 // 7
    g, bins, lo, hi, T, K = sd.groups(t, ok, 2, 0, 0)
    assert g.tolist() == [1, 0, 1, 255, 0, 0, 1, 0] and bins.tolist() == [4, 3] and (T, K) == (7, 7)
    assert _same(lo, [-INF, 1.0]) and _same(hi, [1.0, INF])
    for zeros in ((-0.0, 0.0), (0.0, -0.0)):                                  # -0.0 == 0.0: the lower bin comes first either way
        t[4], t[5] = zeros
        g = sd.groups(t, ok, 7, 0, 0)[0]
        assert g.tolist() == [5, 3, 4, 255, 1, 2, 6, 0]
    g, bins, lo, hi, T, K = sd.groups(t, ok, 7, 0, 0)
    assert _same(lo, [-INF, 0.0, -0.0, 1.0, 1.0, 3.0, INF]) and _same(hi, lo)   # the values themselves, signs of zero included
    # a masked bin is no candidate
    ok[7] = False
    g, bins, _, _, T, K = sd.groups(t, ok, 2, 0, 0)
    assert g.tolist() == [1, 0, 1, 255, 0, 0, 1, 255] and (T, K) == (6, 6) and bins.tolist() == [3, 3]
    # K < Q: g = r * 5 // 3 = 0, 1, 3; the groups 2 and 4 are empty
    g, bins, lo, hi, T, K = sd.groups(np.array([NAN, 2.0, NAN, 1.0, 3.0]), np.ones(5, dtype=bool), 5, 0, 0)
    assert g.tolist() == [255, 1, 255, 0, 3] and bins.tolist() == [1, 1, 0, 1, 0] and np.isnan(lo[[2, 4]]).all() and np.isnan(hi[[2, 4]]).all() and (T, K) == (3, 3)
    # K == 0
    g, bins, lo, hi, T, K = sd.groups(np.full(4, NAN), np.ones(4, dtype=bool), 3, 250, 250)
    assert g.tolist() == [255] * 4 and not bins.any() and np.isnan(lo).all() and (T, K) == (0, 0)
    # trims in basis points, integer division: 40 candidates lose 1 + 1 at 250, 19 + 19 at 4999
    t = np.arange(40.0)[::-1].copy()
    for (tl, th), (lo_, K_) in (((0, 0), (0, 40)), ((250, 250), (1, 38)), ((4999, 4999), (19, 2)), ((4999, 0), (19, 21)), ((0, 250), (0, 39))):
        g, bins, lo, hi, T, K = sd.groups(t, np.ones(40, dtype=bool), 2, tl, th)
        assert (T, K) == (40, K_) and int((g != 255).sum()) == K_
        kept = np.flatnonzero(g != 255)
        assert t[kept].min() == lo_ and t[kept].max() == lo_ + K_ - 1 and lo[0] == lo_ and hi[1] == lo_ + K_ - 1
        assert (g[t < lo_] == 255).all() and bins.tolist() == [(K_ + 1) // 2, K_ // 2]


@pytest.mark.parametrize("Q", [3, 5])
def test_positions_against_the_double_loop(Q):
    off, nb = [0, 1, 3, 15], 55                                               # chromosomes of 1, 2, 12 and 40 bins
    rng = np.random.default_rng(Q)
    g = rng.integers(0, Q, nb).astype(np.uint8)
    g[[0, 3, 14, 15, 30, 54]] = sd.NONE                                       # masked: the one-bin chromosome, firsts, lasts and an interior bin
    full = rng.integers(0, Q, nb).astype(np.uint8)
    seen = 0
    for groups in (g, full):
        for mn in (0, 1, 2):
            for mx in (0, 1, 11, 39, 60):
                if mx and mx < mn:
                    continue
                want = si.brute_positions(groups, off, nb, Q, "cis", mn, mx)
                got = sd.positions(groups, off, nb, Q, "cis", mn, mx)
                assert got.dtype == np.uint64 and np.array_equal(got, want), (mn, mx)
                seen += int(want.sum() > 0)
        want = si.brute_positions(groups, off, nb, Q, "trans", 0, 0)
        assert np.array_equal(sd.positions(groups, off, nb, Q, "trans", 2, 5), want) and want.sum() > 400
    assert seen == 2 * 14
    assert int(si.brute_positions(full, off, nb, Q, "cis", 0, 0).sum()) == 1 + 3 + 78 + 820
    assert int(si.brute_positions(full, off, nb, Q, "trans", 0, 0).sum()) == 55 * 54 // 2 - (1 + 66 + 780)


def test_the_order_of_step_3_bites():
    big = float(2 ** 53)
    n = 2 * sd.CHUNK + 2
    used, a, b = np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    x = np.zeros(n)
    x[0], x[1], x[2] = big, 1.0, 1.0                                          # one chunk, one after the other: 2^53 swallows each 1
    assert sd.chunked(used, a, b, x, 2)[0][1] == big
    x[:] = 0.0
    x[0], x[1], x[sd.CHUNK] = 1.0, 1.0, big                                   # 2 first, then the chunk that holds 2^53
    assert sd.chunked(used, a, b, x, 2)[0][1] == big + 2.0
    x[:] = 0.0
    x[0], x[sd.CHUNK], x[sd.CHUNK + 1] = 1.0, big, 1.0                        # T_1 = 2^53 + 1 = 2^53, then 1 + 2^53: in cell order it would be 2^53 + 2
    assert sd.chunked(used, a, b, x, 2)[0][1] == big
    # unused cells keep their slots: taking them out moves a value into another chunk
    x[:] = 0.0
    x[sd.CHUNK], x[sd.CHUNK + 1], x[sd.CHUNK + 2] = big, 1.0, 1.0             # 2^53 leads chunk 1 and swallows both
    assert sd.chunked(used, a, b, x, 2)[0][1] == big
    hole = used.copy()
    hole[5] = False
    assert sd.chunked(hole, a, b, x, 2)[0][1] == big                          # ... with the hole in place nothing moves
    assert sd.chunked(np.delete(used, 5), a[1:], b[1:], np.delete(x, 5), 2)[0][1] == big + 2.0
    # ordinary values: the chunked sum is the plain loop in this order, and not the bits of np.sum
    x = np.random.default_rng(9).random(n) * 3.0
    T = [0.0, 0.0, 0.0]
    for k in range(n):
        T[k // sd.CHUNK] += float(x[k])
    want = (0.0 + T[0] + T[1]) + T[2]
    got = float(sd.chunked(used, a, b, x, 2)[0][1])
    assert got == want and got != float(np.sum(x)) and abs(got - float(np.sum(x))) < 1e-9 * got
    seq = 0.0
    for k in range(n):
        seq += float(x[k])
    assert got != seq                                                         # ... nor one long chain


def test_scores_on_a_four_by_four_table():
    vs = np.array([[8.0, 2.0, 1.0, 1.0], [0, 6.0, 2.0, 1.0], [0, 0, 6.0, 3.0], [0, 0, 0, 12.0]])
    n = np.array([[2, 2, 2, 1], [0, 2, 2, 2], [0, 0, 2, 2], [0, 0, 0, 2]], dtype=np.uint64)
    st, aa, bb = sd.scores(vs, n, 4)
    # k = 1: BB = (0, 0), AA = (3, 3), AB = (0, 3); k = 2: BB = (0,0) (0,1) (1,1), AA = (2,2) (2,3) (3,3), AB = (0,2) (0,3) (1,2) (1,3)
    ab2 = 5.0 / 7.0
    assert st.tolist() == [((8.0 + 12.0) / 4.0) / 1.0, ((16.0 + 21.0) / 12.0) / ab2]
    assert aa.tolist() == [6.0, (21.0 / 6.0) / ab2] and bb.tolist() == [4.0, (16.0 / 6.0) / ab2]
    sym = lambda u: np.triu(u) + np.triu(u, 1).T                             # the symmetric tables give the same: only a <= b is read
    assert all(_same(x, y) for x, y in zip(sd.scores(sym(vs), sym(n), 4), (st, aa, bb)))
    # zero denominators: no AB position; an AB mean of zero; no BB position
    n0, v0 = n.copy(), vs.copy()
    n0[0][3], v0[0][3] = 0, 0.0
    st, aa, bb = sd.scores(v0, n0, 4)
    assert math.isnan(st[0]) and math.isnan(aa[0]) and math.isnan(bb[0]) and st[1] == ((16.0 + 21.0) / 12.0) / (4.0 / 6.0)
    v0 = vs.copy()
    v0[0][3] = 0.0
    st, aa, bb = sd.scores(v0, n, 4)
    assert math.isnan(st[0]) and math.isnan(aa[0]) and math.isnan(bb[0]) and not math.isnan(st[1])
    n0 = n.copy()
    n0[0][0] = 0
    st, aa, bb = sd.scores(vs, n0, 4)
    assert math.isnan(bb[0]) and aa[0] == 6.0 and st[0] == ((8.0 + 12.0) / 2.0) / 1.0
    assert all(_same(x, [NAN]) for x in sd.scores(np.zeros((2, 2)), np.zeros((2, 2), dtype=np.uint64), 2))      # the one quiet NaN
    assert sd.corner_of(50, 0) == 10 and sd.corner_of(4, 0) == 1 and sd.corner_of(64, 7) == 7


def test_flat_and_planted_matrices():
    """the conditions the GPU test relies on: a dense chromosome of equal counts has mean 1.0 exactly wherever there is a position, and
    the planted compartments give AA and BB above AB at every corner size"""
    ttext, text, off, nb, cells, track = si.flat()
    b1, b2, c = (cells[:, k].astype(np.int64) for k in range(3))
    E = ed.expected(b1, b2, c, nb, off).genome
    for Q, mn in ((2, 0), (5, 2), (7, 1)):
        r = sd.saddle(b1, b2, c, nb, off, track, expected=E.expected, expected_smooth=E.expected_smooth, n_groups=Q, trim_lo=0, trim_hi=0, min_diag=mn)
        assert np.array_equal(r.n, r.nnz) and (r.n > 0).sum() >= Q * Q - 2 and (r.mean[r.n > 0] == 1.0).all() and np.isnan(r.mean[r.n == 0]).all()
        assert all((x[~np.isnan(x)] == 1.0).all() for x in (r.strength, r.aa_ab, r.bb_ab)) and r.info["strength"] == 1.0
        assert r.info["cells_used"] == int(np.triu(r.nnz.astype(np.int64)).sum()) == int((b2 - b1 >= mn).sum())
    ttext, text, off, nb, cells, track = gi.planted()
    b1, b2, c = (cells[:, k].astype(np.int64) for k in range(3))
    E = ed.expected(b1, b2, c, nb, off).genome
    for Q in (4, 5):
        r = sd.saddle(b1, b2, c, nb, off, track, expected=E.expected, expected_smooth=E.expected_smooth, n_groups=Q, trim_lo=0, trim_hi=0)
        assert r.info["kept"] == nb - 6 - 2 and (r.aa_ab > 1).all() and (r.bb_ab > 1).all() and (r.strength > 1).all(), (Q, r.strength)


def test_binding_lists_the_entry_points():
    for name in ("mkt_saddle_opts_default", "mkt_matrix_saddle", "mkt_matrix_fetch_saddle", "mkt_matrix_fetch_saddle_groups", "mkt_matrix_fetch_saddle_edges",
                 "mkt_matrix_fetch_saddle_profile", "mkt_matrix_saddle_timing"):
        assert name in capi.EXPORTS
    assert [f for f, _ in m.SaddleOpts._fields_] == ["n_groups", "trim_lo", "trim_hi", "contact", "kind", "min_diag", "max_diag", "corner", "reserved"]
    assert m.Saddle._fields == sd.FIELDS and m.SaddleInfo._fields[-3:] == sd.SCORES and capi.SADDLE_NONE == sd.NONE == 255
    o = m.SaddleOpts()
    capi.load_library().mkt_saddle_opts_default(o)
    assert [getattr(o, f) for f, _ in m.SaddleOpts._fields_] == [50, 250, 250, 0, 1, 2, 0, 0, 0]
    assert [sd.DEFAULTS[k] for k in ("n_groups", "trim_lo", "trim_hi", "min_diag", "max_diag", "corner")] == [50, 250, 250, 2, 0, 0]


def test_pairs2matrix_saddle_arguments_without_gpu(tmp_path):
    from microcket_amd import build
    build.build_lib()
    build.build_pairs2matrix()
    table = tmp_path / "g.sizes"
    table.write_bytes(md.HAND_TABLE)
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(md.HAND_PAIRS)
    out = tmp_path / "out" / "o"
    os.makedirs(out.parent)
    run = lambda *a: subprocess.run([EXE, "-g", str(table), "-o", str(out), "-r", "100,50", *a, str(pairs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    for sub in (("--saddle-groups", "5"), ("--saddle-trim", "0,0"), ("--saddle-contact", "trans"), ("--saddle-kind", "oe"), ("--saddle-min-dist", "100"), ("--saddle-max-dist", "200"),
                ("--saddle-corner", "1")):
        r = run(*sub)                                                         # a sub-option without --saddle
        assert r.returncode == 2 and b"needs --saddle" in r.stderr and b"Usage" in r.stderr, sub
    for sub, what in ((("--saddle-groups", "1"), b"2 .. 64"), (("--saddle-groups", "65"), b"2 .. 64"), (("--saddle-groups", "x"), b"2 .. 64"),
                      (("--saddle-trim", "250"), b"LO,HI"), (("--saddle-trim", "5000,5000"), b"below 10000 together"), (("--saddle-trim", "-1,0"), b"LO,HI"),
                      (("--saddle-trim", "1,x"), b"LO,HI"), (("--saddle-contact", "both"), b"cis or trans"), (("--saddle-kind", "balanced"), b"oe or oe-smooth"),
                      (("--saddle-min-dist", "-100"), b"base pairs"), (("--saddle-max-dist", "1e3"), b"base pairs"), (("--saddle-corner", "0"), b"at least 1"),
                      (("--saddle-groups", "6", "--saddle-corner", "4"), b"--saddle-corner 4 is larger than half of --saddle-groups 6"),
                      (("--saddle-corner", "26"), b"--saddle-corner 26 is larger than half of --saddle-groups 50"),
                      (("--saddle-min-dist", "300", "--saddle-max-dist", "200"), b"--saddle-max-dist 200 is below --saddle-min-dist 300"),
                      (("--saddle-min-dist", "150"), b"--saddle-min-dist 150 is not a multiple of resolution 100"),
                      (("--saddle-max-dist", "225"), b"--saddle-max-dist 225 is not a multiple of resolution")):
        r = run("--saddle", *sub)
        assert r.returncode == 12 and what in r.stderr, (sub, r.stderr)
    assert os.listdir(out.parent) == []                                       # refused before anything is written
    if m.device_count() == 0:
        r = run("--saddle", "--saddle-groups", "4", "--saddle-trim", "0,0", "--saddle-min-dist", "100", "--saddle-max-dist", "0", "--saddle-corner", "2")
        assert r.returncode == 20 and r.stdout == b"" and os.listdir(out.parent) == []
