"""Pileups and aggregate peak analysis (mkt_matrix_pileup, pairs2matrix --apa / --pileup): what can be checked without a GPU.  The
definition restated in tests/piledef.py against hand-computed 3 x 3 and 5 x 5 cases and the planted-loop input, and the executable's
argument handling."""
import math
import os
import subprocess

import numpy as np
import pytest

import expected_inputs as xi
import expecteddef as ed
import loops_inputs as li
import matrixdef as md
import microcket_amd as m
import piledef as pd
import pileup_inputs as pi
import util
from microcket_amd import capi

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
NAN = float("nan")
B1, B2, CNT = (np.array(x) for x in zip(*pi.HAND))
RAW = dict(kind="balanced", flank=1, corner=1, ignore_diags=0)


def _hand(a, b, **kw):
    o = dict(RAW)
    o.update(kw)
    w = o.pop("weights", None)
    return pd.pileup(B1, B2, CNT, 6, [0], a, b, weights=w, expected=o.pop("expected", None), expected_smooth=o.pop("expected_smooth", None), **o)


def test_three_by_three_by_hand():
    # feature (1, 3): rows 0 .. 2, columns 2 .. 4 of the upper triangle; (2, 2) is not stored
    r = _hand([1], [3])
    assert r.status.tolist() == [pd.USED] and r.n.tolist() == [[1] * 3] * 3
    assert r.csum.tolist() == [[9, 0, 0], [3, 0, 0], [0, 1, 0]] and r.vsum.tolist() == [[9.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    assert r.mean.tolist() == r.vsum.tolist() and r.scores["peak"] == 0.0 and math.isnan(r.scores["p2ll"])       # LL = (2, 2) holds 0: 0 / 0
    # ignore_diags 2 drops (1, 2), (2, 2), (2, 3): an absent cell at a kept position still counts in n
    r = _hand([1], [3], ignore_diags=2)
    assert r.n.tolist() == [[1, 1, 1], [0, 1, 1], [0, 0, 1]] and r.csum.tolist() == [[9, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert np.isnan(r.mean[1][0]) and r.mean[0][0] == 9.0 and r.mean[0][1] == 0.0
    # a mirrored on-diagonal feature: (2, 1) reads the cell (1, 2), (3, 2) the cell (2, 3); the result is symmetric
    r = _hand([2], [2])
    assert r.csum.tolist() == [[4, 3, 0], [3, 0, 1], [0, 1, 7]] and r.n.tolist() == [[1] * 3] * 3
    # a masked bin: positions lose its row and its column; v = (count * w[bin1]) * w[bin2] with bin1 <= bin2 of the cell looked up
    w = np.array([1.0, 0.5, NAN, 2.0, 1.0, 1.0])
    r = _hand([1], [3], weights=w)
    assert r.n.tolist() == [[0, 1, 1], [0, 1, 1], [0, 0, 0]] and not r.csum.any()
    # a feature at the chromosome's start: EDGE with edges 0, clipped with edges 1
    r = _hand([0], [1], weights=w)
    assert r.status.tolist() == [pd.EDGE] and not r.n.any() and np.isnan(r.mean).all() and all(math.isnan(v) for v in r.scores.values())
    r = _hand([0], [1], weights=w, edges=1)
    assert r.status.tolist() == [pd.USED] and r.n.tolist() == [[0, 0, 0], [1, 1, 0], [1, 1, 0]]
    assert r.csum.tolist() == [[0, 0, 0], [5, 2, 0], [2, 4, 0]] and r.vsum.tolist() == [[0.0, 0.0, 0.0], [5.0, 1.0, 0.0], [1.0, 1.0, 0.0]]
    # two features and a divisor by distance: sums over both, one division per cell
    E = np.array([4.0, 2.0, 0.5, 1.0, 1.0, 1.0])
    r = _hand([1, 2, 2], [3, 2, 2], kind="oe", expected=E, expected_smooth=None)
    assert r.n.tolist() == [[3] * 3] * 3 and r.csum.tolist() == [[9 + 8, 6, 0], [3 + 6, 0, 2], [0, 1 + 2, 14]]
    assert r.vsum.tolist() == [[9 / 0.5 + 1.0 + 1.0, 1.5 + 1.5, 0.0], [3 / 2.0 + 1.5 + 1.5, 0.0, 0.5 + 0.5], [0.0, 1 / 2.0 + 0.5 + 0.5, 7 / 4.0 + 7 / 4.0]]
    assert r.mean[0][0] == 20.0 / 3.0
    # statuses: TRANS before DIST before EDGE; a bad feature is named
    st = pd.statuses([0, 0, 2, 5, 6], [7, 1, 3, 5, 8], [0, 6], 12, 1, 0, 1, 2)[0]     # two chromosomes of 6 bins, flank 1, min_dist 1, max_dist 2
    assert st.tolist() == [pd.TRANS, pd.EDGE, pd.USED, pd.DIST, pd.EDGE]
    assert pd.statuses([6], [8], [0, 6], 12, 1, 0, 1, 2)[0].tolist() == [pd.EDGE] and pd.statuses([7], [9], [0, 6], 12, 1, 0, 1, 2)[0].tolist() == [pd.USED]
    assert pd.statuses([7], [10], [0, 6], 12, 1, 0, 1, 2)[0].tolist() == [pd.DIST] and pd.statuses([7], [10], [0, 6], 12, 1, 0, 1, 0)[0].tolist() == [pd.USED]
    for a, b in (([3], [2]), ([3], [12])):
        with pytest.raises(ValueError, match="feature 0"):
            pd.statuses(a, b, [0, 6], 12, 1)


def test_five_by_five_scores_by_hand():
    mean = np.arange(25.0).reshape(5, 5)
    s = pd.scores(mean, 2, 2)
    # LL rows 3 .. 4, columns 0 .. 1: 15, 16, 20, 21; UL 0, 1, 5, 6; UR 3, 4, 8, 9; LR 18, 19, 23, 24; all but the centre: 288 / 24
    assert s == dict(peak=12.0, p2ll=12.0 / 18.0, p2ul=12.0 / 3.0, p2ur=12.0 / 6.0, p2lr=12.0 / 21.0, p2m=1.0, z_ll=(12.0 - 18.0) / math.sqrt(26.0 / 3.0))
    s = pd.scores(mean, 2, 1)
    assert (s["p2ll"], s["p2ul"], s["p2ur"], s["p2lr"]) == (12.0 / 20.0, math.inf, 3.0, 0.5) and math.isnan(s["z_ll"])      # one value has no deviation
    mean[4][0] = NAN                                                          # a position without a kept feature is left out of its box
    s = pd.scores(mean, 2, 2)
    mu = (15.0 + 16.0 + 21.0) / 3.0
    sd = math.sqrt(((15.0 - mu) ** 2 + (16.0 - mu) ** 2 + (21.0 - mu) ** 2) / 2.0)
    assert s["p2ll"] == 12.0 / mu and s["z_ll"] == (12.0 - mu) / sd and s["p2m"] == 12.0 / ((300.0 - 12.0 - 20.0) / 23.0)
    mean[2][2] = NAN
    assert all(math.isnan(v) for v in pd.scores(mean, 2, 2).values())
    # a 5 x 5 pileup whose centre is the one cell with contacts
    r = pd.pileup([2], [7], [4], 12, [0], [2], [7], kind="balanced", flank=2, corner=2, ignore_diags=0)
    assert r.csum[2][2] == 4 and r.csum.sum() == 4 and r.scores["peak"] == 4.0 and r.scores["p2ll"] == math.inf and r.scores["p2m"] == math.inf


def test_chunks_are_added_in_their_order():
    """three values whose sum depends on the order: 2^53, 1, 1 in one chunk is 2^53; 1, 1 in a first chunk and 2^53 in the second is 2^53 + 2"""
    big = float(2 ** 53)
    kept = np.ones((258, 1), dtype=bool)
    c = np.zeros((258, 1), dtype=np.int64)
    val = np.zeros((258, 1))
    val[0], val[1], val[2] = big, 1.0, 1.0
    assert pd.chunked(kept, c, val)[2][0] == big and pd.chunked(kept, c, val)[0][0] == 258
    val[0], val[1], val[2], val[257] = 1.0, 1.0, 0.0, big
    assert pd.chunked(kept, c, val)[2][0] == big + 2.0
    val[:] = 0.0
    val[0], val[256], val[257] = 1.0, 1.0, big                                # chunk 1 is 1 + 2^53 = 2^53, then 1 + 2^53 again; one after the other it would be 2^53 + 2
    assert pd.chunked(kept, c, val)[2][0] == big


def test_planted_loops_pile_up():
    """the condition the GPU test relies on: with the planted pixels as features the centre is the largest finite mean and stands out
    of the corner towards the diagonal"""
    text, cells, pixels = li.planted()
    off, nb = xi.offsets(250000)
    b1, b2, c = (cells[250000][:, k].astype(np.int64) for k in range(3))
    E = ed.expected(b1, b2, c, nb, off).genome
    a, b = pi.planted_features()
    assert a.size == li.STAT_PLANTS
    for kind in ("oe_smooth", "oe", "balanced"):
        r = pd.pileup(b1, b2, c, nb, off, a, b, expected=E.expected, expected_smooth=E.expected_smooth, kind=kind)
        assert (r.status == pd.USED).all() and r.n.max() == r.n[10][10] == li.STAT_PLANTS
        assert r.scores["peak"] == np.nanmax(r.mean) == r.mean[10][10] and r.scores["p2ll"] > 1 and r.scores["z_ll"] > 3, (kind, r.scores)


def test_binding_lists_the_entry_points():
    for name in ("mkt_pileup_opts_default", "mkt_matrix_pileup", "mkt_matrix_fetch_pileup", "mkt_matrix_fetch_pileup_status", "mkt_matrix_pileup_timing"):
        assert name in capi.EXPORTS
    assert [f for f, _ in m.PileupOpts._fields_] == ["flank", "corner", "kind", "ignore_diags", "edges", "min_dist", "max_dist", "reserved"]
    assert (capi.PILE_USED, capi.PILE_TRANS, capi.PILE_EDGE, capi.PILE_DIST) == (pd.USED, pd.TRANS, pd.EDGE, pd.DIST) == (1, 2, 3, 4)
    assert m.PileupInfo._fields[-7:] == pd.SCORES and m.Pileup._fields == ("n", "csum", "vsum", "mean", "status")


def test_pairs2matrix_pileup_arguments_without_gpu(tmp_path):
    from microcket_amd import build
    build.build_lib()
    build.build_pairs2matrix()
    table = tmp_path / "g.sizes"
    table.write_bytes(md.HAND_TABLE)
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(md.HAND_PAIRS)
    out = tmp_path / "out" / "o"
    os.makedirs(out.parent)
    good = tmp_path / "good.bedpe"
    good.write_bytes(b"# a comment\n\nchrB\t100\t200\tchrB\t700\t800\tx\nchrA\t0\t100\tchrB\t0\t100\n")
    run = lambda *a: subprocess.run([EXE, "-g", str(table), "-o", str(out), "-r", "100", *a, str(pairs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    for sub in (("--pile-flank", "3"), ("--pile-corner", "2"), ("--pile-kind", "oe"), ("--pile-edges",)):
        r = run(*sub)                                                         # a sub-option without --apa or --pileup
        assert r.returncode == 2 and b"needs --apa or --pileup" in r.stderr and b"Usage" in r.stderr, sub
    for sub, what in ((("--pile-kind", "raw"), b"balanced, oe or oe-smooth"), (("--pile-flank", "0"), b"1 .. 32"), (("--pile-flank", "33"), b"1 .. 32"), (("--pile-flank", "x"), b"1 .. 32"),
                      (("--pile-corner", "0"), b"at least 1"), (("--pile-flank", "3", "--pile-corner", "4"), b"--pile-corner 4 is larger than --pile-flank 3"),
                      (("--pile-corner", "11"), b"--pile-corner 11 is larger than --pile-flank 10")):
        for main in (("--apa",), ("--pileup", str(good))):
            r = run(*main, *sub)
            assert r.returncode == 12 and what in r.stderr, (main, sub, r.stderr)
    for name, text, what in (("short", b"chrB\t100\t200\tchrB\t700\n", b"line 1: six tab-separated columns"), ("unknown", b"chrB\t100\t200\tchrB\t700\t800\nchrB\t1\t2\tchrZ\t1\t2\n", b"line 2: unknown chromosome chrZ"),
                             ("past", b"chrA\t200\t300\tchrA\t200\t300\n", b"midpoint 250 is past the end of chrA (250)"), ("number", b"chrB\t1e2\t200\tchrB\t700\t800\n", b"'1e2' is not a position"),
                             ("order", b"chrB\t300\t200\tchrB\t700\t800\n", b"an end before its start")):
        f = tmp_path / (name + ".bedpe")
        f.write_bytes(text)
        r = run("--pileup", str(f))
        assert r.returncode == 12 and b"bad pileup file" in r.stderr and what in r.stderr, (name, r.stderr)
    assert run("--pileup", str(tmp_path / "missing.bedpe")).returncode == 10
    assert os.listdir(out.parent) == []                                       # refused before anything is written
    if m.device_count() == 0:
        for main in (("--apa",), ("--pileup", str(good), "--pile-flank", "2", "--pile-kind", "balanced", "--pile-edges")):
            r = run(*main)
            assert r.returncode == 20 and r.stdout == b"" and os.listdir(out.parent) == []
