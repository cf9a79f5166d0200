"""Expected tables and observed / expected values (mkt_matrix_expected, pairs2matrix --expected): what can be checked without a GPU.
The definition restated in tests/expecteddef.py against hand-computed literals, the smoothing edges, the executable's argument
handling, the ABI names."""
import ctypes
import math
import os
import subprocess

import numpy as np

import expecteddef as ed
import matrixdef as md
import microcket_amd as m
import util

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
NAN = float("nan")
# two chromosomes of 3 and 2 bins, 6 cells
B1, B2, CNT = [0, 0, 0, 2, 2, 3], [0, 1, 2, 2, 4, 4], [4, 3, 2, 1, 7, 6]


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


def test_definition_by_hand_with_a_masked_bin_and_a_masked_chromosome():
    # bin 1 is masked and so is all of the second chromosome: valid = T F T | F F
    r = ed.expected(B1, B2, CNT, 5, [0, 3], weights=[0.5, NAN, 2.0, NAN, NAN])
    assert r.balanced.tolist()[0] == 1.0 and _same(r.balanced, [1.0, NAN, 2.0, 4.0, NAN, NAN])     # 4 * .5 * .5, 2 * .5 * 2, 1 * 2 * 2
    assert r.used.tolist() == [True, False, True, True, False, False]
    assert r.seg.tolist() == [0, 1, 2, 0, 5, 4]                           # the trans cell: nbins + row 0; (3, 4): second chromosome, diagonal 1
    assert r.cis.n_valid.tolist() == [2, 0, 1, 0, 0]                      # the second chromosome: n_valid 0 on every diagonal
    assert r.cis.count_sum.tolist() == [5, 0, 2, 0, 0] and r.cis.balanced_sum.tolist() == [5.0, 0.0, 2.0, 0.0, 0.0]
    assert r.trans.n_valid.tolist() == [0] and r.trans.count_sum.tolist() == [0] and r.trans.balanced_sum.tolist() == [0.0]
    assert _same(r.trans.expected, [NAN])
    assert r.genome.n_valid.tolist() == [2, 0, 1] and r.genome.count_sum.tolist() == [5, 0, 2] and r.genome.balanced_sum.tolist() == [5.0, 0.0, 2.0]
    assert _same(r.genome.expected, [2.5, NAN, 2.0]) and _same(r.genome.expected_smooth, [2.5, NAN, 2.0]) and r.smooth_groups == 3
    assert _same(r.oe, [0.4, NAN, 1.0, 1.6, NAN, NAN]) and _same(r.oe_smooth, r.oe)       # every cell of the masked chromosome is NaN
    # raw: every bin valid, weight 1
    r = ed.expected(B1, B2, CNT, 5, [0, 3])
    assert r.balanced.tolist() == [4.0, 3.0, 2.0, 1.0, 7.0, 6.0] and r.used.all()
    assert r.cis.n_valid.tolist() == [3, 2, 1, 2, 1] and r.cis.count_sum.tolist() == [5, 3, 2, 0, 6]
    assert r.trans.n_valid.tolist() == [6] and r.trans.count_sum.tolist() == [7] and r.trans.expected.tolist() == [7.0 / 6.0]
    assert r.genome.n_valid.tolist() == [5, 3, 1] and r.genome.count_sum.tolist() == [5, 9, 2] and r.genome.expected.tolist() == [1.0, 3.0, 2.0]
    assert r.oe.tolist() == [4.0, 1.0, 1.0, 1.0, 7.0 / (7.0 / 6.0), 2.0]
    # three chromosomes: the trans rows in (a, b) order; a chromosome without a bin keeps its rows
    r = ed.expected([0, 0, 1], [1, 2, 2], [1, 2, 3], 3, [0, 1, 2])
    assert r.seg.tolist() == [3, 4, 5] and r.trans.count_sum.tolist() == [1, 2, 3] and r.trans.n_valid.tolist() == [1, 1, 1]
    # nothing at all
    r = ed.expected([], [], [], 4, [0, 3])
    assert r.cis.n_valid.tolist() == [3, 2, 1, 1] and not r.cis.count_sum.any() and r.genome.expected.tolist() == [0.0, 0.0, 0.0]


def test_smoothing_edges_and_groups():
    want = list(range(0, 17)) + [18, 20, 22, 24, 27, 30, 33, 37]
    got = ed.smooth_edges(40)
    assert got[:len(want)] == want and got[-1] == 40 and got[len(want)] == 40
    assert ed.smooth_edges(1) == [0, 1] and ed.smooth_edges(2) == [0, 1, 2] and ed.smooth_edges(17) == list(range(18)) and ed.smooth_edges(0) == [0]
    e = ed.smooth_edges(100000)
    assert all(b - a == max(1, a >> 3) for a, b in zip(e[1:-2], e[2:-1]))
    # one chromosome of 20 bins, raw: diagonals 16 and 17 share a group, 18 and 19 the next one
    r = ed.expected([0, 1, 0], [16, 18, 19], [3, 5, 2], 20, [0])
    assert r.genome.n_valid[16:].tolist() == [4, 3, 2, 1] and r.genome.balanced_sum[16:].tolist() == [3.0, 5.0, 0.0, 2.0]
    assert r.genome.expected_smooth[16:].tolist() == [8.0 / 7.0, 8.0 / 7.0, 2.0 / 3.0, 2.0 / 3.0] and r.genome.expected_smooth[15] == 0.0
    assert r.smooth_groups == 18                                            # diagonal 0, 1 .. 15 alone, [16, 18), [18, 20)
    assert r.oe_smooth.tolist() == [3.0 / (8.0 / 7.0), 5.0 / (8.0 / 7.0), 2.0 / (2.0 / 3.0)]


def test_observed_over_expected_sums_to_n_valid_per_diagonal():
    rng = np.random.default_rng(3)
    nb, off = 90, [0, 40, 41, 70]
    a, b = rng.integers(0, nb, 4000), rng.integers(0, nb, 4000)
    key = np.unique(np.minimum(a, b) * nb + np.maximum(a, b))
    b1, b2 = key // nb, key % nb
    cnt = rng.integers(1, 50, key.size)
    w = rng.uniform(0.2, 3.0, nb)
    w[[5, 40, 77]] = NAN
    r = ed.expected(b1, b2, cnt, nb, off, weights=w)
    chrom = np.searchsorted(off, np.arange(nb), side="right") - 1
    cis = (chrom[b1] == chrom[b2]) & r.used
    checked = 0
    for d in range(r.genome.n_valid.size):
        sel = cis & (b2 - b1 == d)
        if sel.any():
            assert abs(r.oe[sel].sum() / float(r.genome.n_valid[d]) - 1.0) <= 1e-12, d
            checked += 1
    assert checked > 20 and np.isfinite(r.oe[r.used]).all() and np.isnan(r.oe[~r.used]).all() and (~r.used).any()


def test_abi_lists_the_expected_entry_points():
    from microcket_amd import build, capi
    names = ("mkt_expected_opts_default", "mkt_matrix_expected", "mkt_matrix_fetch_expected_cis", "mkt_matrix_fetch_expected_trans", "mkt_matrix_fetch_expected_genome",
             "mkt_matrix_fetch_values", "mkt_matrix_expected_timing")
    for name in names:
        assert name in capi.EXPORTS
    assert ctypes.sizeof(capi.ExpectedOpts) == 8 and ctypes.sizeof(capi._ExpectedInfoC) == 32
    assert capi.VALUE_KINDS == {"balanced": 0, "oe": 1, "oe_smooth": 2}
    build.build_lib()
    lib = ctypes.CDLL(m.lib_path())
    for name in names:
        assert hasattr(lib, name), name
    o = capi.ExpectedOpts(use_weights=7, reserved=9)
    lib.mkt_expected_opts_default(ctypes.byref(o))                                        # needs no GPU
    assert (o.use_weights, o.reserved) == (1, 0)
    assert lib.mkt_abi_version() == 9
    hdr = open(os.path.join(util.ROOT, "include", "mkt.h")).read()
    for d, v in (("MKT_VALUE_BALANCED", 0), ("MKT_VALUE_OE", 1), ("MKT_VALUE_OE_SMOOTH", 2)):
        assert f"#define {d} {v}\n" in hdr


def test_pairs2matrix_expected_arguments(tmp_path):
    from microcket_amd import build
    build.build_lib()
    build.build_pairs2matrix()
    table = tmp_path / "g.sizes"
    table.write_bytes(md.HAND_TABLE)
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(md.HAND_PAIRS)
    out = tmp_path / "out" / "o"
    os.makedirs(out.parent)
    base = ["-g", str(table), "-r", "100", "-o", str(out), str(pairs)]
    run = lambda *a: subprocess.run([EXE, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    assert run("--expected").returncode == 2                                              # the other arguments are still needed
    r = run(*base, "--expected", "5")                                                     # it takes no value: "5" is one more input file
    assert r.returncode == 10
    assert run(*base, "--expect").returncode == 2 and run(*base, "--expected", "--tol", "1e-6").returncode == 2
    assert os.listdir(out.parent) == []
    plain = sorted(["o.100.coo", "o.100.bins.bed", "o.matrix.stat"])
    extra = ["o.100.expected.tsv", "o.100.expected.chrom.tsv", "o.100.expected.trans.tsv"]
    if m.device_count() == 0:
        for a in (["--expected"], ["--balance", "--expected"], []):
            r = run(*base, *a)
            assert r.returncode == 20 and r.stdout == b"", a                              # accepted; no GPU: loud failure ...
            assert os.listdir(out.parent) == []                                           # ... and no output files left behind
    else:
        assert run(*base).returncode == 0                                                 # without --expected: no new file
        assert sorted(os.listdir(out.parent)) == plain
        assert open(out.parent / "o.100.coo", "rb").read() == md.HAND_COO
        assert run(*base, "--expected").returncode == 0
        assert sorted(os.listdir(out.parent)) == sorted(plain + extra)
        lines = open(out.parent / "o.100.expected.tsv", "rb").read().splitlines()
        assert lines[0] == b"diag\tdist_bp\tn_valid\tcount_sum\tbalanced_sum\texpected\texpected_smooth" and len(lines) == 1 + 10
        assert lines[1] == b"0\t0\t14\t2\t2\t" + b"%.17g" % (2.0 / 14.0) + b"\t" + b"%.17g" % (2.0 / 14.0)
        assert math.isclose(float(lines[10].split(b"\t")[4]), 0.0)
