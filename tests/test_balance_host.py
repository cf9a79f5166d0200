"""Matrix balancing (mkt_matrix_balance, pairs2matrix --balance): what can be checked without a GPU.
The definition restated in tests/balancedef.py against hand-computed literals, the executable's argument handling, the ABI names."""
import ctypes
import math
import os
import subprocess

import numpy as np

import balancedef as bd
import matrixdef as md
import microcket_amd as m
import util

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
F = (1, 2, 3, 6)


def _f_cells(extra=()):
    """upper-triangle cells f_i * f_j of 4 bins (diagonal included), plus extra cells"""
    cells = [(i, j, F[i] * F[j]) for i in range(4) for j in range(i, 4)] + list(extra)
    cells.sort()
    b1, b2, c = zip(*cells)
    return b1, b2, c


def test_fixed_point_of_a_rank_one_matrix():
    # off-diagonal counts f_i * f_j: weight_i = 1 / (f_i * sqrt(3)) makes every off-diagonal balanced value 1/3, every marginal 1
    b1, b2, c = _f_cells()
    r = bd.balance(b1, b2, c, 4, [0], ignore_diags=1, min_nnz=0, min_count=0, mad_max=0, tol=1e-24)
    want = np.array([1.0 / (f * math.sqrt(3.0)) for f in F])
    assert np.abs(r.weights - want).max() < 1e-10, r.weights
    assert r.masked == 0 and r.iterations == len(r.variances) and r.longest_row == 3
    bal = bd.balanced_marginals(b1, b2, c, 4, r.weights, ignore_diags=1)
    assert np.abs(bal - 1.0).max() < 1e-10
    w = r.weights
    for i in range(4):
        for j in range(i + 1, 4):
            assert abs(F[i] * F[j] * w[i] * w[j] - 1.0 / 3.0) < 1e-10
    # the first iteration by hand: m = f_i * (12 - f_i) = 11, 20, 27, 36; mean 23.5; var = 84.25 / 23.5
    assert abs(r.variances[0] - 84.25 / 23.5) < 1e-12
    one = bd.balance(b1, b2, c, 4, [0], ignore_diags=1, min_nnz=0, mad_max=0, tol=1e-24, max_iters=1)
    assert one.iterations == 1 and one.converged is False and abs(one.scale - 23.5) < 1e-12
    assert np.allclose(one.weights, np.array([23.5 / 11, 23.5 / 20, 23.5 / 27, 23.5 / 36]) / math.sqrt(23.5), rtol=1e-14, atol=0)


def test_filters_by_hand():
    # a fifth bin that touches bin 0 only, once
    b1, b2, c = _f_cells(extra=[(0, 4, 1)])
    r = bd.balance(b1, b2, c, 5, [0], ignore_diags=1, min_nnz=2, mad_max=0)                 # marg(1) = 4, 3, 3, 3, 1
    assert np.isnan(r.weights).tolist() == [False, False, False, False, True] and r.masked == 1 and r.converged
    r = bd.balance(b1, b2, c, 5, [0], ignore_diags=1, min_nnz=0, mad_max=0)
    assert r.masked == 0 and r.filter_marg.tolist() == [12.0, 20.0, 27.0, 36.0, 1.0]
    r = bd.balance(b1, b2, c, 5, [0], ignore_diags=1, min_nnz=0, min_count=2, mad_max=0)    # the marginal 1 is below 2
    assert np.isnan(r.weights).tolist() == [False, False, False, False, True]
    r = bd.balance(b1, b2, c, 5, [0], ignore_diags=1, min_nnz=0, min_count=12.5, mad_max=0)
    assert np.isnan(r.weights).tolist() == [True, False, False, False, True]
    # MAD: 12 bins, every pair 100 except the starved bin 11 (1 with everyone): marginals 1001 x 11 and 11; the median of the
    # chromosome is 1001, so the logs are 0 x 11 and log(11 / 1001); both medians are 0, cut = exp(0) = 1 and only bin 11 is below it
    cells = [(i, j, 100 if j < 11 else 1) for i in range(12) for j in range(i + 1, 12)]
    b1, b2, c = zip(*cells)
    r = bd.balance(b1, b2, c, 12, [0], ignore_diags=1, min_nnz=0)
    assert r.cut == 1.0 and r.filter_marg[:11].tolist() == [1.0] * 11 and r.filter_marg[11] == 11 / 1001
    assert np.isnan(r.weights).tolist() == [False] * 11 + [True] and r.masked == 1 and r.converged
    assert np.allclose(r.weights[:11], 1.0 / math.sqrt(1000.0), rtol=1e-12)               # 10 neighbours at 100: balanced value 1/10
    # ... per chromosome: the same bins as two chromosomes of 6; the second one holds 1001 x 5 and 11, its median is still 1001 and its starved bin still falls
    r2 = bd.balance(b1, b2, c, 12, [0, 6], ignore_diags=1, min_nnz=0)
    assert r2.cut == 1.0 and np.isnan(r2.weights).tolist() == [False] * 11 + [True]
    # ignore_diags = 0: a diagonal cell is in its bin's row and in its column
    r = bd.balance([0, 0, 1], [0, 1, 1], [5, 3, 2], 2, [0], ignore_diags=0, min_nnz=0, mad_max=0)
    assert r.filter_marg.tolist() == [13.0, 7.0] and r.longest_row == 3
    r = bd.balance([0, 0, 1], [0, 1, 1], [5, 3, 2], 2, [0], ignore_diags=1, min_nnz=0, mad_max=0)
    assert r.filter_marg.tolist() == [3.0, 3.0]
    # everything masked, and no cell at all
    b1, b2, c = _f_cells()
    for r in (bd.balance(b1, b2, c, 4, [0], ignore_diags=1, min_nnz=100), bd.balance([], [], [], 7, [0, 3])):
        assert np.isnan(r.weights).all() and r.masked == r.weights.size and r.iterations == 1 and r.converged is False
        assert math.isnan(r.scale) and math.isnan(r.var) and r.variances == []


def test_abi_lists_the_balance_entry_points():
    from microcket_amd import capi
    for name in ("mkt_balance_opts_default", "mkt_matrix_balance", "mkt_matrix_fetch_weights", "mkt_matrix_balance_timing"):
        assert name in capi.EXPORTS
    assert ctypes.sizeof(capi.BalanceOpts) == 40 and ctypes.sizeof(capi._BalanceStatsC) == 32
    assert m.BalanceStats._fields == ("iterations", "converged", "var", "scale", "masked")
    from microcket_amd import build
    build.build_lib()
    o = capi.BalanceOpts()
    lib = ctypes.CDLL(m.lib_path())
    lib.mkt_balance_opts_default(ctypes.byref(o))                                         # needs no GPU
    assert (o.ignore_diags, o.min_nnz, o.min_count, o.mad_max, o.tol, o.max_iters, o.reserved) == (2, 10, 0.0, 5.0, 1e-5, 200, 0)
    assert {k: getattr(o, k) for k in bd.DEFAULTS} == bd.DEFAULTS


def test_pairs2matrix_balance_arguments_without_gpu(tmp_path):
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
    # a sub-option without --balance, an option without its value, an unknown option: usage
    for extra in (["--tol", "1e-6"], ["--max-iters", "5"], ["--ignore-diags", "1"], ["--min-nnz", "3"], ["--min-count", "1"], ["--mad-max", "3"],
                  ["--balance", "--tol"], ["--balance", "--balanced"]):
        r = run(*base, *extra)
        assert r.returncode == 2 and b"Usage" in r.stderr, extra
    # malformed values: exit 12 before a GPU is asked for
    for extra in (["--max-iters", "0"], ["--max-iters", "-3"], ["--max-iters", "2.5"], ["--tol", "abc"], ["--tol", "-1e-5"], ["--tol", "nan"], ["--tol", ""],
                  ["--mad-max", "inf"], ["--mad-max", "0x10"], ["--tol", "1e-5x"], ["--tol", "1-5"], ["--min-count", "-1"], ["--min-nnz", "1e3"], ["--ignore-diags", "-1"], ["--ignore-diags", "99999999999"]):
        r = run(*base, "--balance", *extra)
        assert r.returncode == 12 and b"bad value" in r.stderr, extra
    # the other argument errors are what they were
    assert run("--balance").returncode == 2
    assert run("-g", str(table), "-r", "100", "--balance").returncode == 2
    assert run("-g", str(table), "-r", "0", "-o", str(out), "--balance", str(pairs)).returncode == 12
    assert run("-g", str(tmp_path / "missing"), "-r", "100", "-o", str(out), "--balance", str(pairs)).returncode == 10
    assert os.listdir(out.parent) == []
    if m.device_count() == 0:
        r = run(*base, "--balance", "--tol", "1e-6", "--max-iters", "50", "--ignore-diags", "1", "--min-nnz", "0", "--min-count", "0", "--mad-max", "0")
        assert r.returncode == 20 and r.stdout == b""                                   # accepted; no GPU: loud failure ...
        assert os.listdir(out.parent) == []                                             # ... and no output files left behind
