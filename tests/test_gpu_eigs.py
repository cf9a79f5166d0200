"""Compartment eigenvectors on the GPU (mkt_matrix_eigs, Matrix.eigs / eigs_apply) against the definition restated in tests/eigsdef.py,
fed the GPU's own cells, weights and expected table.  The product A x of the sweep kernel is checked per entry against
(T_i + 2 ignore_diags + 3) 2^-52 (|A| |x|)_i (the reordering bound of the sums plus the three operations behind oe) with an identical
zero pattern; the eigenpairs through their residual, the eigenvalue within the residual, the angle by Davis-Kahan, the norm, the NaN
pattern and the orientation.  Parity with cooltools and juicer_tools is unpinned (neither is run)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import eigs_inputs as gi
import eigsdef as gd
import loops_inputs as li
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu
U = 2.0 ** -52


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")


def _loaded(text, res, table):
    mx = m.Matrix(table, list(res), device=0)
    mx.add(text)
    mx.run()
    return mx


def _chroms(mx, k, nb, off, use_weights, **opts):
    """the definition's dense matrices from the GPU's own cells, weights and expected table (which this computes)"""
    b1, b2, c = mx.cells(k)
    w = mx.weights(k) if use_weights else None
    E = mx.expected(k, use_weights=use_weights).genome.expected_smooth
    return gd.chromosomes(b1, b2, c, nb, off, E, weights=w, **opts)


def _check_apply(label, mx, chs, nb, x, **opts):
    ig = gd.options(**opts)["ignore_diags"]
    got = mx.eigs_apply(0, x, **opts)
    want = gd.apply(chs, nb, x, ignore_diags=ig)
    bound = gd.apply_bound(chs, nb, x, ignore_diags=ig)
    dev = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.nanmax(np.where(bound > 0, dev / bound, 0.0)) if dev.size else 0.0
    print(f"{label}: max |dev| {dev.max():.3e}, worst dev / bound {worst:.3f}")
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(got == 0, want == 0), label
    assert (dev <= bound).all(), (label, float(worst))


# ---- apply, the hot kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_apply_on_the_edge_table(masked):
    _need_gpu()
    ttext, text, off, nb, cells, empty = li.edge_matrix(masked)
    if not masked:
        assert 2 * len(cells) // nb >= 48                                    # the 64-lane width (the masked table gives 32 lanes)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((nb, 8))
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        for use_weights in (False, True):
            if use_weights:
                mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
                assert set(np.flatnonzero(np.isnan(mx.weights(0))).tolist()) == empty
            for ig in (0, 1, 2, 3):
                for clip in (0.0, 1.3):
                    chs = _chroms(mx, 0, nb, off, use_weights, ignore_diags=ig, clip=clip)
                    assert [c.skipped for c in chs] == [True, False, False, False, False]       # 1 bin; 12, 64, 65 and 41 bins
                    if masked:                                                # the first and the last bin of a chromosome are not good
                        assert not chs[2].good[[0, 63]].any() and not chs[3].good[[0, 63, 64]].any()
                    _check_apply(f"edge masked={masked} w={use_weights} ig={ig} clip={clip}", mx, chs, nb, x, ignore_diags=ig, clip=clip)
            chs = _chroms(mx, 0, nb, off, use_weights)
            _check_apply(f"edge masked={masked} w={use_weights} one column", mx, chs, nb, x[:, 0])
            chs = _chroms(mx, 0, nb, off, use_weights, min_good=50)          # the 12- and the 41-bin chromosome are skipped too
            assert [c.skipped for c in chs] == [True, True, False, False, True]
            _check_apply(f"edge masked={masked} w={use_weights} min_good=50", mx, chs, nb, x[:, :3], min_good=50)


def test_apply_on_long_rows_and_chunk_sizes():
    _need_gpu()
    ttext, text, off, nb, cells = gi.shapes()
    b1, b2 = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
    per_bin = np.bincount(b1, minlength=nb) + np.bincount(b2, minlength=nb)
    assert (per_bin > 1024).sum() == 3 and 2 * len(cells) // nb < 12         # three long rows; the 8-lane width for the others
    x = np.random.default_rng(9).standard_normal((nb, 8))
    with _loaded(text, [gi.R], ttext) as mx:
        for use_weights in (False, True):
            if use_weights:
                mx.balance(0, min_nnz=1, mad_max=0)
            for ig in (0, 2, 3):
                chs = _chroms(mx, 0, nb, off, use_weights, ignore_diags=ig)
                assert not any(c.skipped for c in chs)
                _check_apply(f"shapes w={use_weights} ig={ig}", mx, chs, nb, x, ignore_diags=ig)
            _check_apply(f"shapes w={use_weights} one column", mx, _chroms(mx, 0, nb, off, use_weights), nb, x[:, 3])


# ---- eigenpairs ------------------------------------------------------------------------------------------------------------------------------
def _check_eigs(label, res, chs, nb, track, **opts):
    o = gd.options(**opts)
    ne, tol = o["n_eigs"], o["tol"]
    assert res.vectors.shape == (ne, nb) and res.lambdas.shape == (len(chs), ne)
    solved = 0
    for c, ch in enumerate(chs):
        g = ch.good
        assert res.n_good[c] == g.sum()
        if ch.skipped:                                                        # (f)
            assert np.isnan(res.vectors[:, ch.lo:ch.hi]).all() and np.isnan(res.lambdas[c]).all() and res.iterations[c] == 0 and not res.converged[c]
            continue
        solved += 1
        lam_ref, vec_ref = gd.reference_eigs(ch, ne, track)
        A = ch.A[np.ix_(g, g)]
        for j in range(ne):
            xf = res.vectors[j, ch.lo:ch.hi]
            assert np.array_equal(np.isnan(xf), ~g), (label, c, j)            # (d) NaN exactly on the other bins
            x, lam = xf[g], res.lambdas[c, j]
            assert abs(np.linalg.norm(x) - 1.0) <= (g.sum() + 2) * U, (label, c, j)
            full = np.zeros(nb)
            full[ch.lo:ch.hi][g] = x
            ab = np.linalg.norm(gd.apply_bound(chs, nb, full, ignore_diags=o["ignore_diags"]))
            rho = np.linalg.norm(A @ x - lam * x)
            print(f"{label} chrom {c} pair {j}: lambda {lam:.6f} (ref {lam_ref[j]:.6f}), rho {rho:.3e}, device resid {res.resid[c, j]:.3e}, iterations {res.iterations[c]}")
            if res.converged[c]:
                assert rho <= tol * abs(res.lambdas[c, 0]) + ab, (label, c, j, rho)           # (a)
            # (b) and (c) hold for the exact eigenpairs; numpy's are within ref_err = n_good 2^-52 |lambda_1| of them (the backward error of
            # eigh), which counts once the device's residual is that small
            ref_err = g.sum() * U * abs(lam_ref[0])
            assert abs(lam - lam_ref[j]) <= rho + ref_err, (label, c, j)      # (b)
            others = np.delete(lam_ref, j)
            gap = np.min(np.abs(others - lam))
            v = vec_ref[j][g]
            sin = np.linalg.norm(x - (x @ v) * v)
            assert sin <= (rho + ref_err) / gap, (label, c, j, sin, rho / gap)                # (c)
            want = gd.orient(xf, g, None if track is None else track[ch.lo:ch.hi])
            assert np.array_equal(want[g], x), (label, c, j)                  # (e) the orientation rule leaves it as it is
    i = res.info
    assert (i.n_chrom, i.solved, i.skipped) == (len(chs), solved, len(chs) - solved) and i.converged == int(res.converged.sum())
    assert i.max_iterations == res.iterations.max()


@pytest.mark.parametrize("balanced", [False, True])
def test_eigenpairs_of_the_planted_matrix(balanced):
    _need_gpu()
    ttext, text, off, nb, cells, track = gi.planted()
    with _loaded(text, [gi.R], ttext) as mx:
        if balanced:
            mx.balance(0)
        for opts in (dict(), dict(n_eigs=1), dict(clip=1.5), dict(n_eigs=1, clip=1.5, ignore_diags=0)):
            chs = _chroms(mx, 0, nb, off, balanced, **opts)
            for tr in (None, track):
                res = mx.eigs(0, phasing=tr, **opts)
                assert res.converged[[0, 2]].all() and res.iterations.max() <= 75
                _check_eigs(f"planted balanced={balanced} {opts} track={tr is not None}", res, chs, nb, tr, **opts)
            flipped = mx.eigs(0, phasing=-track, **opts)                      # the other sign of the track: the other sign of every vector
            ok = ~np.isnan(res.vectors)
            assert np.array_equal(flipped.vectors[ok], -res.vectors[ok])
        s, w, r = mx.eigs_timing_ms(0)
        assert s > 0 and w > 0 and r > 0
        # max_iters = 2: not converged, two sweeps, what there is has unit norm
        chs = _chroms(mx, 0, nb, off, balanced)
        res = mx.eigs(0, max_iters=2)
        assert not res.converged.any() and res.iterations.tolist() == [2, 0, 2] and res.info.converged == 0 and res.info.max_iterations == 2
        for c in (0, 2):
            g = chs[c].good
            for j in range(3):
                x = res.vectors[j, chs[c].lo:chs[c].hi]
                assert np.array_equal(np.isnan(x), ~g) and abs(np.linalg.norm(x[g]) - 1.0) <= (g.sum() + 2) * U


def test_eigenpairs_across_reduction_chunks():
    """one chromosome of 400 bins: the 8 x 8 dot products are sums over two chunks of 256 bins.  With clip 2 the isolated cell of 3 000
    contacts does not make a pair of equal |lambda| (checked by the separations below)."""
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    opts = dict(n_eigs=2, clip=2.0)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        chs = _chroms(mx, 0, nb, off, False, **opts)
        lam = np.abs(gd.reference_eigs(chs[0], 2)[0])
        assert nb == 400 and chs[0].good.sum() > 256 and lam[0] >= 1.25 * lam[1] and lam[1] >= 1.1 * lam[2] and lam[1] >= 1.5 * lam[8]
        it, conv, _, _ = gd.block_iteration(chs[0], **gd.options(**opts))
        assert conv and it <= 75
        res = mx.eigs(0, **opts)
        assert res.converged.all() and res.iterations.max() <= 75
        _check_eigs("band, 400 bins", res, chs, nb, None, **opts)


# ---- the same bits on a second call, by another route and in another process ------------------------------------------------------------
def _all_bytes(mx, k, **opts):
    r = mx.eigs(k, **opts)
    return b"".join(a.tobytes() for a in (r.vectors, r.lambdas, r.resid, r.n_good, r.iterations, r.converged.astype(np.uint8)))


def test_same_bits_by_every_route(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells, track = gi.planted()
    with _loaded(text, [gi.R], ttext) as mx:
        mx.balance(0)
        mx.expected(0)
        first = _all_bytes(mx, 0)
        assert _all_bytes(mx, 0) == first
    from microcket_amd import capi
    hip = C.CDLL(capi.hip_runtimes()[0])                                      # the runtime the library itself uses
    d_text = C.c_void_p()
    with m.Matrix(ttext, [gi.R], device=0) as mx:
        assert hip.hipMalloc(C.byref(d_text), C.c_size_t(len(text))) == 0
        try:
            assert hip.hipMemcpy(d_text, text, C.c_size_t(len(text)), 1) == 0 # hipMemcpyHostToDevice
            mx.add_device(d_text.value, len(text))
        finally:
            hip.hipFree(d_text)
        mx.run()
        mx.balance(0)
        mx.expected(0)
        assert _all_bytes(mx, 0) == first
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    script = ("import sys, numpy as np, microcket_amd as m\n"
              "mx = m.Matrix(open(sys.argv[1], 'rb').read(), [1000])\n"
              "mx.add(open(sys.argv[2], 'rb').read()); mx.run(); mx.balance(0); mx.expected(0)\n"
              "r = mx.eigs(0)\n"
              "parts = [a.tobytes() for a in (r.vectors, r.lambdas, r.resid, r.n_good, r.iterations, r.converged.astype(np.uint8))]\n"
              "open(sys.argv[3], 'wb').write(b''.join(parts)); mx.close()\n")
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "g.sizes"), str(tmp_path / "in.pairs"), str(tmp_path / "out")], env=env, cwd=util.ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out", "rb").read() == first


# ---- state and argument errors ------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    with m.Matrix(ttext, [li.R_EDGE, 5 * li.R_EDGE]) as mx:
        with pytest.raises(m.MktError, match="eigs before run"):
            mx.eigs(0)
        mx.add(text)
        mx.run()
        with pytest.raises(m.MktError, match="expected first"):
            mx.eigs(0)
        with pytest.raises(m.MktError, match="expected first"):
            mx.eigs_apply(0, np.zeros(nb))
        with pytest.raises(m.MktError, match="eigs first"):
            mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 0, 0, 0, None), "fetch")
        mx.expected(0, use_weights=False)                                     # raw: no balance has built the transposed copy
        res = mx.eigs(0, n_eigs=2)
        assert res.info.solved == 1 and res.vectors.shape == (2, nb)
        loops = mx.loops(0)                                                   # loops and eigenvectors of one resolution leave each other alone
        assert np.array_equal(mx.eigs(0, n_eigs=2).vectors, res.vectors, equal_nan=True) and mx.loops(0).loops == loops.loops
        assert mx.loop_cells(0).status.size == mx.info(0)[1]
        with pytest.raises(m.MktError, match="expected first"):
            mx.eigs(1)                                                        # the other resolution has no tables
        mx.expected(1, use_weights=False)
        other = mx.eigs(1, n_eigs=1)
        assert other.vectors.shape == (1, mx.info(1)[0])
        buf = np.zeros(nb)
        mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 1, 0, nb, buf.ctypes.data_as(C.c_void_p)), "fetch")
        assert np.array_equal(buf, res.vectors[1], equal_nan=True)            # two resolutions do not disturb each other
        with pytest.raises(m.MktError, match="resolution index"):
            mx.eigs(2)
        for bad, what in ((dict(n_eigs=0), "n_eigs"), (dict(n_eigs=5), "n_eigs"), (dict(ignore_diags=-1), "ignore_diags"), (dict(min_good=-1), "min_good"),
                          (dict(max_iters=-1), "max_iters"), (dict(tol=0.0), "tol"), (dict(tol=1.0), "tol"), (dict(tol=float("nan")), "tol"),
                          (dict(clip=-1.0), "clip"), (dict(clip=float("nan")), "clip")):
            with pytest.raises(m.MktError, match=what):
                mx.eigs(0, **bad)
            with pytest.raises(m.MktError, match=what):
                mx.eigs_apply(0, np.zeros(nb), **bad)
        o = m.EigsOpts()
        mx.L.mkt_eigs_opts_default(C.byref(o))
        assert (o.n_eigs, o.ignore_diags, o.min_good, o.max_iters, o.tol, o.clip, o.reserved) == (3, 2, 9, 300, 1e-8, 0.0, 0)
        o.reserved = 3
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_eigs(mx.h, 0, C.byref(o), None, None), "eigs")
        mx._chk(mx.L.mkt_matrix_eigs(mx.h, 0, None, None, None), "eigs")     # NULL options: the defaults
        with pytest.raises(m.MktError, match="eigenvector 3"):
            mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 3, 0, 0, None), "fetch")
        with pytest.raises(m.MktError, match="eigenvector bins"):
            mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 0, nb - 1, 2, None), "fetch")
        with pytest.raises(m.MktError, match="eigenvalues of chromosomes"):
            mx._chk(mx.L.mkt_matrix_fetch_eigvals(mx.h, 0, 1, 1, *[None] * 5), "fetch")
        mx._chk(mx.L.mkt_matrix_fetch_eigvals(mx.h, 0, 0, 1, *[None] * 5), "fetch")      # any pointer may be NULL
        with pytest.raises(m.MktError, match="ncols"):
            mx.eigs_apply(0, np.zeros((nb, 9)))
        assert mx.L.mkt_matrix_eigs_timing(mx.h, 2, None, None, None) != 0 and mx.L.mkt_abi_version() == 9
        # a later expected, balance, run or add of that resolution discards the results
        line = text.splitlines(keepends=True)[0]
        for what, again in (("expected", lambda: mx.expected(0, use_weights=False)), ("balance", lambda: mx.balance(0, min_nnz=1)), ("run", lambda: mx.run()),
                            ("add", lambda: mx.add(line))):
            mx.run()
            mx.expected(0, use_weights=False)
            assert mx.eigs(0).info.solved == 1 and mx.eigs_timing_ms(0)[1] > 0
            again()
            with pytest.raises(m.MktError, match="eigs first"):
                mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 0, 0, 0, None), "fetch")
            assert mx.eigs_timing_ms(0) == (0.0, 0.0, 0.0), what
        mx.run()
        mx.balance(0, min_nnz=1)
        with pytest.raises(m.MktError, match="expected first"):               # the balance took the tables with it
            mx.eigs(0)


# ---- the executable ------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")


def test_executable_writes_the_eigenvectors(tmp_path):
    _need_gpu()
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()
    ttext, text, off, nb, cells, track = gi.planted()
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    for d in "abcde":
        os.makedirs(tmp_path / d)
    run = lambda d, *a, r=str(gi.R): subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", r, "-o", str(tmp_path / d / "o"), *a, str(tmp_path / "in.pairs")],
                                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run("a", "--expected").returncode == 0 and run("c").returncode == 0
    bins = open(tmp_path / "a" / f"o.{gi.R}.bins.bed").read().splitlines()
    names = ["c0", "c1", "c2"]
    with open(tmp_path / "track.bed", "w") as f:
        for line, p in zip(bins, track.tolist()):
            f.write(f"{line}\t{p!r}\n")
    r = run("b", "--eigs", "--eigs-track", str(tmp_path / "track.bed"), "--eigs-n", "2", "--eigs-clip", "1.5")
    assert r.returncode == 0 and b"WARN" not in r.stderr, r.stderr
    plain = sorted([f"o.{gi.R}.coo", f"o.{gi.R}.bins.bed", "o.matrix.stat"])
    exp = sorted(plain + [f"o.{gi.R}.expected{x}.tsv" for x in ("", ".chrom", ".trans")])
    assert sorted(os.listdir(tmp_path / "c")) == plain and sorted(os.listdir(tmp_path / "a")) == exp
    assert sorted(os.listdir(tmp_path / "b")) == sorted(exp + [f"o.{gi.R}.eigs.tsv", "o.eigs.stat"])          # --eigs implies --expected
    for f in exp:                                                             # --eigs changes none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    with _loaded(text, [gi.R], ttext) as mx:
        mx.expected(0, use_weights=False)
        res = mx.eigs(0, phasing=track, n_eigs=2, clip=1.5)
        lines = open(tmp_path / "b" / f"o.{gi.R}.eigs.tsv").read().splitlines()
        assert lines[0].split("\t") == ["chrom", "start", "end", "E1", "E2"] and len(lines) == 1 + nb
        got = np.array([[float(v) for v in l.split("\t")[3:]] for l in lines[1:]]).T
        assert np.array_equal(got, res.vectors, equal_nan=True)               # %.17g parses back to exactly the API's doubles
        assert ["\t".join(l.split("\t")[:3]) for l in lines[1:]] == bins and "nan" in lines[1 + off[1]]
        stat = [l.split("\t") for l in open(tmp_path / "b" / "o.eigs.stat").read().splitlines()]
        assert len(stat) == 3
        for c, row in enumerate(stat):
            assert row[:6] == [str(gi.R), names[c], str(gi.PLANT_BINS[c]), str(res.n_good[c]), str(res.iterations[c]), str(int(res.converged[c]))]
            assert np.array_equal(np.array([float(v) for v in row[6:]]), res.lambdas[c], equal_nan=True)
    # not converged: a warning, exit 0
    r = run("d", "--eigs", "--eigs-max-iters", "2", "--balance")
    assert r.returncode == 0 and r.stderr.count(b"WARN: eigenvectors of") == 2, r.stderr
    assert [l.split("\t")[4:6] for l in open(tmp_path / "d" / "o.eigs.stat").read().splitlines()] == [["2", "0"], ["0", "0"], ["2", "0"]]
    # usage and values
    assert run("e", "--eigs-n", "2").returncode == 2                          # a sub-option without --eigs
    assert run("e", "--eigs", "--eigs-track", str(tmp_path / "track.bed"), r=f"{gi.R},{2 * gi.R}").returncode == 2      # a track with two resolutions
    for bad in (("--eigs-n", "5"), ("--eigs-n", "0"), ("--eigs-tol", "1.5"), ("--eigs-tol", "x"), ("--eigs-clip", "-1"), ("--eigs-ignore-diags", "-2"),
                ("--eigs-min-good", "1.5"), ("--eigs-max-iters", "")):
        assert run("e", "--eigs", *bad).returncode == 12, bad
    with open(tmp_path / "short.bed", "w") as f:
        f.write("\n".join(f"{l}\t1" for l in bins[:-1]) + "\n")
    with open(tmp_path / "wrong.bed", "w") as f:
        f.write("\n".join(f"{l}\t1" for l in bins[:5] + bins[4:-1]) + "\n")
    for bad in ("short.bed", "wrong.bed"):
        assert run("e", "--eigs", "--eigs-track", str(tmp_path / bad)).returncode == 12, bad
    assert os.listdir(tmp_path / "e") == []
