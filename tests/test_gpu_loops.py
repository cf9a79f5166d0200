"""Loop calling on the GPU (mkt_matrix_loops, Matrix.loops / loop_cells, pairs2matrix --loops) against the definition restated in
tests/loopsdef.py, fed the GPU's own weights and expected table.  Integers (Csum_LL, window, kept positions, status, integer-valued
Bsum) must be identical; Esum, e_R and r_R agree within P x 2^-52 relative, P = the region's kept positions (the bound of
reordering a sum of P positive terms) plus 3 x 2^-52 for the three operations behind the sum.  The statistics are checked in stages:
chunks against the definition except within that bound of an edge, then histogram, thresholds, flags and loops exactly against the
definition applied to the GPU's own per-cell arrays.  Parity with juicer_tools is unpinned (it is not run)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import expected_inputs as xi
import expecteddef as ed
import loops_inputs as li
import loopsdef as ld
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
U = 2.0 ** -52


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _loaded(text, res, table):
    mx = m.Matrix(table, list(res), device=0)
    mx.add(text)
    mx.run()
    return mx


def _want(mx, k, nb, off, use_weights, **opts):
    """the definition's per-cell results for the GPU's own cells, weights and expected table"""
    b1, b2, c = mx.cells(k)
    w = mx.weights(k) if use_weights else None
    e = mx.expected(k, use_weights=use_weights)
    want = ld.cells_pass(b1, b2, c, nb, off, e.genome.expected_smooth, weights=w, **opts)
    return (b1.astype(np.int64), b2.astype(np.int64), c.astype(np.int64)), want


def _compare_cells(label, got, want, exact_bsum):
    """integers identical; Esum, e, r within (P + 3) x 2^-52; chunks identical except where the definition's r is that close to an edge.
    Returns the number of borderline tested cells."""
    cand = want.status != ld.NONE
    assert np.array_equal(got.window, want.window), label
    assert np.array_equal(got.csum_ll, want.csum_ll), label
    assert np.array_equal(got.kept, want.kept), label
    if exact_bsum:
        assert np.array_equal(got.bsum, want.bsum), label
    P = want.kept.astype(np.float64)
    for name, g, w_, extra in (("bsum", got.bsum, want.bsum, 0), ("esum", got.esum, want.esum, 0), ("e", got.e, want.e, 3), ("r", got.r, want.r, 3)):
        assert (np.isnan(g) == np.isnan(w_)).all(), (label, name)
        ok = ~np.isnan(w_) & (w_ != 0)
        assert (g[~ok & ~np.isnan(w_)] == 0).all(), (label, name)
        dev = np.abs(g[ok] / w_[ok] - 1.0)
        bound = (P[ok] + extra) * U
        print(f"{label} {name}: max rel dev {dev.max() if dev.size else 0.0:.3e} (bound at that cell {bound[np.argmax(dev - bound)] if dev.size else 0.0:.3e})")
        assert (dev <= bound).all(), (label, name, float(dev.max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        near = (np.abs(want.r[:, :, None] / ld.EDGES[None, None, :] - 1.0) <= ((P + 3) * U)[:, :, None]).any(axis=2)
    differs = got.chunk != want.chunk
    assert not (differs & ~near).any(), label
    border = near.any(axis=1) & cand
    # the status can depend on rounding only through r <= 512, the last edge: everywhere else it is identical
    with np.errstate(invalid="ignore", divide="ignore"):
        near_last = (np.abs(want.r / ld.EDGES[-1] - 1.0) <= (P + 3) * U).any(axis=1)
    assert np.array_equal(got.status[~near_last], want.status[~near_last]), label
    return int((border & (want.status == ld.TESTED)).sum())


def _rest_from(got, cells, off, opts):
    """steps 6 .. 9 of the definition applied to the GPU's own (status, window, chunk, r)"""
    b1, b2, c = cells
    o = ld.options(**opts)
    H = ld.histogram(got.status, got.chunk, c)
    T = ld.thresholds(H, o["fdr"])
    en = ld.enriched(got.status, got.chunk, c, T)
    return H, T, en, ld.loops(b1, b2, c, off, en, got.window, got.r, o["cluster_radius"])


def _compare_rest(label, mx, k, got, cells, off, opts, res):
    H, T, en, L = _rest_from(got, cells, off, opts)
    assert np.array_equal(mx.loop_hist(k), H), label
    assert np.array_equal(mx.loop_thresholds(k), T), label
    assert np.array_equal(got.enriched.astype(bool), en), label
    assert [tuple(x) for x in res.loops] == [tuple(x) for x in L], label
    i = res.info
    st = got.status
    assert (i.cells, i.candidates, i.tested, i.undefined, i.over) == (st.size, int((st != 0).sum()), int((st == 1).sum()), int((st == 2).sum()), int((st == 3).sum())), label
    o = ld.options(**opts)
    assert i.grew == int(((got.window > o["window"]) & (st != 0)).sum()) and i.enriched == int(en.sum()) and i.loops == len(L), label
    assert i.at_max == int(((got.window == o["window_max"]) & (got.csum_ll < o["min_ll_count"]) & (st != 0)).sum()), label
    return H, T, en, L


EDGE_OPTS = (dict(), dict(peak=1, window=3, window_max=7, min_dist=0, min_ll_count=40), dict(min_dist=2, window=20, window_max=20))


# ---- 1. chromosome starts, ends and neighbours; raw counts, so every Bsum is an integer ------------------------------------------------
def test_edge_table_exact():
    _need_gpu()
    ttext, text, off, nb, cells, _ = li.edge_matrix(False)
    assert off == [0, 1, 13, 77, 142] and nb == 183
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        assert (np.stack(mx.cells(0), axis=1) == cells).all()
        for opts in EDGE_OPTS:
            cl, want = _want(mx, 0, nb, off, False, **opts)
            res = mx.loops(0, **opts)
            got = mx.loop_cells(0)
            _compare_cells(f"edge {opts}", got, want, exact_bsum=True)
            assert (want.status == ld.TESTED).sum() > 200 and (want.status == ld.NONE).any()
            _compare_rest(f"edge {opts}", mx, 0, got, cl, off, opts, res)
        assert (want.status == ld.UNDEFINED).any()                            # window 20 in chromosomes of 12 .. 65 bins


# ---- 2. masked bins: regions lose exactly those positions ----------------------------------------------------------------------------------
def test_masked_bins():
    _need_gpu()
    ttext, text, off, nb, cells, empty = li.edge_matrix(True)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        w = mx.weights(0)
        assert set(np.flatnonzero(np.isnan(w)).tolist()) == empty and len(empty) >= 5
        opts = dict(min_dist=0, min_ll_count=30)
        (b1, b2, c), want = _want(mx, 0, nb, off, True, **opts)
        res = mx.loops(0, **opts)
        got = mx.loop_cells(0)
        _compare_cells("masked", got, want, exact_bsum=False)
        _compare_rest("masked", mx, 0, got, (b1, b2, c), off, opts, res)
        # a cell two bins from a masked bin, position by position
        dense = np.zeros((nb, nb), dtype=np.int64)
        dense[b1, b2] = c
        dense[b2, b1] = c
        E = mx.expected(0).genome.expected_smooth
        bounds = off + [nb]
        checked = 0
        for s in np.flatnonzero((b1 >= off[3]) & (b1 < off[4]) & (got.status != 0))[::23]:
            win, cs, bs, es, kp = ld.brute_cell(dense, ~np.isnan(w), bounds[3], bounds[4], E, w, int(b1[s]), int(b2[s]), **opts)
            assert (got.window[s], int(got.csum_ll[s]), got.kept[s].tolist()) == (win, cs, kp)
            checked += 1
        assert checked >= 20
        # near the diagonal LL has no kept position: such a cell is not tested
        lost = (got.kept[:, 1] == 0) & (got.status != 0)
        assert lost.any() and (got.status[lost] == ld.UNDEFINED).all() and np.isnan(got.r[lost, 1]).all()
        # a cell eleven bins from the diagonal whose LL rows (window 5, no growth) are the five masked bins: LL is lost to the mask alone
        opts = dict(window_max=5)
        _, want = _want(mx, 0, nb, off, True, **opts)
        res = mx.loops(0, **opts)
        got = mx.loop_cells(0)
        _compare_cells("masked, window 5", got, want, exact_bsum=False)
        cell = lambda t: int(np.flatnonzero((b1 == off[t[0]] + t[1]) & (b2 == off[t[0]] + t[2]))[0])
        s0, s1 = cell(li.LL_LOST), cell(li.LL_KEPT)
        assert np.isnan(w[off[4] + 20:off[4] + 25]).all() and not np.isnan(w[[off[4] + 18, off[4] + 19, off[4] + 30]]).any()
        assert got.window[s0] == 5 and got.kept[s0, 1] == 0 and (got.kept[s0, [0, 2, 3]] > 0).all() and got.status[s0] == ld.UNDEFINED
        assert np.isnan(got.r[s0, 1]) and not np.isnan(got.r[s0, [0, 2, 3]]).any() and got.chunk[s0, 1] == ld.NOCHUNK
        assert got.kept[s1, 1] == 5 - 2 and got.status[s1] == ld.TESTED       # one row up, row 19 is there: columns 25, 26, 27 of it


# ---- 3. window growth, 4. limits -----------------------------------------------------------------------------------------------------------
def test_window_growth_and_limits():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        cl, want = _want(mx, 0, nb, off, False)
        cand = want.status != ld.NONE
        assert set(want.window[cand].tolist()) == set(range(5, 21))           # every window occurs ...
        assert ((want.window == 20) & (want.csum_ll < 16) & cand).any()      # ... and some cells stop at window_max below min_ll_count
        res = mx.loops(0)
        got = mx.loop_cells(0)
        _compare_cells("band", got, want, exact_bsum=True)
        H, T, en, L = _compare_rest("band", mx, 0, got, cl, off, {}, res)
        assert res.info.grew > 0 and res.info.at_max > 0
        # the isolated cell with 3000 contacts: nothing around it, so r = 0 in every region: chunk 0, and the last column of the histogram
        s = int(np.flatnonzero((cl[0] == 40) & (cl[1] == 330))[0])
        assert cl[2][s] == 3000 and got.status[s] == ld.TESTED and got.window[s] == 20 and (got.r[s] == 0.0).all() and (got.chunk[s] == 0).all()
        assert (mx.loop_hist(0)[:, 0, 2047] >= 1).all()
    # r = k exactly in every region.  512.0 is the last edge itself (r <= edge_27 holds: chunk 27) and 513.0 the next integer count past
    # it (OVER): the boundary value and one count beyond, not values one ulp either side of the edge.
    for k, status, chunk in ((512, ld.TESTED, 27), (513, ld.OVER, ld.NOCHUNK)):
        ttext, text, off, nb, cells = li.flat_matrix(k)
        with _loaded(text, [li.R_EDGE], ttext) as mx:
            mx.expected(0, use_weights=False)
            res = mx.loops(0)
            got = mx.loop_cells(0)
            cand = got.status != 0
            assert cand.sum() == sum(30 - d for d in range(8, 30))
            inner = cand & (got.kept > 0).all(axis=1)
            assert inner.sum() > 100 and (got.r[inner] == float(k)).all() and (got.status[inner] == status).all() and (got.chunk[inner] == chunk).all()
            assert res.info.over == (inner.sum() if status == ld.OVER else 0) and res.info.tested == (inner.sum() if status == ld.TESTED else 0)


# ---- 5. statistics, staged ---------------------------------------------------------------------------------------------------------------------
def test_statistics_on_planted_loops():
    _need_gpu()
    text, cells, pixels = li.planted()
    opts = li.STAT_OPTS
    with _loaded(text, li.STAT_RES, xi.TABLE) as mx:
        for k, r in enumerate(li.STAT_RES):
            off, nb = xi.offsets(r)
            assert (np.stack(mx.cells(k), axis=1) == cells[r]).all()
            cl, want = _want(mx, k, nb, off, False, **opts)
            # the definition alone, on the CPU: it finds every planted pixel, and at least three chunks have a finite threshold
            H0, T0, en0, L0 = _rest_from(want, cl, off, opts)
            for x, y in pixels[r]:
                assert any(max(abs(l.bin1 - x), abs(l.bin2 - y)) <= 2 for l in L0), (r, x, y)
            assert (T0 < 2048).any(axis=0).sum() >= 3, T0                      # chunks with a finite threshold
            res = mx.loops(k, **opts)
            got = mx.loop_cells(k)
            border = _compare_cells(f"r={r}", got, want, exact_bsum=True)
            tested = int((want.status == ld.TESTED).sum())
            print(f"r={r}: {tested} tested cells, {border} within the bound of an edge, {len(res.loops)} loops")
            assert tested > 10000 and border * 1000 <= tested
            H, T, en, L = _compare_rest(f"r={r}", mx, k, got, cl, off, opts, res)
            p, h, f = mx.loops_timing_ms(k)
            assert p > 0 and h > 0 and f > 0


# ---- 6. the same bits on a second call, in another process and by another route ---------------------------------------------------------
def _all_bytes(mx, k, **opts):
    res = mx.loops(k, **opts)
    return b"".join([a.tobytes() for a in mx.loop_cells(k)] + [mx.loop_hist(k).tobytes(), mx.loop_thresholds(k).tobytes(), repr(res.loops).encode()])


def test_same_bits_by_every_route(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1, ignore_diags=1)
        mx.expected(0)
        first = _all_bytes(mx, 0)
        assert _all_bytes(mx, 0) == first
        mx.expected(0)                                                        # new tables discard the loops; the next call gives them again
        assert _all_bytes(mx, 0) == first
    lines = text.splitlines(keepends=True)
    other = b"".join(lines[i] for i in np.random.default_rng(4).permutation(len(lines)).tolist())
    with m.Matrix(ttext, [li.R_EDGE], device=0) as mx:
        for at in range(0, len(other), 100_003):                              # chunks that end inside a line
            mx.add(other[at:at + 100_003])
        mx.run()
        mx.balance(0, min_nnz=1, ignore_diags=1)
        mx.expected(0)
        assert _all_bytes(mx, 0) == first
    from microcket_amd import capi
    hip = C.CDLL(capi.hip_runtimes()[0])                                      # the runtime the library itself uses
    d_text = C.c_void_p()
    with m.Matrix(ttext, [li.R_EDGE], device=0) as mx:
        assert hip.hipMalloc(C.byref(d_text), C.c_size_t(len(text))) == 0
        try:
            assert hip.hipMemcpy(d_text, text, C.c_size_t(len(text)), 1) == 0 # hipMemcpyHostToDevice
            mx.add_device(d_text.value, len(text))
        finally:
            hip.hipFree(d_text)
        mx.run()
        mx.balance(0, min_nnz=1, ignore_diags=1)
        mx.expected(0)
        assert _all_bytes(mx, 0) == first
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    script = ("import sys, microcket_amd as m\n"
              "mx = m.Matrix(open(sys.argv[1], 'rb').read(), [1000])\n"
              "mx.add(open(sys.argv[2], 'rb').read()); mx.run(); mx.balance(0, min_nnz=1, ignore_diags=1); mx.expected(0)\n"
              "res = mx.loops(0)\n"
              "parts = [a.tobytes() for a in mx.loop_cells(0)] + [mx.loop_hist(0).tobytes(), mx.loop_thresholds(0).tobytes(), repr(res.loops).encode()]\n"
              "open(sys.argv[3], 'wb').write(b''.join(parts)); mx.close()\n")
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "g.sizes"), str(tmp_path / "in.pairs"), str(tmp_path / "out")], env=env, cwd=util.ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out", "rb").read() == first
    # the add_keys route against the text route
    c = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
    try:
        p = c.run_bytes(util.synth("unc", 61, 20000), chunk=1 << 20)[0]
        with m.Matrix(xi.TABLE, [2500000]) as a, _loaded(p, [2500000], xi.TABLE) as b:
            a.add_keys(c, True, None)
            a.run()
            o = dict(min_dist=1, min_ll_count=4)
            for x in (a, b):
                x.expected(0, use_weights=False)
            assert a.info(0)[1] == b.info(0)[1] > 0 and _all_bytes(a, 0, **o) == _all_bytes(b, 0, **o)
            assert a.loops(0, **o).info.candidates > 0
    finally:
        c.close()


# ---- 7. state, argument and discard errors; the executable -------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    with m.Matrix(ttext, [li.R_EDGE, 5 * li.R_EDGE]) as mx:
        with pytest.raises(m.MktError, match="loops before run"):
            mx.loops(0)
        mx.add(text)
        mx.run()
        nnz = mx.info(0)[1]
        with pytest.raises(m.MktError, match="expected first"):
            mx.loops(0)
        with pytest.raises(m.MktError, match="loops first"):
            mx.loop_cells(0)
        mx.expected(0, use_weights=False)                                     # raw: no balance, the pass builds its own row pointers
        res = mx.loops(0)
        assert res.info.cells == nnz and res.info.tested > 0
        with pytest.raises(m.MktError, match="expected first"):
            mx.loops(1)                                                       # the other resolution has no tables
        with pytest.raises(m.MktError, match="resolution index"):
            mx.loops(2)
        for bad, what in ((dict(peak=-1), "peak"), (dict(window=2), "window"), (dict(window_max=4), "window_max"), (dict(window_max=21), "window_max"),
                          (dict(fdr=0.0), "fdr"), (dict(fdr=1.0), "fdr"), (dict(fdr=float("nan")), "fdr"), (dict(min_dist=-1), "min_dist"),
                          (dict(cluster_radius=-1), "cluster_radius"), (dict(min_ll_count=-1), "min_ll_count")):
            with pytest.raises(m.MktError, match=what):
                mx.loops(0, **bad)
        o = m.LoopsOpts()
        mx.L.mkt_loops_opts_default(C.byref(o))
        assert (o.peak, o.window, o.window_max, o.min_ll_count, o.min_dist, o.max_dist, o.fdr, o.cluster_radius, o.reserved) == (2, 5, 20, 16, 8, 0, 0.1, 2, 0)
        o.reserved = 3
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_loops(mx.h, 0, C.byref(o), None), "loops")
        assert mx.loop_cells(0).status.size == nnz                            # a refused call leaves the results alone
        mx._chk(mx.L.mkt_matrix_loops(mx.h, 0, None, None), "loops")         # NULL options: the defaults
        buf = (C.c_uint8 * 8)()
        with pytest.raises(m.MktError, match="loop cells"):
            mx._chk(mx.L.mkt_matrix_fetch_loop_cells(mx.h, 0, nnz - 2, 4, buf, *[None] * 9), "fetch")
        mx._chk(mx.L.mkt_matrix_fetch_loop_cells(mx.h, 0, nnz - 4, 4, buf, *[None] * 9), "fetch")       # any pointer may be NULL
        assert list(buf)[:4] == mx.loop_cells(0).status[-4:].tolist()
        mx._chk(mx.L.mkt_matrix_fetch_loop_cells(mx.h, 0, nnz, 0, *[None] * 10), "fetch")
        with pytest.raises(m.MktError, match="loops \\["):
            mx._chk(mx.L.mkt_matrix_fetch_loops(mx.h, 0, len(res.loops), 1, None), "fetch")
        assert mx.L.mkt_abi_version() == 9
        # a later expected, balance, run or add (text, device text, keys) of that resolution discards the results
        from microcket_amd import capi
        hip = C.CDLL(capi.hip_runtimes()[0])
        line = text.splitlines(keepends=True)[0]
        d_line = C.c_void_p()
        assert hip.hipMalloc(C.byref(d_line), C.c_size_t(len(line))) == 0 and hip.hipMemcpy(d_line, line, C.c_size_t(len(line)), 1) == 0
        ctx = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
        try:
            ctx.run_bytes(util.synth("unc", 61, 2000), chunk=1 << 20)
            for what, again in (("expected", lambda: mx.expected(0, use_weights=False)), ("balance", lambda: mx.balance(0, min_nnz=1)), ("run", lambda: mx.run()),
                                ("add", lambda: mx.add(line)), ("add_device", lambda: mx.add_device(d_line.value, len(line))), ("add_keys", lambda: mx.add_keys(ctx, True, None))):
                mx.run()
                mx.expected(0, use_weights=False)
                assert mx.loops(0).info.tested > 0 and mx.loop_hist(0).any() and mx.loops_timing_ms(0)[0] > 0
                again()
                with pytest.raises(m.MktError, match="loops first"):
                    mx.loop_hist(0)
                with pytest.raises(m.MktError, match="loops first"):
                    mx.loop_cells(0)
                with pytest.raises(m.MktError, match="loops first"):
                    mx._chk(mx.L.mkt_matrix_fetch_loops(mx.h, 0, 0, 0, None), "fetch")
                assert mx.loops_timing_ms(0) == (0.0, 0.0, 0.0), what
        finally:
            ctx.close()
            hip.hipFree(d_line)
    with m.Matrix(xi.TABLE, [2500000]) as mx:                                 # an empty matrix
        assert mx.run() == (0, 0)
        mx.expected(0, use_weights=False)
        res = mx.loops(0)
        assert res.loops == [] and res.info.cells == 0 and not mx.loop_hist(0).any() and (mx.loop_thresholds(0) == 2048).all()


def test_executable_writes_the_loops(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    for d in "abc":
        os.makedirs(tmp_path / d)
    res = [li.R_EDGE, 2 * li.R_EDGE]
    rl = ",".join(map(str, res))
    run = lambda d, *a: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", rl, "-o", str(tmp_path / d / "o"), *a, str(tmp_path / "in.pairs")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    runs = [run("a", "--expected"), run("b", "--loops", "--loop-min-ll-count", "12", "--loop-fdr", "0.2"), run("c")]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted([f"o.{r}.coo" for r in res] + [f"o.{r}.bins.bed" for r in res] + ["o.matrix.stat"])
    exp = sorted(plain + [f"o.{r}.expected{x}.tsv" for r in res for x in ("", ".chrom", ".trans")])
    assert sorted(os.listdir(tmp_path / "c")) == plain and sorted(os.listdir(tmp_path / "a")) == exp
    assert sorted(os.listdir(tmp_path / "b")) == sorted(exp + [f"o.{r}.loops.bedpe" for r in res] + ["o.loops.stat"])      # --loops implies --expected
    for f in exp:                                                             # --loops changes none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    assert run("c", "--loop-fdr", "0.2").returncode == 2                      # a sub-option without --loops
    os.makedirs(tmp_path / "e")
    for bad in (("--loop-fdr", "1.5"), ("--loop-window-max", "25"), ("--loop-window", "2"), ("--loop-window", "9", "--loop-window-max", "8"), ("--loop-peak", "x")):
        assert run("e", "--loops", *bad).returncode == 12, bad                # refused before anything is read or written
    assert os.listdir(tmp_path / "e") == []
    # every other sub-option, with --balance: the files equal the API's values
    os.makedirs(tmp_path / "d")
    sub = dict(peak=1, window=4, window_max=12, min_dist=6, max_dist=100, cluster_radius=1, min_ll_count=10)
    args = [x for k, v in sub.items() for x in ("--loop-" + k.replace("_", "-"), str(v))]
    assert run("d", "--balance", "--loops", *args).returncode == 0
    assert sorted(os.listdir(tmp_path / "d")) == sorted(exp + [f"o.{r}.weights.bed" for r in res] + ["o.balance.stat"] + [f"o.{r}.loops.bedpe" for r in res] + ["o.loops.stat"])
    dstat = open(tmp_path / "d" / "o.loops.stat", "rb").read().decode().splitlines()
    with _loaded(text, res, ttext) as mx:
        for k, r in enumerate(res):
            mx.balance(k)
            mx.expected(k)
            got = mx.loops(k, **sub)
            i = got.info
            assert dstat[k] == "\t".join(map(str, (r, i.cells, i.candidates, i.tested, i.undefined, i.over, i.grew, i.at_max, i.enriched, i.loops)))
            lines = open(tmp_path / "d" / f"o.{r}.loops.bedpe", "rb").read().decode().splitlines()
            assert len(lines) == 1 + len(got.loops)
            for line, L in zip(lines[1:], got.loops):
                f = line.split("\t")
                assert (int(f[1]), int(f[4]), int(f[6]), int(f[11]), int(f[12])) == (L.bin1 * r, L.bin2 * r, L.count, L.window, L.n_cells) and tuple(float(x) for x in f[7:11]) == L.r
    stat = open(tmp_path / "b" / "o.loops.stat", "rb").read().decode().splitlines()
    with _loaded(text, res, ttext) as mx:
        for k, r in enumerate(res):
            mx.expected(k, use_weights=False)
            got = mx.loops(k, min_ll_count=12, fdr=0.2)
            i = got.info
            assert stat[k] == "\t".join(map(str, (r, i.cells, i.candidates, i.tested, i.undefined, i.over, i.grew, i.at_max, i.enriched, i.loops)))
            lines = open(tmp_path / "b" / f"o.{r}.loops.bedpe", "rb").read().decode().splitlines()
            assert lines[0].split("\t") == ["#chrom1", "start1", "end1", "chrom2", "start2", "end2", "count", "expected_donut", "expected_ll", "expected_h", "expected_v",
                                            "window", "cells", "box_start1", "box_end1", "box_start2", "box_end2"]
            assert len(lines) == 1 + len(got.loops)
            for line, L in zip(lines[1:], got.loops):
                f = line.split("\t")
                assert f[0] == f[3] == "c0" and (int(f[1]), int(f[2]), int(f[4]), int(f[5])) == (L.bin1 * r, min((L.bin1 + 1) * r, 400000), L.bin2 * r, min((L.bin2 + 1) * r, 400000))
                assert int(f[6]) == L.count and tuple(float(x) for x in f[7:11]) == L.r and (int(f[11]), int(f[12])) == (L.window, L.n_cells)
                assert tuple(int(x) for x in f[13:]) == (L.box[0] * r, min((L.box[1] + 1) * r, 400000), L.box[2] * r, min((L.box[3] + 1) * r, 400000))
        assert len(mx.loops(0, min_ll_count=12, fdr=0.2).loops) > 0
