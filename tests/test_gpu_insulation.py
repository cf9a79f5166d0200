"""Insulation scores and boundaries on the GPU (mkt_matrix_insulation, Matrix.insulation / insulation_track, pairs2matrix --insulation)
against the definition restated in tests/insuldef.py, fed the GPU's own cells and weights.  Integers (n_valid, csum), the NaN pattern
and integer-valued bsum must be identical; other bsum agree within P x 2^-52 relative and scores within (P + 1) x 2^-52, P = the
stored cells at the diamond's kept positions: two orderings of a sum of P positive terms are each within (P - 1) x 2^-53 of the true
sum, and the score adds one division.  Steps 4 .. 7 are checked in stages against the definition applied to the GPU's own arrays.
Parity with cooltools is unpinned (it is not run)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import expected_inputs as xi
import insuldef as idf
import insulation_inputs as ii
import loops_inputs as li
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
U = 2.0 ** -52
FIELDS = ("n_valid", "csum", "bsum", "score", "log2_score", "strength", "boundary")


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


def _cells(mx, k):
    return tuple(a.astype(np.int64) for a in mx.cells(k))


def _same(a, b):
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _compare_sums(label, mx, k, windows, want, sc, exact):
    """window by window: integers and the NaN pattern identical; bsum identical (exact) or within P x 2^-52, the score within one more"""
    worst = (0.0, 0.0)
    for j in range(len(windows)):
        got = mx.insulation_track(k, j)
        assert np.array_equal(got.n_valid, want.n_valid[j]), (label, windows[j])
        assert np.array_equal(got.csum, want.csum[j]), (label, windows[j])
        assert np.array_equal(np.isnan(got.score), np.isnan(sc[j])), (label, windows[j])
        assert not np.isnan(got.bsum).any()
        P = want.stored[j].astype(np.float64)
        if exact:
            assert np.array_equal(got.bsum, want.bsum[j]), (label, windows[j])
        for name, g, w_, bound in (("bsum", got.bsum, want.bsum[j], P * U), ("score", got.score, sc[j], (1.0 if exact else P + 1.0) * U)):
            ok = ~np.isnan(w_) & (w_ != 0)
            assert (g[~ok & ~np.isnan(w_)] == 0).all(), (label, name, windows[j])
            dev = np.abs(g[ok] / w_[ok] - 1.0)
            if dev.size and dev.max() >= worst[0]:
                worst = (float(dev.max()), float(np.broadcast_to(bound, g.shape)[ok][np.argmax(dev)]))
            assert (dev <= np.broadcast_to(bound, g.shape)[ok]).all(), (label, name, windows[j], float(dev.max()))
    print(f"{label} windows {windows}: largest relative deviation {worst[0]:.3e} (bound there {worst[1]:.3e})")


def _check(label, mx, k, nb, off, windows, use_weights, exact, ignore_diags=2, fracs=(0.66,)):
    b1, b2, c = _cells(mx, k)
    w = mx.weights(k) if use_weights else None
    want = idf.sums(b1, b2, c, nb, off, windows, w, ignore_diags)
    for frac in fracs:
        sc = idf.score(want.n_valid, want.bsum, windows, ignore_diags, frac)
        info = mx.insulation(k, windows, use_weights=use_weights, ignore_diags=ignore_diags, min_frac_valid=frac)
        assert info.n_chrom == len(off) and info.windows == tuple(windows)
        _compare_sums(f"{label} ignore_diags {ignore_diags} min_frac_valid {frac}", mx, k, windows, want, sc, exact)
    return want, sc


# ---- 1. chromosome starts, ends and neighbours; raw counts, so every bsum is an integer ---------------------------------------------
def test_edges_raw_counts_exact():
    _need_gpu()
    ttext, text, off, nb, cells, _ = li.edge_matrix(False)
    assert off == [0, 1, 13, 77, 142] and nb == 183
    windows = (1, 2, 5, 20)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        assert (np.stack(mx.cells(0), axis=1) == cells).all()
        for ig in (0, 2):
            want, sc = _check("edge", mx, 0, nb, off, windows, False, True, ig, fracs=(0.0, 0.66))
            # window 20 inside the 12-bin chromosome: every diamond is clipped, and scored only with min_frac_valid 0
            assert (want.n_valid[3][1:13] < idf.n_full(20, ig)).all() and np.isnan(sc[3][1:13]).all()
            assert not np.isnan(idf.score(want.n_valid, want.bsum, windows, ig, 0.0)[3][2:12]).any()
            # the one-bin chromosome: the position (0, 0) with ignore_diags 0, none with 2
            assert want.n_valid[:, 0].tolist() == ([1] * 4 if ig == 0 else [0] * 4)
        got = mx.insulation_track(0, 0)                                      # window 1 with ignore_diags 2: n_full == 0
        assert idf.n_full(1, 2) == 0 and np.isnan(got.score).all() and np.isnan(got.log2_score).all() and not got.boundary.any()


# ---- 2. masked bins: the diamonds lose exactly those rows and columns -----------------------------------------------------------------
def test_masked_bins():
    _need_gpu()
    ttext, text, off, nb, cells, empty = li.edge_matrix(True)
    windows = (1, 2, 5, 20)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        w = mx.weights(0)
        assert set(np.flatnonzero(np.isnan(w)).tolist()) == empty and len(empty) >= 5
        want, _ = _check("masked", mx, 0, nb, off, windows, True, False, 2, fracs=(0.66, 0.0))
        _check("masked", mx, 0, nb, off, windows, True, False, 0, fracs=(0.5,))
        raw = idf.sums(*_cells(mx, 0), nb, off, windows, None, 2)
        assert (want.n_valid <= raw.n_valid).all() and (want.n_valid[2] < raw.n_valid[2]).sum() >= 20
        far = np.ones(nb, dtype=bool)                                         # bins whose window-5 diamond holds no masked bin
        for e in empty:
            far[max(e - 4, 0):e + 5] = False
        assert far.sum() > 50 and (want.n_valid[2][far] == raw.n_valid[2][far]).all()


# ---- 3. lane and shell boundaries ------------------------------------------------------------------------------------------------------------
BAND_WINDOWS = ((7, 8, 9), (31, 32, 33), (63, 64, 65, 66), (1, 64, 65, 130))


def test_lane_and_shell_boundaries():
    _need_gpu()
    ttext, text, off, nb, cells = ii.band()
    assert off == [0, 3, 303] and nb == 373
    with _loaded(text, [ii.R], ttext) as mx:
        assert (np.stack(mx.cells(0), axis=1) == cells).all()
        for windows in BAND_WINDOWS:
            want, sc = _check("band raw", mx, 0, nb, off, windows, False, True)
            together = [mx.insulation_track(0, j) for j in range(len(windows))]
            for j, W in enumerate(windows):                                   # each window alone: the same bits
                mx.insulation(0, (W,), use_weights=False)
                alone = mx.insulation_track(0, 0)
                for f in FIELDS:
                    assert getattr(alone, f).tobytes() == getattr(together[j], f).tobytes(), (windows, W, f)
            assert not np.isnan(sc[1][off[1] + windows[1]:off[2] - windows[1]]).any()
        assert np.isnan(sc[3][off[2]:]).all() and not np.isnan(sc[3][off[1] + 129:off[2] - 129]).any()      # window 130 in 70 and in 300 bins
        mx.balance(0, min_nnz=1, mad_max=0)                                   # masks the middle bin of the 3-bin chromosome: no contact two bins away
        assert np.flatnonzero(np.isnan(mx.weights(0))).tolist() == [1]
        for windows in BAND_WINDOWS:
            _check("band balanced", mx, 0, nb, off, windows, True, False)


# ---- 4. normalisation, minima, strengths and flags, staged ------------------------------------------------------------------------------------
def test_staged_boundaries_on_planted_domains():
    _need_gpu()
    ttext, text, off, nb, cells, edges = ii.planted()
    windows = (5, 10)
    with _loaded(text, [ii.R], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0)
        assert not np.isnan(mx.weights(0)).any()
        _check("planted", mx, 0, nb, off, windows, True, False)
        info = mx.insulation(0, windows)
        worst = 0.0
        for j in range(len(windows)):
            got = mx.insulation_track(0, j)
            L = idf.normalise(got.score, off, nb)                             # step 4 from the GPU's own score
            assert np.array_equal(np.isnan(got.log2_score), np.isnan(L)) and np.isfinite(L).sum() > nb - 40
            ok = ~np.isnan(L)
            ulps = np.abs(got.log2_score[ok] - L[ok]) / np.spacing(np.abs(L[ok]))
            worst = max(worst, float(ulps.max()))
            assert (ulps <= 2.0).all(), (windows[j], float(ulps.max()))
            st, bd, mn = idf.call(got.log2_score, off, nb, 0.2)               # steps 5 .. 7 from the GPU's own L
            assert _same(got.strength, st) and np.array_equal(got.boundary, bd) and np.array_equal(~np.isnan(got.strength), mn)
            assert (info.defined[j], info.minima[j], info.boundaries[j]) == (int(np.isfinite(got.log2_score).sum()), int(mn.sum()), int(bd.sum()))
        print(f"planted: log2 track within {worst:.2f} ulp of math.log2")
        assert ii.boundaries_are_the_planted(mx.insulation_track(0, 0).boundary, edges)
        s, t = mx.insulation_timing_ms(0)
        assert s > 0 and t > 0


# ---- 5. the same bits on a second call, in another object and by another route ---------------------------------------------------------
def _all_bytes(mx, k, windows, **opts):
    mx.insulation(k, windows, **opts)
    return b"".join(getattr(mx.insulation_track(k, j), f).tobytes() for j in range(len(windows)) for f in FIELDS)


def test_same_bits_by_every_route():
    _need_gpu()
    ttext, text, off, nb, cells, edges = ii.planted()
    windows = (3, 5, 10, 25)
    with _loaded(text, [ii.R], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0)
        first = _all_bytes(mx, 0, windows)
        assert _all_bytes(mx, 0, windows) == first
    lines = text.splitlines(keepends=True)
    other = b"".join(lines[i] for i in np.random.default_rng(4).permutation(len(lines)).tolist())
    with m.Matrix(ttext, [ii.R], device=0) as mx:
        for at in range(0, len(other), 100_003):                              # chunks that end inside a line
            mx.add(other[at:at + 100_003])
        mx.run()
        mx.balance(0, min_nnz=1, mad_max=0)
        assert _all_bytes(mx, 0, windows) == first
    # the add_keys route against the text route
    c = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
    try:
        p = c.run_bytes(util.synth("unc", 61, 20000), chunk=1 << 20)[0]
        with m.Matrix(xi.TABLE, [2500000]) as a, _loaded(p, [2500000], xi.TABLE) as b:
            a.add_keys(c, True, None)
            a.run()
            o = dict(use_weights=False, min_frac_valid=0.0, ignore_diags=1)
            assert a.info(0)[1] == b.info(0)[1] > 0 and _all_bytes(a, 0, (1, 2, 5), **o) == _all_bytes(b, 0, (1, 2, 5), **o)
            assert a.insulation_track(0, 2).csum.sum() > 0
    finally:
        c.close()


# ---- 6. state, argument and discard errors -------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    with m.Matrix(ttext, [li.R_EDGE, 5 * li.R_EDGE]) as mx:
        with pytest.raises(m.MktError, match="insulation before run"):
            mx.insulation(0)
        mx.add(text)
        mx.run()
        with pytest.raises(m.MktError, match="balance first"):
            mx.insulation(0)
        with pytest.raises(m.MktError, match="insulation first"):
            mx.insulation_track(0, 0)
        assert mx.insulation_timing_ms(0) == (0.0, 0.0)
        info = mx.insulation(0, use_weights=False)                            # raw: no balance, the sweep builds its own row pointers
        assert info.windows == (5, 10, 25) and info.n_chrom == 1 and info.defined[0] > 300
        mx.balance(0, min_nnz=1)
        with pytest.raises(m.MktError, match="insulation first"):             # new weights discard the scores
            mx.insulation_track(0, 0)
        with pytest.raises(m.MktError, match="balance first"):
            mx.insulation(1)                                                  # the other resolution has no weights
        with pytest.raises(m.MktError, match="resolution index"):
            mx.insulation(2)
        for windows, what in (((), "n_windows"), ((1, 2, 3, 4, 5), "n_windows"), ((0,), "window 0"), ((5, 1025), "window 1025"), ((5, 5), "ascending"), ((10, 5), "ascending")):
            with pytest.raises(m.MktError, match=what):
                mx.insulation(0, windows)
        for bad, what in ((dict(ignore_diags=-1), "ignore_diags"), (dict(use_weights=2), "use_weights"), (dict(min_frac_valid=-0.1), "min_frac_valid"),
                          (dict(min_frac_valid=1.5), "min_frac_valid"), (dict(min_frac_valid=float("nan")), "min_frac_valid"), (dict(min_strength=-1.0), "min_strength"),
                          (dict(min_strength=float("nan")), "min_strength")):
            with pytest.raises(m.MktError, match=what):
                mx.insulation(0, **bad)
        with pytest.raises(TypeError):
            mx.insulation(0, peak=1)
        o = m.InsulationOpts()
        mx.L.mkt_insulation_opts_default(C.byref(o))
        assert (o.n_windows, list(o.window), o.ignore_diags, o.use_weights, o.min_frac_valid, o.min_strength, o.reserved) == (3, [5, 10, 25, 0], 2, 1, 0.66, 0.2, 0)
        info = mx.insulation(0, (5, 10))
        o.reserved = 3
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_insulation(mx.h, 0, C.byref(o), None), "insulation")
        assert mx.insulation_track(0, 1).score.size == nb                     # a refused call leaves the results alone
        with pytest.raises(m.MktError, match="insulation window 2 of 2"):
            mx.insulation_track(0, 2)
        buf = (C.c_uint64 * 8)()
        with pytest.raises(m.MktError, match="insulation bins"):
            mx._chk(mx.L.mkt_matrix_fetch_insulation(mx.h, 0, 0, nb - 2, 4, buf, *[None] * 6), "fetch")
        mx._chk(mx.L.mkt_matrix_fetch_insulation(mx.h, 0, 0, nb - 4, 4, buf, *[None] * 6), "fetch")      # any pointer may be NULL
        assert list(buf)[:4] == mx.insulation_track(0, 0).n_valid[-4:].tolist()
        mx._chk(mx.L.mkt_matrix_fetch_insulation(mx.h, 0, 0, nb, 0, *[None] * 7), "fetch")
        mx._chk(mx.L.mkt_matrix_insulation(mx.h, 0, None, None), "insulation")                             # NULL options: the defaults
        assert mx.insulation_track(0, 2).n_valid.max() == idf.n_full(25, 2) and mx.L.mkt_abi_version() == 9
        # expected, loops, eigs and insulation of one resolution do not disturb each other
        ins_bytes = lambda: b"".join(getattr(mx.insulation_track(0, j), f).tobytes() for j in range(3) for f in FIELDS)

        def other_bytes():
            rows = mx.info(0)[0]
            g = [np.zeros(rows, np.uint64), np.zeros(rows, np.uint64)] + [np.zeros(rows, np.float64) for _ in range(3)]
            mx._chk(mx.L.mkt_matrix_fetch_expected_genome(mx.h, 0, 0, rows, *[a.ctypes.data_as(C.c_void_p) for a in g]), "fetch")
            v = np.zeros((2, nb), np.float64)
            for j in range(2):
                mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, j, 0, nb, v[j].ctypes.data_as(C.c_void_p)), "fetch")
            return b"".join([a.tobytes() for a in g] + [a.tobytes() for a in mx.loop_cells(0)] + [mx.loop_hist(0).tobytes(), v.tobytes(), mx.values(0, "oe").tobytes()])
        before = ins_bytes()
        mx.expected(0)
        mx.loops(0)
        mx.eigs(0, n_eigs=2)
        assert ins_bytes() == before                                          # ... by new tables, loops and eigenvectors
        others = other_bytes()
        mx.insulation(0, (4, 8, 16), ignore_diags=1)
        assert other_bytes() == others                                        # ... and those not by an insulation call
        mx.insulation(0)
        assert ins_bytes() == before
        # a later balance, run or add of that resolution discards the results
        line = text.splitlines(keepends=True)[0]
        for what, again in (("balance", lambda: mx.balance(0, min_nnz=1)), ("run", lambda: mx.run()), ("add", lambda: mx.add(line))):
            mx.run()
            mx.balance(0, min_nnz=1)
            assert mx.insulation(0).defined[0] > 300 and mx.insulation_timing_ms(0)[1] > 0
            again()
            with pytest.raises(m.MktError, match="insulation first"):
                mx.insulation_track(0, 0)
            assert mx.insulation_timing_ms(0) == (0.0, 0.0), what
    with m.Matrix(xi.TABLE, [2500000]) as mx:                                 # an empty matrix
        assert mx.run() == (0, 0)
        info = mx.insulation(0, use_weights=False)
        t = mx.insulation_track(0, 0)
        assert info.defined == (0, 0, 0) and info.boundaries == (0, 0, 0) and not t.csum.any() and t.n_valid.max() == 22 and np.isnan(t.log2_score).all()


# ---- 7. the executable ---------------------------------------------------------------------------------------------------------------------------
def test_executable_writes_the_insulation(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells, edges = ii.planted()
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    for d in "ab":
        os.makedirs(tmp_path / d)
    res, bp = [ii.R, 2 * ii.R], [4 * ii.R, 10 * ii.R]
    run = lambda d, *a: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", ",".join(map(str, res)), "-o", str(tmp_path / d / "o"), *a, str(tmp_path / "in.pairs")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    sub = ["--ins-ignore-diags", "1", "--ins-min-frac-valid", "0.5", "--ins-min-strength", "0.3"]
    runs = [run("a", "--balance"), run("b", "--balance", "--insulation", ",".join(map(str, bp)), *sub)]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted([f"o.{r}.{x}" for r in res for x in ("coo", "bins.bed", "weights.bed")] + ["o.matrix.stat", "o.balance.stat"])
    assert sorted(os.listdir(tmp_path / "a")) == plain                        # without --insulation no new file appears ...
    assert sorted(os.listdir(tmp_path / "b")) == sorted(plain + [f"o.{r}.insulation.tsv" for r in res] + ["o.insulation.stat"])
    for f in plain:                                                           # ... and --insulation changes none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    stat = open(tmp_path / "b" / "o.insulation.stat", "rb").read().decode().splitlines()
    assert len(stat) == 4
    with _loaded(text, res, ttext) as mx:
        for k, r in enumerate(res):
            mx.balance(k)
            windows = [b // r for b in bp]
            info = mx.insulation(k, windows, ignore_diags=1, min_frac_valid=0.5, min_strength=0.3)
            bins = mx.info(k)[0]
            lines = open(tmp_path / "b" / f"o.{r}.insulation.tsv", "rb").read().decode().splitlines()
            bed = open(tmp_path / "b" / f"o.{r}.bins.bed", "rb").read().decode().splitlines()
            assert lines[0].split("\t") == ["chrom", "start", "end"] + [f"{c}_{b}" for b in bp for c in ("n_valid", "score", "log2_insulation_score", "boundary_strength", "is_boundary")]
            assert len(lines) == 1 + bins == 1 + len(bed)
            rows = [x.split("\t") for x in lines[1:]]
            assert ["\t".join(x[:3]) for x in rows] == bed
            for j, b in enumerate(bp):
                assert stat[2 * k + j] == "\t".join(map(str, (r, b, bins, info.defined[j], info.minima[j], info.boundaries[j])))
                t = mx.insulation_track(k, j)
                col = lambda q: np.array([float(x[3 + 5 * j + q]) for x in rows])
                assert np.array_equal(col(0), t.n_valid.astype(np.float64)) and np.array_equal(col(4).astype(bool), t.boundary)
                assert all(x[3 + 5 * j + 4] in ("0", "1") for x in rows)
                for q, want in ((1, t.score), (2, t.log2_score), (3, t.strength)):      # %.17g round-trips
                    assert _same(col(q), want), (r, b, q)
            assert k or info.boundaries[0] > 0
