"""Pileups and aggregate peak analysis on the GPU (mkt_matrix_pileup, Matrix.pileup / pileup_loops / pileup_boundaries, pairs2matrix
--apa / --pileup) against the definition restated in tests/piledef.py, fed the GPU's own cells, weights and expected tables.  The
summation order is part of the definition, so there is no tolerance: n, csum, the statuses, the NaN pattern, vsum, mean and the seven
scores must be the same bytes.  Parity with juicer_tools apa and cooltools pileup is unpinned (neither is run)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import expected_inputs as xi
import insulation_inputs as ii
import loops_inputs as li
import microcket_amd as m
import piledef as pd
import pileup_inputs as pi
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
FIELDS = ("n", "csum", "vsum", "mean", "status")


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


class Ref:
    """the definition on the GPU's own cells, weights and tables of resolution index k (expected(k) has been called with use_weights)"""

    def __init__(self, mx, k, nb, off, ex, use_weights):
        self.b1, self.b2, self.cnt = (a.astype(np.int64) for a in mx.cells(k))
        self.nb, self.off = nb, off
        self.w = mx.weights(k) if use_weights else None
        self.valid = np.ones(nb, dtype=bool) if self.w is None else ~np.isnan(self.w)
        self.v = pd.cell_values(self.cnt, self.b1, self.b2, self.w)
        self.div = dict(balanced=None, oe=ex.genome.expected, oe_smooth=ex.genome.expected_smooth)
        self.key, self.feat, self.look = None, None, None

    def want(self, a, b, **opts):
        o = dict(pd.DEFAULTS)
        o.update(opts)
        st, lo, hi = pd.statuses(a, b, self.off, self.nb, o["flank"], o["edges"], o["min_dist"], o["max_dist"])
        key = (o["flank"], o["edges"], o["min_dist"], o["max_dist"])
        if key != self.key or self.feat is None or a is not self.feat[0] or b is not self.feat[1]:      # the lookup does not depend on kind and ignore_diags
            self.key, self.feat, self.look = key, (a, b), pd.lookup(self.b1, self.b2, self.nb, a, b, st, lo, hi, self.valid, o["flank"])
        kept, c, val = pd.values(self.look, self.cnt, self.v, self.div[o["kind"]], o["ignore_diags"])
        return pd.finish(*pd.chunked(kept, c, val), st, o["flank"], o["corner"])


def _bits(x):
    return struct.pack("<d", x)


def _compare(label, mx, k, info, want):
    got = mx.pileup_result(k)
    for f in FIELDS:
        assert getattr(got, f).dtype == getattr(want, f).dtype and getattr(got, f).tobytes() == getattr(want, f).tobytes(), (label, f)
    for s in pd.SCORES:
        assert _bits(getattr(info, s)) == _bits(want.scores[s]), (label, s, getattr(info, s), want.scores[s])
    st = want.status
    assert (info.features, info.used, info.trans, info.edge, info.dist) == (st.size, *[int((st == x).sum()) for x in (pd.USED, pd.TRANS, pd.EDGE, pd.DIST)]), label
    assert info.side == want.n.shape[0] and info.chunks == (st.size + 255) // 256
    return got


def _check(label, mx, k, ref, a, b, **opts):
    want = ref.want(a, b, **opts)
    return _compare(f"{label} {opts}", mx, k, mx.pileup(k, a, b, **opts), want), want


def _all_bytes(mx, k, a, b, **opts):
    info = mx.pileup(k, a, b, **opts)
    return b"".join([getattr(mx.pileup_result(k), f).tobytes() for f in FIELDS] + [_bits(getattr(info, s)) for s in pd.SCORES])


# ---- 1. chromosome starts, ends and neighbours; raw counts -------------------------------------------------------------------------
@pytest.mark.parametrize("flank", [1, 2, 5, 32])
def test_edges_raw_counts(flank):
    _need_gpu()
    ttext, text, off, nb, cells, _ = li.edge_matrix(False)
    a, b = pi.edge_features(False)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        assert (np.stack(mx.cells(0), axis=1) == cells).all()
        ref = Ref(mx, 0, nb, off, mx.expected(0, use_weights=False), False)
        for edges in (0, 1):
            for ig in (0, 2):
                for kind in pd.KINDS:
                    got, want = _check("edge", mx, 0, ref, a, b, flank=flank, corner=1, edges=edges, ignore_diags=ig, kind=kind)
                    if kind == "balanced":
                        assert np.array_equal(got.vsum, got.csum.astype(np.float64))          # raw counts: every value is its count
                assert got.csum.sum() > 0
            st = want.status
            first = np.flatnonzero((a < off[2]) & (st != pd.TRANS))              # the features of the one-bin and the 12-bin chromosome
            assert (st == pd.TRANS).sum() >= 3 and first.size > 50
            if edges == 0:
                assert (st[a == 0] != pd.USED).all() and (st[first] == pd.EDGE).sum() >= (first.size if flank > 5 else 10)
                assert (st == pd.USED).sum() >= 1                             # flank 32: the centre of the 65-bin chromosome alone
            else:
                assert not (st == pd.EDGE).any() and (st[first] == pd.USED).all()
                assert got.n.min() < got.n.max()                              # clipped positions


# ---- 2. masked bins --------------------------------------------------------------------------------------------------------------------
def test_masked_bins():
    _need_gpu()
    ttext, text, off, nb, cells, empty = li.edge_matrix(True)
    a, b = pi.edge_features(True)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        w = mx.weights(0)
        assert set(np.flatnonzero(np.isnan(w)).tolist()) == empty and len(empty) >= 5
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        raw = Ref(mx, 0, nb, off, mx.expected(0), True)
        raw.valid = np.ones(nb, dtype=bool)                                   # the same without a mask: what n would be
        for opts in (dict(flank=2, corner=2, edges=1, ignore_diags=0, kind="balanced"), dict(flank=5, corner=3, edges=0, kind="oe"), dict(flank=5, corner=3, edges=1)):
            got, want = _check("masked", mx, 0, ref, a, b, **opts)
            F, S = opts["flank"], 2 * opts["flank"] + 1
            full = raw.want(a, b, **opts)
            use = np.flatnonzero(want.status == pd.USED)
            em = np.array(sorted(empty))
            lost = np.zeros((S, S), dtype=np.uint64)                          # per position: the used features with a masked row or column there
            for p in range(-F, F + 1):
                for q in range(-F, F + 1):
                    i, j = a[use] + p, b[use] + q
                    kept = raw.look.inside[use, (p + F) * S + (q + F)] & (np.abs(j - i) >= want_ig(opts))
                    lost[p + F][q + F] = int((kept & (np.isin(i, em) | np.isin(j, em))).sum())
            assert np.array_equal(full.n - got.n, lost) and lost.sum() > 100, opts


def want_ig(opts):
    return opts.get("ignore_diags", pd.DEFAULTS["ignore_diags"])


# ---- 3. chunk and batch boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 512, 513, 4096 * 256 + 257])
def test_chunk_and_batch_boundaries(n):
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    opts = dict(flank=1, corner=1, min_dist=pi.BAND_MIN_DIST, kind="oe")
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1)
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        for holes, empty_chunk in ((False, False), (True, False), (True, True)):
            if (empty_chunk and n < 512) or (not empty_chunk and n > 100000):      # the batch boundary: the fullest variant alone
                continue
            a, b = pi.band_features(n, holes, empty_chunk)
            got, want = _check(f"band n={n}", mx, 0, ref, a, b, **opts)
            assert (want.status != pd.USED).any() and (want.status == pd.USED).any() or n == 1
            if holes:
                assert want.status[0] == pd.DIST and (n <= 255 or want.status[255] == pd.DIST) and (n <= 256 or want.status[256] == pd.DIST)
            if empty_chunk:
                assert (want.status[256:512] == pd.DIST).all()
            # the features that are not used keep their slots: taking them out moves the others to other chunks, and the definition says
            # what that does to the bits; the integers do not change
            a2, b2 = pi.without(a, b, want.status)
            got2, want2 = _check(f"band n={n} without", mx, 0, ref, a2, b2, **opts)
            assert np.array_equal(got2.n, got.n) and np.array_equal(got2.csum, got.csum)
            assert np.array_equal(got2.vsum == got.vsum, want2.vsum == want.vsum)
        s, t = mx.pileup_timing_ms(0)
        assert s >= 0 and (t > 0 or n == 1)                                   # n = 1: the last call had no feature left, so no batch


# ---- 4. the mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    (da, db), (oa, ob) = pi.mirror_features()
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1)
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        for opts in (dict(flank=3, corner=2, ignore_diags=0, kind="balanced"), dict(flank=10, corner=6), dict(flank=32, corner=8, kind="oe", ignore_diags=1, edges=1)):
            got, _ = _check("diagonal", mx, 0, ref, da, db, **opts)
            for f in ("n", "csum", "vsum", "mean"):                           # on-diagonal features: the transpose, bit for bit
                x = getattr(got, f)
                assert x.tobytes() == np.ascontiguousarray(x.T).tobytes() and (f != "csum" or x.sum() > 0), (opts, f)
            got, want = _check("near the diagonal", mx, 0, ref, oa, ob, **opts)
            assert 1 <= (ob - oa).min() and (ob - oa).max() < 5 and (want.status == pd.USED).all() and got.csum.sum() > 0


# ---- 5. APA on planted loops, boundaries of planted domains -----------------------------------------------------------------------------------
def test_apa_on_planted_loops():
    _need_gpu()
    text, cells, pixels = li.planted()
    off, nb = xi.offsets(250000)
    a, b = pi.planted_features()
    with _loaded(text, [250000], xi.TABLE) as mx:
        mx.balance(0)
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        got, want = _check("planted", mx, 0, ref, a, b)
        assert want.scores["peak"] == np.nanmax(want.mean) == want.mean[10][10] and want.scores["p2ll"] > 1      # the condition of test_pileup_host
        loops = mx.loops(0, **li.STAT_OPTS).loops
        assert len(loops) >= 10
        la, lb = np.array([l.bin1 for l in loops]), np.array([l.bin2 for l in loops])
        for opts in (dict(), dict(flank=5, corner=2, kind="oe", edges=1)):
            direct = _all_bytes(mx, 0, la, lb, **opts)
            info = mx.pileup_loops(0, **opts)
            assert b"".join([getattr(mx.pileup_result(0), f).tobytes() for f in FIELDS] + [_bits(getattr(info, s)) for s in pd.SCORES]) == direct
            assert info.features == len(loops) and info.p2ll > 1
        _check("loops", mx, 0, ref, la, lb)
    ttext, text, off, nb, cells, edges = ii.planted()
    with _loaded(text, [ii.R], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0)
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        mx.insulation(0, (5, 10))
        bins = np.flatnonzero(mx.insulation_track(0, 0).boundary)
        assert ii.boundaries_are_the_planted(mx.insulation_track(0, 0).boundary, edges)
        direct = _all_bytes(mx, 0, bins, bins, flank=6, corner=3)
        info = mx.pileup_boundaries(0, 0, flank=6, corner=3)
        assert b"".join([getattr(mx.pileup_result(0), f).tobytes() for f in FIELDS] + [_bits(getattr(info, s)) for s in pd.SCORES]) == direct
        got, want = _check("boundaries", mx, 0, ref, bins, bins.copy(), flank=6, corner=3)
        assert info.features == bins.size and want.mean[3][9] < want.mean[2][5]      # (-3, +3) lies across the boundary, (-4, -1) inside the domain before it


# ---- 6. the same bits on a second call, in another object and by another route ---------------------------------------------------------
def test_same_bits_by_every_route():
    _need_gpu()
    ttext, text, off, nb, cells, edges = ii.planted()
    a = np.arange(3, nb - 3, 2)
    b = np.minimum(a + np.arange(a.size) % 9, nb - 1)
    opts = dict(flank=4, corner=2, edges=1)
    with _loaded(text, [ii.R], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0)
        mx.expected(0)
        first = _all_bytes(mx, 0, a, b, **opts)
        assert _all_bytes(mx, 0, a, b, **opts) == first
    lines = text.splitlines(keepends=True)
    other = b"".join(lines[i] for i in np.random.default_rng(4).permutation(len(lines)).tolist())
    with m.Matrix(ttext, [ii.R], device=0) as mx:
        for at in range(0, len(other), 100_003):                              # chunks that end inside a line
            mx.add(other[at:at + 100_003])
        mx.run()
        mx.balance(0, min_nnz=1, mad_max=0)
        mx.expected(0)
        assert _all_bytes(mx, 0, a, b, **opts) == first
    # the add_keys route against the text route
    c = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
    try:
        p = c.run_bytes(util.synth("unc", 61, 20000), chunk=1 << 20)[0]
        with m.Matrix(xi.TABLE, [2500000]) as x, _loaded(p, [2500000], xi.TABLE) as y:
            x.add_keys(c, True, None)
            x.run()
            assert x.info(0)[1] == y.info(0)[1] > 0
            ca, cb, _ = x.cells(0)
            o = dict(flank=2, corner=1, edges=1, ignore_diags=1, kind="oe")
            x.expected(0, use_weights=False)
            y.expected(0, use_weights=False)
            assert _all_bytes(x, 0, ca, cb, **o) == _all_bytes(y, 0, ca, cb, **o)
            assert x.pileup_result(0).csum.sum() > 0
    finally:
        c.close()


# ---- 7. state, argument and discard errors -------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    a, b = pi.band_features(300)
    with m.Matrix(ttext, [li.R_EDGE, 5 * li.R_EDGE]) as mx:
        with pytest.raises(m.MktError, match="pileup before run"):
            mx.pileup(0, a, b)
        mx.add(text)
        mx.run()
        with pytest.raises(m.MktError, match="expected first"):
            mx.pileup(0, a, b)
        with pytest.raises(m.MktError, match="pileup first"):
            mx.pileup_result(0)
        assert mx.pileup_timing_ms(0) == (0.0, 0.0)
        mx.balance(0, min_nnz=1)
        ex = mx.expected(0)
        ref = Ref(mx, 0, nb, off, ex, True)
        info = mx.pileup(0, a, b, min_dist=pi.BAND_MIN_DIST)
        kept = b"".join(getattr(mx.pileup_result(0), f).tobytes() for f in FIELDS)
        with pytest.raises(m.MktError, match="expected first"):
            mx.pileup(1, a, b)                                                # the other resolution has no tables
        with pytest.raises(m.MktError, match="resolution index"):
            mx.pileup(2, a, b)
        for bad, what in ((dict(flank=0), "flank 0"), (dict(flank=33), "flank 33"), (dict(corner=0), "corner 0"), (dict(flank=4, corner=5), "corner 5"), (dict(kind=3), "kind 3"),
                          (dict(kind=-1), "kind -1"), (dict(ignore_diags=-1), "ignore_diags"), (dict(min_dist=-1), "min_dist"), (dict(max_dist=-2), "max_dist"),
                          (dict(edges=2), "edges 2"), (dict(edges=-1), "edges -1"), (dict(min_dist=5, max_dist=4), "max_dist 4 is below min_dist 5")):
            with pytest.raises(m.MktError, match=what):
                mx.pileup(0, a, b, **bad)
        with pytest.raises(TypeError):
            mx.pileup(0, a, b, window=3)
        with pytest.raises(ValueError):
            mx.pileup(0, a, b, kind="raw")
        for fa, fb, what in (([5, 9], [7, 8], r"feature 1 \(9, 8\)"), ([5], [nb], rf"feature 0 \(5, {nb}\)"), ([1, 2, nb + 3], [1, 2, nb + 4], "feature 2")):
            with pytest.raises(m.MktError, match=what):
                mx.pileup(0, fa, fb)
        o = m.PileupOpts()
        mx.L.mkt_pileup_opts_default(C.byref(o))
        assert (o.flank, o.corner, o.kind, o.ignore_diags, o.edges, o.min_dist, o.max_dist, o.reserved) == (10, 6, 2, 2, 0, 0, 0, 0)
        o.reserved = 3
        ua, ub = a.astype(np.uint32), b.astype(np.uint32)
        pa, pb = ua.ctypes.data_as(C.c_void_p), ub.ctypes.data_as(C.c_void_p)
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_pileup(mx.h, 0, pa, pb, ua.size, C.byref(o), None), "pileup")
        with pytest.raises(m.MktError, match="NULL"):
            mx._chk(mx.L.mkt_matrix_pileup(mx.h, 0, None, pb, ua.size, None, None), "pileup")
        with pytest.raises(m.MktError, match="2\\^32"):
            mx._chk(mx.L.mkt_matrix_pileup(mx.h, 0, pa, pb, 1 << 32, None, None), "pileup")
        assert b"".join(getattr(mx.pileup_result(0), f).tobytes() for f in FIELDS) == kept      # a refused call leaves the results alone
        with pytest.raises(m.MktError, match="pileup features"):
            mx._chk(mx.L.mkt_matrix_fetch_pileup_status(mx.h, 0, 299, 2, None), "fetch")
        one = (C.c_uint8 * 2)()
        mx._chk(mx.L.mkt_matrix_fetch_pileup_status(mx.h, 0, 298, 2, one), "fetch")
        assert list(one) == mx.pileup_result(0).status[-2:].tolist()
        mx._chk(mx.L.mkt_matrix_fetch_pileup(mx.h, 0, None, None, None, None), "fetch")       # any pointer may be NULL
        mx._chk(mx.L.mkt_matrix_fetch_pileup_status(mx.h, 0, 300, 0, None), "fetch")
        from microcket_amd.capi import _PileupInfoC
        ic = _PileupInfoC()
        mx._chk(mx.L.mkt_matrix_pileup(mx.h, 0, pa, pb, ua.size, None, C.byref(ic)), "pileup")     # NULL options: the defaults
        want = ref.want(a, b)
        assert (ic.side, ic.features, ic.used) == (21, 300, int((want.status == pd.USED).sum())) and _bits(ic.peak) == _bits(want.scores["peak"])
        mx._chk(mx.L.mkt_matrix_pileup(mx.h, 0, pa, pb, ua.size, None, None), "pileup")            # ... and no info
        assert mx.L.mkt_abi_version() == 9
        # no feature at all
        info = mx.pileup(0, [], [])
        r = mx.pileup_result(0)
        assert (info.features, info.used, info.chunks, info.side) == (0, 0, 0, 21) and not r.n.any() and not r.csum.any() and not r.vsum.any()
        assert np.isnan(r.mean).all() and r.status.size == 0 and all(_bits(getattr(info, s)) == _bits(float("nan")) for s in pd.SCORES)
        _compare("none", mx, 0, info, ref.want(np.zeros(0, np.int64), np.zeros(0, np.int64)))
        # loops, eigs, insulation and pileup of one resolution do not disturb each other
        pile_bytes = lambda: b"".join(getattr(mx.pileup_result(0), f).tobytes() for f in FIELDS)

        def other_bytes():
            v = np.zeros((2, nb), np.float64)
            for j in range(2):
                mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, j, 0, nb, v[j].ctypes.data_as(C.c_void_p)), "fetch")
            return b"".join([x.tobytes() for x in mx.loop_cells(0)] + [mx.loop_hist(0).tobytes(), v.tobytes(), mx.values(0, "oe").tobytes()] +
                            [getattr(mx.insulation_track(0, j), f).tobytes() for j in range(3) for f in m.InsulationTrack._fields])
        mx.pileup(0, a, b, min_dist=pi.BAND_MIN_DIST)
        assert pile_bytes() == kept
        mx.loops(0)
        mx.eigs(0, n_eigs=2)
        mx.insulation(0)
        assert pile_bytes() == kept                                           # ... by loops, eigenvectors and insulation scores
        others = other_bytes()
        mx.pileup(0, a, b, flank=3, corner=1, kind="balanced")
        assert other_bytes() == others                                        # ... and those not by a pileup
        # a later balance, expected, run or add of that resolution discards the results
        line = text.splitlines(keepends=True)[0]
        for what, again in (("balance", lambda: mx.balance(0, min_nnz=1)), ("expected", lambda: mx.expected(0, use_weights=False)), ("run", lambda: mx.run()), ("add", lambda: mx.add(line))):
            mx.run()
            mx.balance(0, min_nnz=1)
            mx.expected(0)
            assert mx.pileup(0, a, b).used > 200 and mx.pileup_timing_ms(0)[1] > 0
            again()
            with pytest.raises(m.MktError, match="pileup first"):
                mx.pileup_result(0)
            assert mx.pileup_timing_ms(0) == (0.0, 0.0), what


# ---- 8. the executable ---------------------------------------------------------------------------------------------------------------------------
def test_executable_writes_the_pileups(tmp_path):
    _need_gpu()
    text, cells, pixels = li.planted()
    off, nb = xi.offsets(250000)
    (tmp_path / "g.sizes").write_bytes(xi.TABLE)
    (tmp_path / "in.pairs").write_bytes(text)
    names = [n for n, _ in xi.HG38]
    offa = np.asarray(off)
    rows = []
    for x, y in pixels[250000][:12]:
        c = int(np.searchsorted(offa, x, side="right")) - 1
        s1, s2 = (x - off[c]) * 250000, (y - off[c]) * 250000
        rows.append((names[c], s1 + 100, s1 + 200_100, names[c], s2, s2 + 250_000))
    rows[3] = rows[3][3:] + rows[3][:3]                                       # the larger bin first: swapped
    rows.append((names[0], 0, 1000, names[1], 0, 1000))                       # a trans pair
    bedpe = "# planted\n\n" + "".join("\t".join(map(str, r)) + "\tx\n" for r in rows)
    (tmp_path / "f.bedpe").write_bytes(bedpe.encode())
    for d in "ab":
        os.makedirs(tmp_path / d)
    run = lambda d, *a: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", "250000", "-o", str(tmp_path / d / "o"), "--loops", "--loop-max-dist", "48", *a, str(tmp_path / "in.pairs")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    sub = ["--pile-flank", "5", "--pile-corner", "2", "--pile-kind", "oe", "--pile-edges"]
    runs = [run("a"), run("b", "--apa", "--pileup", str(tmp_path / "f.bedpe"), *sub)]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted(os.listdir(tmp_path / "a"))
    assert "o.250000.loops.bedpe" in plain and not any("apa" in f or "pileup" in f for f in plain)      # without the flags no new file appears ...
    assert sorted(os.listdir(tmp_path / "b")) == sorted(plain + ["o.250000.apa.tsv", "o.apa.stat", "o.250000.pileup.tsv", "o.pileup.stat"])
    for f in plain:                                                           # ... and the flags change none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    num = lambda s: float(s)                                                  # "nan" round-trips through float()
    with _loaded(text, [250000], xi.TABLE) as mx:
        mx.expected(0, use_weights=False)
        mx.loops(0, **li.STAT_OPTS)
        o = dict(flank=5, corner=2, kind="oe", edges=1)
        fa = [min(off[names.index(r[0])] + ((r[1] + r[2]) // 2) // 250000, off[names.index(r[3])] + ((r[4] + r[5]) // 2) // 250000) for r in rows]
        fb = [max(off[names.index(r[0])] + ((r[1] + r[2]) // 2) // 250000, off[names.index(r[3])] + ((r[4] + r[5]) // 2) // 250000) for r in rows]
        assert list(zip(fa[:12], fb[:12])) == [tuple(p) for p in pixels[250000][:12]]
        for what, call in (("apa", lambda: mx.pileup_loops(0, **o)), ("pileup", lambda: mx.pileup(0, fa, fb, **o))):
            info = call()
            res = mx.pileup_result(0)
            lines = open(tmp_path / "b" / f"o.250000.{what}.tsv", "rb").read().decode().splitlines()
            assert lines[0].split("\t") == ["p", "q", "n", "csum", "vsum", "mean"] and len(lines) == 1 + 121
            t = [x.split("\t") for x in lines[1:]]
            assert [(int(x[0]), int(x[1])) for x in t] == [(p, q) for p in range(-5, 6) for q in range(-5, 6)]
            assert [int(x[2]) for x in t] == res.n.ravel().tolist() and [int(x[3]) for x in t] == res.csum.ravel().tolist()
            for col, arr in ((4, res.vsum), (5, res.mean)):                   # %.17g round-trips
                assert np.array([num(x[col]) for x in t]).tobytes() == arr.ravel().tobytes(), (what, col)
            stat = open(tmp_path / "b" / f"o.{what}.stat", "rb").read().decode().splitlines()
            assert len(stat) == 1
            f = stat[0].split("\t")
            assert [int(x) for x in f[:6]] == [250000, info.features, info.used, info.trans, info.edge, info.dist]
            assert b"".join(_bits(num(x)) for x in f[6:]) == b"".join(_bits(getattr(info, s)) for s in pd.SCORES)
            assert info.used >= 12 and info.p2ll > 1 and (what == "apa" or info.trans == 1)
