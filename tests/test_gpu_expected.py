"""Expected tables and observed / expected values on the GPU (mkt_matrix_expected, Matrix.expected / values, pairs2matrix --expected)
against the definition restated in tests/expecteddef.py, fed the GPU's own weights.  Integers (n_valid, count_sum, table sizes) and
the NaN pattern must be identical; float64 sums agree to the bound of reordering a sum of T positive terms, T x 2^-52 relative (derived
from the input, not tuned); repeated calls, another process and another route of the same pairs give the same bits.  Parity with
cooltools and juicer is unpinned (neither is run)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import balancedef as bd
import expected_inputs as xi
import expecteddef as ed
import matrixdef as md
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
RES = (2500000, 500000, 100000)
# At 100 kb the longest chromosome has 2490 bins, so no (chromosome, diagonal) segment of RES can hold 4096 cells: 25 kb is added to
# the three resolutions for that condition (chr1: 9959 bins), and 50 kb so that every lane width of the sums is taken.
RES_LONG = RES + (50000, 25000)
SEED = 21
U = 2.0 ** -52


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _loaded(text, res, table=xi.TABLE):
    mx = m.Matrix(table, list(res), device=0)
    mx.add(text)
    mx.run()
    return mx


def _rel(got, want):
    """largest |got / want - 1| over want != 0; where want is 0 or NaN, got must be the same"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert (np.isnan(got) == np.isnan(want)).all()
    z = want == 0
    assert (got[z] == 0).all()
    ok = ~z & ~np.isnan(want)
    return np.abs(got[ok] / want[ok] - 1.0), ok


def _check(label, got, want, bound):
    dev, ok = _rel(got, want)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(want))[ok]
    worst = int(np.argmax(dev - b)) if dev.size else -1
    print(f"{label}: max rel dev {dev.max() if dev.size else 0.0:.3e}; closest to its bound: dev {dev[worst] if dev.size else 0.0:.3e} bound {b[worst] if dev.size else 0.0:.3e}")
    assert (dev <= b).all(), (label, float(dev[worst]), float(b[worst]))


def _compare(label, got, vals, want, nbins, off):
    """got: Matrix.expected(), vals: {kind: Matrix.values()}, want: expecteddef.Result of the same cells and weights"""
    nchr = len(off)
    assert got.n_chrom == nchr and got.smooth_groups == want.smooth_groups
    for g, w in ((got.cis, want.cis), (got.trans, want.trans), (got.genome, want.genome)):
        assert g.n_valid.dtype == np.uint64 and g.count_sum.dtype == np.uint64 and g.balanced_sum.dtype == np.float64
        assert g.n_valid.shape == w.n_valid.shape and (g.n_valid == w.n_valid).all(), label
        assert g.count_sum.shape == w.count_sum.shape and (g.count_sum == w.count_sum).all(), label
    assert got.cis.n_valid.size == nbins and got.trans.n_valid.size == nchr * (nchr - 1) // 2
    n_c = np.diff(np.append(np.asarray(off), nbins))
    assert got.genome.n_valid.size == n_c.max()
    for a, b in ((got.trans.expected, want.trans.expected), (got.genome.expected, want.genome.expected), (got.genome.expected_smooth, want.genome.expected_smooth),
                 (vals["balanced"], want.balanced), (vals["oe"], want.oe), (vals["oe_smooth"], want.oe_smooth)):
        assert a.shape == b.shape and (np.isnan(a) == np.isnan(b)).all(), label
    assert np.isfinite(vals["oe"][want.used]).all() and np.isfinite(vals["oe_smooth"][want.used]).all()
    assert np.array_equal(vals["balanced"], want.balanced, equal_nan=True)      # two multiplications in a fixed order: exact
    T = want.seg_cells.astype(np.float64)
    _check(f"{label} cis balanced_sum", got.cis.balanced_sum, want.cis.balanced_sum, T[:nbins] * U)
    _check(f"{label} trans balanced_sum", got.trans.balanced_sum, want.trans.balanced_sum, T[nbins:] * U)
    _check(f"{label} trans expected", got.trans.expected, want.trans.expected, (T[nbins:] + 1) * U)
    Tg = np.zeros(n_c.max())
    for c in range(nchr):
        Tg[:n_c[c]] += T[off[c]:off[c] + n_c[c]]
    _check(f"{label} genome balanced_sum", got.genome.balanced_sum, want.genome.balanced_sum, (Tg + nchr) * U)
    _check(f"{label} genome expected", got.genome.expected, want.genome.expected, (Tg + nchr) * U)
    edges = ed.smooth_edges(Tg.size)
    Ts = np.zeros(Tg.size)
    for a, b in zip(edges[:-1], edges[1:]):
        Ts[a:b] = Tg[a:b].sum()
    _check(f"{label} genome expected_smooth", got.genome.expected_smooth, want.genome.expected_smooth, (Ts + nchr) * U)
    # values: the bound of their divisor + 2^-51
    seg = want.seg
    cis = seg < nbins
    chrom = np.searchsorted(np.asarray(off), np.arange(nbins), side="right") - 1
    d = np.where(cis, seg - np.asarray(off)[chrom[np.minimum(seg, nbins - 1)]], 0)
    tb = T[np.where(cis, nbins, seg)] if T.size > nbins else np.zeros(seg.size)
    _check(f"{label} oe", vals["oe"], want.oe, np.where(cis, Tg[d] + nchr, tb + 1) * U + 2 * U)
    _check(f"{label} oe_smooth", vals["oe_smooth"], want.oe_smooth, np.where(cis, Ts[d] + nchr, tb + 1) * U + 2 * U)


def _all_bytes(mx, k, use_weights):
    e = mx.expected(k, use_weights=use_weights)
    parts = [a.tobytes() for t in (e.cis, e.trans, e.genome) for a in t] + [mx.values(k, kind).tobytes() for kind in ("balanced", "oe", "oe_smooth")]
    return b"".join(parts)


# ---- 1. chromosome offsets that are not word-aligned, bins without a contact at every edge of the validity bits ------------------
def test_edge_table_exact():
    _need_gpu()
    nb_c = [1, 63, 64, 65, 130, 1]
    r = 1000
    table = [(f"c{i}", n * r if i < 5 else 500) for i, n in enumerate(nb_c)]
    ttext = "".join(f"{n}\t{l}\n" for n, l in table).encode()
    off, nb = xi.offsets(r, [(n.encode(), l) for n, l in table])
    assert off == [0, 1, 64, 128, 193, 323] and nb == 324
    empty = {off[2], off[3] + 64, off[4] + 63, off[4] + 64, off[5]}       # first bin of c2, last bin of c3, bins 63 and 64 of c4, all of c5
    live = np.array([k for k in range(nb) if k not in empty])
    rng = np.random.default_rng(8)
    a = np.concatenate([live, live, rng.choice(live, 3000)])
    b = np.concatenate([live, rng.choice(live, live.size), rng.choice(live, 3000)])
    chrom = np.searchsorted(off, np.arange(nb), side="right") - 1
    names = [n for n, _ in table]
    text = "".join(f"q\t{names[chrom[x]]}\t{(x - off[chrom[x]]) * r + 7}\t{names[chrom[y]]}\t{(y - off[chrom[y]]) * r + 9}\t+\t-\n" for x, y in zip(a.tolist(), b.tolist())).encode()
    cells = md.definition(ttext, [r], text)[r][0]
    assert not (set(cells[:, 0].tolist()) | set(cells[:, 1].tolist())) & empty
    with _loaded(text, [r], ttext) as mx:
        b1, b2, c = mx.cells(0)
        assert (np.stack([b1, b2, c], axis=1) == cells).all()
        mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        w = mx.weights(0)
        assert set(np.flatnonzero(np.isnan(w)).tolist()) == empty
        for uw in (1, 0):
            want = ed.expected(b1, b2, c, nb, off, weights=w if uw else None)
            got = mx.expected(0, use_weights=bool(uw))
            vals = {k: mx.values(0, k) for k in ("balanced", "oe", "oe_smooth")}
            _compare(f"edge use_weights={uw}", got, vals, want, nb, off)
            if uw:
                assert got.cis.n_valid[off[5]] == 0 and got.trans.n_valid[-1] == 0 and np.isnan(got.trans.expected[-1])
                assert got.cis.n_valid[off[4]] == 128 and got.cis.n_valid[off[4] + 1] == 126 and got.cis.n_valid[off[4] + 64] == 63
            else:
                assert (got.cis.n_valid == np.concatenate([np.arange(n, 0, -1) for n in nb_c])).all() and vals["balanced"].tolist() == c.astype(np.float64).tolist()


def _width(nnz, nseg):
    """the sums' lanes per segment, as mkt_expected.hip picks them from the cells a segment holds on average"""
    avg = nnz // nseg
    return 64 if avg >= 48 else 32 if avg >= 24 else 16 if avg >= 12 else 8


# ---- 2. hg38, drawn pairs, the default balance -----------------------------------------------------------------------------------
def test_hg38_against_the_definition():
    _need_gpu()
    text, cells, n = xi.drawn(3_000_000, SEED, RES_LONG)
    # conditions on the input, asked of the checker alone
    pre = {}
    for r in RES_LONG:
        off, nb = xi.offsets(r)
        c = cells[r]
        wdef = bd.balance(c[:, 0], c[:, 1], c[:, 2], nb, off).weights
        pre[r] = (int(np.isnan(wdef).sum()), ed.expected(c[:, 0], c[:, 1], c[:, 2], nb, off, weights=wdef).seg_cells, ed.expected(c[:, 0], c[:, 1], c[:, 2], nb, off).seg_cells, nb)
    assert 0 < pre[100000][0] < pre[100000][3]                              # masked bins exist at 100 kb
    assert max(int(pre[r][1][pre[r][3]:].max()) for r in RES) >= 4096        # the longest trans segment, with the weights
    assert int(pre[25000][2][:pre[25000][3]].max()) >= 4096                  # the longest cis segment (raw, 25 kb: see RES_LONG)
    assert int(pre[100000][1][:pre[100000][3]].max()) > 1024                 # ... and at 100 kb a cis segment is cut into chunks as well
    nchr = len(xi.HG38)
    widths = [_width(cells[r].shape[0], pre[r][3] + nchr * (nchr - 1) // 2) for r in RES_LONG]
    assert set(widths) == {64, 32, 16, 8}, widths                            # one resolution per compiled variant of the sums at least
    with _loaded(text, RES_LONG) as mx:
        for k, r in enumerate(RES_LONG):
            off, nb = xi.offsets(r)
            b1, b2, c = mx.cells(k)
            assert (np.stack([b1, b2, c], axis=1) == cells[r]).all()
            mx.balance(k)
            w = mx.weights(k)
            for uw in (1, 0):
                want = ed.expected(b1, b2, c, nb, off, weights=w if uw else None)
                got = mx.expected(k, use_weights=bool(uw))
                vals = {kind: mx.values(k, kind) for kind in ("balanced", "oe", "oe_smooth")}
                _compare(f"r={r} use_weights={uw}", got, vals, want, nb, off)
                setup_ms, sums_ms = mx.expected_timing_ms(k)
                assert sums_ms > 0 and (setup_ms > 0) == (uw == 1)           # the grouping is made once and reused
            # the property: observed / expected of the used cis cells of a diagonal add up to its n_valid
            chrom = np.searchsorted(np.asarray(off), np.arange(nb), side="right") - 1
            sel = (chrom[b1] == chrom[b2]) & ~np.isnan(vals["oe"])
            tot = np.bincount((b2 - b1)[sel], weights=vals["oe"][sel], minlength=got.genome.n_valid.size)
            has = np.bincount((b2 - b1)[sel], minlength=tot.size) > 0
            assert np.abs(tot[has] / got.genome.n_valid[has] - 1.0).max() < 1e-9


# ---- 3. the same bits on a second call, in another process, by another chunking and order, and from a context's keys -------------
def test_same_bits_by_every_route(tmp_path):
    _need_gpu()
    text = xi.drawn(3_000_000, SEED, RES_LONG)[0]
    res = RES[1:]
    first = {}
    with _loaded(text, res) as mx:
        for k in range(len(res)):
            mx.balance(k)
            first[k, 1] = _all_bytes(mx, k, True)
            assert _all_bytes(mx, k, True) == first[k, 1]
            first[k, 0] = _all_bytes(mx, k, False)
            mx.balance(k)
            assert _all_bytes(mx, k, True) == first[k, 1]
    lines = text.splitlines(keepends=True)
    order = np.random.default_rng(4).permutation(len(lines))
    other = b"".join(lines[i] for i in order.tolist())
    with m.Matrix(xi.TABLE, list(res), device=0) as mx:
        for at in range(0, len(other), 7_000_003):                            # chunks that end inside a line
            mx.add(other[at:at + 7_000_003])
        mx.run()
        for k in range(len(res)):
            assert _all_bytes(mx, k, False) == first[k, 0]
            mx.balance(k)
            assert _all_bytes(mx, k, True) == first[k, 1]
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(text)
    (tmp_path / "g.sizes").write_bytes(xi.TABLE)
    script = ("import sys, microcket_amd as m\n"
              "mx = m.Matrix(open(sys.argv[1], 'rb').read(), [int(x) for x in sys.argv[3].split(',')])\n"
              "mx.add(open(sys.argv[2], 'rb').read()); mx.run()\n"
              "for k in range(len(mx.resolutions)):\n"
              "    mx.balance(k); e = mx.expected(k)\n"
              "    parts = [a.tobytes() for t in (e.cis, e.trans, e.genome) for a in t] + [mx.values(k, kind).tobytes() for kind in ('balanced', 'oe', 'oe_smooth')]\n"
              "    open(sys.argv[4] + '.%d' % k, 'wb').write(b''.join(parts))\n"
              "mx.close()\n")
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "g.sizes"), str(pairs), ",".join(map(str, res)), str(tmp_path / "e")], env=env, cwd=util.ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    for k in range(len(res)):
        assert open(f"{tmp_path}/e.{k}", "rb").read() == first[k, 1]
    # the add_keys route against the text route
    c = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
    try:
        p = c.run_bytes(util.synth("unc", 61, 20000), chunk=1 << 20)[0]
        with m.Matrix(xi.TABLE, [2500000, 500000]) as a, _loaded(p, [2500000, 500000]) as b:
            a.add_keys(c, True, None)
            a.run()
            for k in range(2):
                assert a.info(k)[1] == b.info(k)[1] > 0
                assert _all_bytes(a, k, False) == _all_bytes(b, k, False)
                a.balance(k, min_nnz=2, ignore_diags=1), b.balance(k, min_nnz=2, ignore_diags=1)
                assert _all_bytes(a, k, True) == _all_bytes(b, k, True)
    finally:
        c.close()


# ---- 4. the state and argument errors -------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    import ctypes as C
    text = xi.drawn(3_000_000, SEED, RES_LONG)[0][:400000].rsplit(b"\n", 1)[0] + b"\n"
    with m.Matrix(xi.TABLE, [2500000, 500000]) as mx:
        with pytest.raises(m.MktError, match="expected before run"):
            mx.expected(0, use_weights=False)
        mx.add(text)
        mx.run()
        nb, nnz, _ = mx.info(0)
        for kind in ("balanced", "oe", "oe_smooth"):                          # a fetch before expected (and before balance)
            with pytest.raises(m.MktError, match="expected first|balance first"):
                mx.values(0, kind)
        buf = (C.c_uint64 * 4)()
        fetches = ((mx.L.mkt_matrix_fetch_expected_cis, 2), (mx.L.mkt_matrix_fetch_expected_trans, 3), (mx.L.mkt_matrix_fetch_expected_genome, 4))
        for fn, nulls in fetches:
            with pytest.raises(m.MktError, match="expected first"):
                mx._chk(fn(mx.h, 0, 0, 1, buf, *[None] * nulls), "fetch")
        with pytest.raises(m.MktError, match="balance first"):
            mx.expected(0)                                                    # use_weights = 1 before balance
        e0 = mx.expected(0, use_weights=False)                                # raw needs no weights
        assert mx.values(0, "balanced").tolist() == mx.cells(0)[2].astype(np.float64).tolist()
        assert int(e0.cis.count_sum.sum() + e0.trans.count_sum.sum()) == int(mx.cells(0)[2].sum())
        with pytest.raises(m.MktError, match="expected first"):
            mx.values(1, "oe")                                                # the other resolution has no tables
        mx.balance(0)                                                         # a balance discards the tables ...
        with pytest.raises(m.MktError, match="expected first"):
            mx.values(0, "oe")
        w = mx.weights(0)
        b1, b2, c = mx.cells(0)
        assert np.array_equal(mx.values(0, "balanced"), (c.astype(np.float64) * w[b1]) * w[b2], equal_nan=True)   # ... BALANCED needs only the weights
        mx.expected(0)
        assert mx.values(0, "oe").size == nnz
        # bad kind, ranges, index, reserved, use_weights
        out = (C.c_double * 8)()
        with pytest.raises(m.MktError, match="kind 3"):
            mx._chk(mx.L.mkt_matrix_fetch_values(mx.h, 0, 3, 0, 1, out), "values")
        with pytest.raises(m.MktError, match="kind -1"):
            mx._chk(mx.L.mkt_matrix_fetch_values(mx.h, 0, -1, 0, 1, out), "values")
        with pytest.raises(ValueError):
            mx.values(0, "observed")
        with pytest.raises(m.MktError, match="values of cells"):
            mx._chk(mx.L.mkt_matrix_fetch_values(mx.h, 0, 1, nnz - 2, 4, out), "values")
        mx._chk(mx.L.mkt_matrix_fetch_values(mx.h, 0, 1, nnz - 4, 4, out), "values")
        assert np.array_equal(np.array(list(out)[:4]), mx.values(0, "oe")[-4:], equal_nan=True)
        nchr = len(xi.HG38)
        for (fn, nulls), rows, what in zip(fetches, (nb, nchr * (nchr - 1) // 2, e0.genome.n_valid.size), ("cis rows", "trans rows", "genome rows")):
            with pytest.raises(m.MktError, match=what):
                mx._chk(fn(mx.h, 0, rows - 2, 4, buf, *[None] * nulls), "fetch")
            mx._chk(fn(mx.h, 0, rows - 4, 4, buf, *[None] * nulls), "fetch")  # any output pointer may be NULL
            mx._chk(fn(mx.h, 0, rows, 0, None, *[None] * nulls), "fetch")
        with pytest.raises(m.MktError, match="resolution index"):
            mx.expected(2)
        with pytest.raises(m.MktError, match="resolution index"):
            mx.values(2, "oe")
        o = m.ExpectedOpts(use_weights=1, reserved=5)
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_expected(mx.h, 0, C.byref(o), None), "expected")
        o = m.ExpectedOpts(use_weights=2, reserved=0)
        with pytest.raises(m.MktError, match="use_weights"):
            mx._chk(mx.L.mkt_matrix_expected(mx.h, 0, C.byref(o), None), "expected")
        assert mx.values(0, "oe").size == nnz                                 # a refused call leaves the tables alone
        mx._chk(mx.L.mkt_matrix_expected(mx.h, 0, None, None), "expected")   # NULL options: the defaults
        mx.run()                                                              # a new run discards everything
        with pytest.raises(m.MktError, match="expected first|balance first"):
            mx.values(0, "balanced")
        with pytest.raises(m.MktError, match="expected first"):
            mx._chk(mx.L.mkt_matrix_fetch_expected_cis(mx.h, 0, 0, 1, buf, None, None), "fetch")
        assert mx.expected_timing_ms(0) == (0.0, 0.0)
    with m.Matrix(xi.TABLE, [2500000]) as mx:                                 # an empty matrix
        assert mx.run() == (0, 0)
        e = mx.expected(0, use_weights=False)
        assert not e.cis.count_sum.any() and not e.trans.count_sum.any() and (e.genome.expected == 0).all() and mx.values(0, "oe").size == 0
        assert e.cis.n_valid[0] == mx.info(0)[0] - sum(-(-l // 2500000) for _, l in xi.HG38[1:])


# ---- 5. the executable -----------------------------------------------------------------------------------------------------------------
def _tsv(path, ncols):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b""
    rows = [l.split(b"\t") for l in lines[1:-1]]
    assert all(len(x) == ncols for x in rows)
    return lines[0].split(b"\t"), rows


def _f(col):
    return np.array([float(x) for x in col], dtype=np.float64)


def _u(col):
    return np.array([int(x) for x in col], dtype=np.uint64)


def test_executable_writes_the_three_tables(tmp_path):
    _need_gpu()
    text = xi.drawn(3_000_000, SEED, RES_LONG)[0]
    t = tmp_path / "g.sizes"
    t.write_bytes(xi.TABLE)
    p = tmp_path / "in.pairs"
    p.write_bytes(text)
    for d in "abcd":
        os.makedirs(tmp_path / d)
    res = RES[:2]
    rl = ",".join(map(str, res))
    run = lambda d, *a: subprocess.run([EXE, "-g", str(t), "-r", rl, "-o", str(tmp_path / d / "o"), *a, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    runs = [run("a"), run("b", "--balance"), run("c", "--balance", "--expected"), run("d", "--expected")]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted([f"o.{r}.coo" for r in res] + [f"o.{r}.bins.bed" for r in res] + ["o.matrix.stat"])
    bal = sorted(plain + [f"o.{r}.weights.bed" for r in res] + ["o.balance.stat"])
    exp = [f"o.{r}.expected{x}.tsv" for r in res for x in ("", ".chrom", ".trans")]
    # without --expected: the file set and the bytes of a run before this option existed (test_gpu_balance.py pins that set and the .coo / .bed bytes)
    assert sorted(os.listdir(tmp_path / "a")) == plain and sorted(os.listdir(tmp_path / "b")) == bal
    cells = xi.drawn(3_000_000, SEED, RES_LONG)[1]
    for r in res:
        assert open(tmp_path / "a" / f"o.{r}.coo", "rb").read() == md.coo_text(cells[r])
        assert open(tmp_path / "a" / f"o.{r}.bins.bed", "rb").read() == md.bins_bed(xi.TABLE, r)
    assert open(tmp_path / "a" / "o.matrix.stat", "rb").read() == md.stat_text(len(text.splitlines()), 0, [(r, cells[r].shape[0]) for r in res])
    assert sorted(os.listdir(tmp_path / "c")) == sorted(bal + exp) and sorted(os.listdir(tmp_path / "d")) == sorted(plain + exp)
    for f in plain:                                                           # --expected changes none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "d" / f, "rb").read() == open(tmp_path / "c" / f, "rb").read(), f
    for f in bal:
        assert open(tmp_path / "b" / f, "rb").read() == open(tmp_path / "c" / f, "rb").read(), f
    names = [n.encode() for n, _ in xi.HG38]
    with _loaded(text, res) as mx:
        for d, uw in (("c", True), ("d", False)):
            for k, r in enumerate(res):
                if uw:
                    mx.balance(k)
                e = mx.expected(k, use_weights=uw)
                off, nb = xi.offsets(r)
                n_c = np.diff(np.append(np.asarray(off), nb))
                hdr, rows = _tsv(tmp_path / d / f"o.{r}.expected.tsv", 7)
                assert hdr == [b"diag", b"dist_bp", b"n_valid", b"count_sum", b"balanced_sum", b"expected", b"expected_smooth"]
                cols = list(zip(*rows))
                g = e.genome
                assert (_u(cols[0]) == np.arange(g.n_valid.size)).all() and (_u(cols[1]) == np.arange(g.n_valid.size) * r).all()
                assert (_u(cols[2]) == g.n_valid).all() and (_u(cols[3]) == g.count_sum).all()
                for col, arr in zip(cols[4:], (g.balanced_sum, g.expected, g.expected_smooth)):                  # %.17g round-trips a double exactly
                    assert np.array_equal(_f(col), arr, equal_nan=True) and all((x == b"nan") == bool(np.isnan(y)) for x, y in zip(col, arr))
                hdr, rows = _tsv(tmp_path / d / f"o.{r}.expected.chrom.tsv", 5)
                assert hdr == [b"chrom", b"diag", b"n_valid", b"count_sum", b"balanced_sum"] and len(rows) == nb
                cols = list(zip(*rows))
                assert list(cols[0]) == [names[c] for c in range(len(names)) for _ in range(n_c[c])]
                assert (_u(cols[1]) == np.concatenate([np.arange(n) for n in n_c])).all()
                assert (_u(cols[2]) == e.cis.n_valid).all() and (_u(cols[3]) == e.cis.count_sum).all() and np.array_equal(_f(cols[4]), e.cis.balanced_sum)
                hdr, rows = _tsv(tmp_path / d / f"o.{r}.expected.trans.tsv", 6)
                assert hdr == [b"chrom1", b"chrom2", b"n_valid", b"count_sum", b"balanced_sum", b"expected"]
                cols = list(zip(*rows))
                assert [(x, y) for x, y in zip(cols[0], cols[1])] == [(names[a], names[b]) for a in range(len(names)) for b in range(a + 1, len(names))]
                assert (_u(cols[2]) == e.trans.n_valid).all() and (_u(cols[3]) == e.trans.count_sum).all()
                assert np.array_equal(_f(cols[4]), e.trans.balanced_sum) and np.array_equal(_f(cols[5]), e.trans.expected, equal_nan=True)
