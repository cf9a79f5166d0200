"""Matrix balancing on the GPU (mkt_matrix_balance, Matrix.balance, pairs2matrix --balance) against the definition restated in
tests/balancedef.py.  The mask, the iteration count and the stopping decision must be identical; the weights agree to the bound
iterations x longest row x 2^-52 (the linear worst case of float64 sums of positive terms taken in another order: derived from the
input, not tuned); repeated calls, another process and another route of the same pairs give the same bits.  Parity with cooler's
`balance` is unpinned (cooler is not run)."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import balancedef as bd
import matrixdef as md
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
RES = [2500000, 500000, 100000]
HG38 = [("chr1", 248956422), ("chr10", 133797422), ("chr11", 135086622), ("chr12", 133275309), ("chr13", 114364328), ("chr14", 107043718),
        ("chr15", 101991189), ("chr16", 90338345), ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr2", 242193529),
        ("chr20", 64444167), ("chr21", 46709983), ("chr22", 50818468), ("chr3", 198295559), ("chr4", 190214555), ("chr5", 181538259),
        ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636), ("chr9", 138394717), ("chrM", 16569), ("chrX", 156040895),
        ("chrY", 57227415)]
TABLE = "".join(f"{n}\t{l}\n" for n, l in HG38).encode()
TROWS = [(n.encode(), l) for n, l in HG38]
SEED = 21


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _text(ia, pa, ib, pb):
    names = [nm for nm, _ in HG38]
    return "".join(f"q\t{names[a]}\t{p}\t{names[b]}\t{q}\t+\t-\n" for a, p, b, q in zip(ia.tolist(), pa.tolist(), ib.tolist(), pb.tolist())).encode()


def generate(n_draw, seed):
    """Pairs inside the tabulated lengths, two thirds cis with log-uniform distances from 1 kb to 50 Mb, thinned by a visibility factor
    per 250 kb bin (uniform in [0.3, 1], about 3 % of the bins at 0.01) on both sides: (ia, pa, ib, pb) of the kept pairs."""
    rng = np.random.default_rng(seed)
    L = np.array([l for _, l in HG38], dtype=np.int64)
    w = L / L.sum()
    ia = rng.choice(len(L), size=n_draw, p=w)
    ib = np.where(rng.random(n_draw) < 0.67, ia, rng.choice(len(L), size=n_draw, p=w))
    pa = np.minimum(1 + (rng.random(n_draw) * L[ia]).astype(np.int64), L[ia])
    dist = np.exp(rng.uniform(math.log(1e3), math.log(5e7), size=n_draw)).astype(np.int64) * rng.choice(np.array([-1, 1]), size=n_draw)
    near = np.clip(pa + dist, 1, L[ia])
    far = np.minimum(1 + (rng.random(n_draw) * L[ib]).astype(np.int64), L[ib])
    pb = np.where(ia == ib, near, far)
    off, _, nb = md.bin_layout(TROWS, 250000)
    off = np.array(off, dtype=np.int64)
    vis = rng.uniform(0.3, 1.0, size=nb)
    vis[rng.random(nb) < 0.03] = 0.01
    keep = rng.random(n_draw) < vis[off[ia] + (pa - 1) // 250000] * vis[off[ib] + (pb - 1) // 250000]
    return ia[keep], pa[keep], ib[keep], pb[keep]


@functools.lru_cache(maxsize=None)
def _main_input():
    ia, pa, ib, pb = generate(3_000_000, SEED)
    cells = {r: c for r, (c, _sk) in md.definition_arrays(TROWS, RES, ia, pa, ib, pb).items()}
    return _text(ia, pa, ib, pb), cells, ia.size


def _offsets(r):
    return md.bin_layout(TROWS, r)[0:3:2]                                   # (offsets, nbins)


def _define(cells, r, **opts):
    off, nb = _offsets(r)
    return bd.balance(cells[:, 0], cells[:, 1], cells[:, 2], nb, off, **opts)


def _preconditions(want, tol, expect_converged=True):
    """on the checker alone, before the GPU is asked: conditions on the input, not measurements of the code under test"""
    if expect_converged:
        assert want.converged
        assert want.variances[-1] < tol * (1 - 1e-6)
        if len(want.variances) > 1:
            assert want.variances[-2] > tol * (1 + 1e-6)
    else:
        assert not want.converged and all(v > tol * (1 + 1e-6) for v in want.variances)
    if want.cut is not None:
        fm = want.filter_marg[want.filter_marg > 0]
        assert np.abs(fm / want.cut - 1.0).min() > 1e-9                     # no marginal sits on the filter's threshold


def _compare(got_w, got_st, want, label=""):
    """the mask and the discrete outcomes identical; the weights within the derived bound.  Returns the largest relative deviation."""
    wn, gn = np.isnan(want.weights), np.isnan(got_w)
    assert (wn == gn).all(), (label, int(wn.sum()), int(gn.sum()))
    assert (got_st.iterations, got_st.converged, got_st.masked) == (want.iterations, want.converged, want.masked), (label, got_st, want[1:6])
    if wn.all():
        assert math.isnan(got_st.scale) and math.isnan(got_st.var)
        return 0.0
    rtol = want.iterations * want.longest_row * 2.0 ** -52
    dev = float(np.abs(got_w[~wn] / want.weights[~wn] - 1.0).max())
    print(f"balance {label}: iterations {want.iterations} masked {want.masked} longest row {want.longest_row} max rel dev {dev:.3e} bound {rtol:.3e}")
    assert dev <= rtol, (label, dev, rtol)
    assert abs(got_st.scale / want.scale - 1.0) <= rtol and abs(got_st.var / want.var - 1.0) < 1e-6
    return dev


def _loaded(text, res=RES):
    mx = m.Matrix(TABLE, res, device=0)
    mx.add(text)
    mx.run()
    return mx


# ---- 1. the generated input against the definition, at three resolutions ---------------------------------------------------------
def test_generated_input_against_the_definition(tmp_path):
    _need_gpu()
    text, cells, n = _main_input()
    assert 1_000_000 < n < 1_500_000
    wants = [_define(cells[r], r) for r in RES]
    for want in wants:
        _preconditions(want, 1e-5)
        assert 0 < want.masked < want.weights.size // 4
    assert max(w.longest_row for w in wants) > 500
    with _loaded(text) as mx:
        before = [(mx.cells(k), mx.text(k)) for k in range(3)]
        for k, r in enumerate(RES):
            assert (np.stack(before[k][0], axis=1) == cells[r]).all()
        with pytest.raises(m.MktError, match="balance first"):
            mx.weights(1)
        ws = {}
        for k in (1, 0, 2):                                                 # not in index order: a resolution is on its own
            st = mx.balance(k)
            ws[k] = mx.weights(k)
            assert ws[k].dtype == np.float64 and ws[k].size == mx.info(k)[0]
            _compare(ws[k], st, wants[k], f"r={RES[k]}")
            setup_ms, iter_ms = mx.balance_timing_ms(k)
            assert setup_ms > 0 and iter_ms > 0
            # the property itself, from the GPU's weights and the GPU's cells: the balanced marginals of the unmasked bins
            b1, b2, c = before[k][0]
            bal = bd.balanced_marginals(b1, b2, c, ws[k].size, ws[k])[~np.isnan(ws[k])]
            mean = bal.mean()
            print(f"balanced marginals r={RES[k]}: mean {mean:.9f} var(m/mean) {np.var(bal / mean):.3e}")
            assert np.var(bal / mean) < 1e-5 and abs(mean - 1.0) < math.sqrt(1e-5)
            # cells and text of every resolution are what they were, and so are the other resolutions' weights
            for j in range(3):
                now = mx.cells(j)
                assert all((a == b).all() for a, b in zip(now, before[j][0])) and mx.text(j) == before[j][1]
            for j, w in ws.items():
                assert mx.weights(j).tobytes() == w.tobytes()
        # again in the same process: the same bits, and the setup is reused
        for k in range(3):
            st2 = mx.balance(k)
            assert mx.weights(k).tobytes() == ws[k].tobytes() and st2.iterations == wants[k].iterations
            assert mx.balance_timing_ms(k)[0] == 0.0
        # a later run discards the weights
        mx.run()
        with pytest.raises(m.MktError, match="balance first"):
            mx.weights(0)
        assert mx.balance(0).iterations == wants[0].iterations and mx.weights(0).tobytes() == ws[0].tobytes()
    # another process
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(text)
    (tmp_path / "g.sizes").write_bytes(TABLE)
    script = ("import sys, microcket_amd as m\n"
              "mx = m.Matrix(open(sys.argv[1], 'rb').read(), [int(x) for x in sys.argv[3].split(',')])\n"
              "mx.add(open(sys.argv[2], 'rb').read()); mx.run()\n"
              "for k in range(len(mx.resolutions)):\n"
              "    mx.balance(k); open(sys.argv[4] + '.%d' % k, 'wb').write(mx.weights(k).tobytes())\n"
              "mx.close()\n")
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "g.sizes"), str(pairs), ",".join(map(str, RES)), str(tmp_path / "w")], env=env, cwd=util.ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    for k in range(3):
        assert open(f"{tmp_path}/w.{k}", "rb").read() == ws[k].tobytes()


# ---- 1a. every lane width of the sweep: 8, 16, 32 and 64 lanes per bin ------------------------------------------------------------
def _width(nnz, nbins):
    """the sweep's lanes per bin, as mkt_balance.hip picks them from the cells a bin walks on average"""
    avg = 2 * nnz // nbins
    return 64 if avg >= 48 else 32 if avg >= 24 else 16 if avg >= 12 else 8


def test_every_lane_width_of_the_sweep():
    _need_gpu()
    ia, pa, ib, pb = generate(3_000_000, SEED)
    res = [100000, 50000, 25000, 10000]
    opts = dict(min_nnz=4)
    cells = {r: c for r, (c, _sk) in md.definition_arrays(TROWS, res, ia, pa, ib, pb).items()}
    widths = [_width(cells[r].shape[0], _offsets(r)[1]) for r in res]
    assert widths == [64, 32, 16, 8], widths                               # a condition on the input: one resolution per compiled variant
    wants = [_define(cells[r], r, **opts) for r in res]
    for want in wants:
        _preconditions(want, 1e-5)
        assert want.masked < want.weights.size // 2
    with _loaded(_main_input()[0], res) as mx:
        for k, r in enumerate(res):
            assert mx.info(k)[:2] == (_offsets(r)[1], cells[r].shape[0])
            st = mx.balance(k, **opts)
            _compare(mx.weights(k), st, wants[k], f"width {widths[k]} r={r}")


# ---- 2. options other than the defaults ------------------------------------------------------------------------------------------
def test_options_are_honoured():
    _need_gpu()
    text, cells, _ = _main_input()
    r = RES[1]
    cases = [dict(ignore_diags=0), dict(mad_max=0), dict(min_nnz=0), dict(min_count=50), dict(tol=1e-12), dict(max_iters=2),
             dict(ignore_diags=5, min_nnz=3, min_count=20, mad_max=3.0, tol=1e-8, max_iters=100)]
    wants = []
    for o in cases:
        want = _define(cells[r], r, **o)
        _preconditions(want, o.get("tol", 1e-5), expect_converged="max_iters" not in o or o["max_iters"] > 2)
        wants.append(want)
    assert len({(w.masked, w.iterations) for w in wants}) >= 5               # the options do change the outcome
    assert wants[5].iterations == 2 and not wants[5].converged
    with _loaded(text) as mx:
        for o, want in zip(cases, wants):
            st = mx.balance(1, **o)
            _compare(mx.weights(1), st, want, str(o))
        with pytest.raises(TypeError):
            mx.balance(1, cis_only=True)


# ---- 3. the add_keys route gives the bits of the text route ----------------------------------------------------------------------
def test_pairs_from_context_keys_give_the_same_weights():
    _need_gpu()
    res = [2500000, 500000]
    opts = dict(min_nnz=2, ignore_diags=1)
    c = m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS)
    try:
        p, _s, st, _log = c.run_bytes(util.synth("unc", 61, 20000), chunk=1 << 20)
        total, dups, flags = c.ext_dedup(True)
        assert total == md.n_pairs(p) and dups < total
        lines = p.splitlines(keepends=True)
        kept = b"".join(l for l, f in zip(lines, flags) if not f)
        for fl, body in ((None, p), (flags, kept)):
            with m.Matrix(TABLE, res) as a, _loaded(body, res) as b:
                a.add_keys(c, True, fl)
                a.run()
                for k, r in enumerate(res):
                    sa, sb = a.balance(k, **opts), b.balance(k, **opts)
                    wa, wb = a.weights(k), b.weights(k)
                    assert wa.tobytes() == wb.tobytes() and sa[:2] == sb[:2] and sa.masked == sb.masked
                    assert repr(sa.var) == repr(sb.var) and repr(sa.scale) == repr(sb.scale)
                    assert not np.isnan(wa).all()
    finally:
        c.close()


# ---- 4. nothing to balance, and the errors -----------------------------------------------------------------------------------------
def test_empty_all_masked_and_errors():
    _need_gpu()
    with m.Matrix(TABLE, [2500000, 500000]) as mx:
        with pytest.raises(m.MktError, match="balance before run"):
            mx.balance(0)
        assert mx.run() == (0, 0)
        st = mx.balance(0)                                                  # an empty matrix
        w = mx.weights(0)
        assert w.size == mx.info(0)[0] and np.isnan(w).all()
        assert (st.iterations, st.converged, st.masked) == (1, False, w.size) and math.isnan(st.scale) and math.isnan(st.var)
        st = mx.balance(1, min_nnz=0, mad_max=0)
        assert np.isnan(mx.weights(1)).all() and not st.converged
    text = _main_input()[0][:200000].rsplit(b"\n", 1)[0] + b"\n"
    with _loaded(text, [500000]) as mx:
        nb = mx.info(0)[0]
        st = mx.balance(0, min_nnz=1000000)                                 # every bin below the filter
        assert np.isnan(mx.weights(0)).all() and (st.iterations, st.converged, st.masked) == (1, False, nb)
        b1, b2, c = mx.cells(0)
        want = _define(np.stack([b1, b2, c], axis=1).astype(np.uint64), 500000, min_nnz=1000000)
        assert want.masked == nb and want.iterations == 1 and not want.converged
        for o, what in ((dict(ignore_diags=-1), "ignore_diags"), (dict(min_nnz=-2), "min_nnz"), (dict(min_count=-1.0), "min_count"), (dict(min_count=float("nan")), "min_count"),
                        (dict(mad_max=-0.5), "mad_max"), (dict(mad_max=float("nan")), "mad_max"), (dict(tol=-1e-9), "tol"), (dict(tol=float("nan")), "tol"),
                        (dict(max_iters=0), "max_iters"), (dict(max_iters=-4), "max_iters")):
            with pytest.raises(m.MktError, match=what):
                mx.balance(0, **o)
        with pytest.raises(m.MktError, match="resolution index"):
            mx.balance(3)
        with pytest.raises(m.MktError, match="resolution index"):
            mx.weights(3)
        assert np.isnan(mx.weights(0)).all()                                # a refused call leaves the weights alone
        mx.balance(0, min_nnz=0, mad_max=0)
        import ctypes as C
        buf = (C.c_double * 4)()
        with pytest.raises(m.MktError, match="weights"):
            mx._chk(mx.L.mkt_matrix_fetch_weights(mx.h, 0, nb - 2, 4, buf), "mkt_matrix_fetch_weights")
        mx._chk(mx.L.mkt_matrix_fetch_weights(mx.h, 0, nb - 4, 4, buf), "mkt_matrix_fetch_weights")
        assert np.array_equal(np.array(list(buf)), mx.weights(0)[-4:], equal_nan=True)
        # NULL options are the defaults
        mx._chk(mx.L.mkt_matrix_balance(mx.h, 0, None, None), "mkt_matrix_balance")
        w0 = mx.weights(0)
        mx.balance(0)
        assert mx.weights(0).tobytes() == w0.tobytes()


# ---- 5. a hot cell and a bin that touches every other bin: the long-row path -------------------------------------------------------
def test_hot_cell_and_a_row_through_every_bin():
    _need_gpu()
    rng = np.random.default_rng(5)
    ia, pa, ib, pb = generate(700_000, 13)
    off, _, nb = md.bin_layout(TROWS, 2500000)
    L = np.array([l for _, l in HG38], dtype=np.int64)
    # chr7:5,000,001-7,500,000 (one bin at 2.5 Mb) meets every bin of the genome 40 times
    starts = [(i, s) for i in range(len(L)) for s in range(0, int(L[i]), 2500000)]
    assert len(starts) == nb
    hub = []
    for i, s in starts:
        for _ in range(40):
            hub.append((19, 5_000_001 + int(rng.integers(0, 2_400_000)), i, min(s + 1 + int(rng.integers(0, 2_500_000)), int(L[i]))))
    ha, hp, hb, hq = (np.array(x, dtype=np.int64) for x in zip(*hub))
    assert HG38[19][0] == "chr7"
    hot = b"h\tchr7\t5000001\tchr7\t12600999\t+\t-\n" * 250000            # one cell of 250,000, three bins off the diagonal at 2.5 Mb
    text = _text(np.concatenate([ia, ha]), np.concatenate([pa, hp]), np.concatenate([ib, hb]), np.concatenate([pb, hq])) + hot
    res = [2500000, 500000]
    cells = {r: c for r, (c, _sk) in md.definition(TABLE, res, text).items()}
    wants = [_define(cells[r], r) for r in res]
    assert wants[0].longest_row > 1200 and int(cells[2500000][:, 2].max()) >= 250000
    for want in wants:
        _preconditions(want, 1e-5)
    with _loaded(text, res) as mx:
        for k, r in enumerate(res):
            assert (np.stack(mx.cells(k), axis=1) == cells[r]).all()
            st = mx.balance(k)
            w = mx.weights(k)
            _compare(w, st, wants[k], f"hot r={r}")
            hubbin = off[19] + 2
            if k == 0:
                assert not np.isnan(w[hubbin])
            assert mx.balance(k).iterations == st.iterations and mx.weights(k).tobytes() == w.tobytes()


# ---- 6. the executable ---------------------------------------------------------------------------------------------------------------
def test_executable_writes_weights_and_stats(tmp_path):
    _need_gpu()
    text = _main_input()[0]
    t = tmp_path / "g.sizes"
    t.write_bytes(TABLE)
    p = tmp_path / "in.pairs"
    p.write_bytes(text)
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    os.makedirs(tmp_path / "c")
    rl = ",".join(map(str, RES))
    ra = subprocess.run([EXE, "-g", str(t), "-r", rl, "-o", str(tmp_path / "a" / "o"), str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    rb = subprocess.run([EXE, "-g", str(t), "-r", rl, "-o", str(tmp_path / "b" / "o"), "--balance", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    assert b"WARN" not in rb.stderr
    plain = sorted(os.listdir(tmp_path / "a"))
    assert plain == sorted([f"o.{r}.coo" for r in RES] + [f"o.{r}.bins.bed" for r in RES] + ["o.matrix.stat"])      # the file set of a run without --balance
    assert sorted(os.listdir(tmp_path / "b")) == sorted(plain + [f"o.{r}.weights.bed" for r in RES] + ["o.balance.stat"])
    for f in plain:                                                          # ... and --balance changes none of their bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    cells = _main_input()[1]
    for r in RES:
        assert open(tmp_path / "a" / f"o.{r}.coo", "rb").read() == md.coo_text(cells[r])
        assert open(tmp_path / "a" / f"o.{r}.bins.bed", "rb").read() == md.bins_bed(TABLE, r)
    stat = [l.split(b"\t") for l in open(tmp_path / "b" / "o.balance.stat", "rb").read().splitlines()]
    assert [int(l[0]) for l in stat] == RES and all(len(l) == 6 for l in stat)
    with _loaded(text) as mx:
        for k, r in enumerate(RES):
            st = mx.balance(k)
            w = mx.weights(k)
            bins = open(tmp_path / "b" / f"o.{r}.bins.bed", "rb").read().splitlines()
            wl = open(tmp_path / "b" / f"o.{r}.weights.bed", "rb").read().splitlines()
            assert len(wl) == len(bins) == w.size
            assert [l.rsplit(b"\t", 1)[0] for l in wl] == bins
            vals = [l.rsplit(b"\t", 1)[1] for l in wl]
            assert all((v == b"nan") == bool(np.isnan(x)) for v, x in zip(vals, w))
            assert all(float(v) == x for v, x in zip(vals, w) if v != b"nan")           # %.17g round-trips a double exactly
            assert (int(stat[k][1]), int(stat[k][2]), int(stat[k][5])) == (st.iterations, int(st.converged), st.masked)
            assert float(stat[k][3]) == st.var and float(stat[k][4]) == st.scale
    # options reach the library; a resolution that does not converge is a warning, not a failure
    rc = subprocess.run([EXE, "-g", str(t), "-r", "500000", "-o", str(tmp_path / "c" / "o"), "--balance", "--max-iters", "2", "--ignore-diags", "0", "--min-nnz", "0",
                         "--mad-max", "0", "--min-count", "50", "--tol", "1e-12", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert rc.returncode == 0 and b"WARN" in rc.stderr and b"did not converge" in rc.stderr
    want = _define(cells[500000], 500000, max_iters=2, ignore_diags=0, min_nnz=0, mad_max=0, min_count=50, tol=1e-12)
    line = open(tmp_path / "c" / "o.balance.stat", "rb").read().split(b"\t")
    assert (int(line[0]), int(line[1]), int(line[2]), int(line[5])) == (500000, 2, 0, want.masked)
    assert abs(float(line[4]) / want.scale - 1.0) < 1e-9
