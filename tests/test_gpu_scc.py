"""Replicate comparison on the GPU (mkt_matrix_scc, Matrix.scc, pairs2matrix --compare) against the definition restated in
tests/sccdef.py, fed the GPU's own cells and weights.  The summation order is part of the definition, so there is no tolerance: the
strata table, the per-chromosome arrays and the info doubles must be the same bytes.  Parity with HiCRep is unpinned (it is not run)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import microcket_amd as m
import scc_inputs as si
import sccdef as sd
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _loaded(ttext, text, res=(si.R,), pieces=0):
    mx = m.Matrix(ttext, list(res), device=0)
    if pieces:
        for p in range(0, len(text), pieces):
            mx.add(text[p:p + pieces])
    else:
        mx.add(text)
    mx.run()
    return mx


def _bits(x):
    return struct.pack("<d", x)


def _want(a, b, k, rep, swap=False, **opts):
    """the definition on the GPU's own cells and weights"""
    o = dict(opts)
    o.pop("slab_rows", None)
    if o.pop("use_weights", 0):
        o["weights_a"], o["weights_b"] = a.weights(k), b.weights(k)
    return sd.scc(tuple(x.astype(np.int64) for x in a.cells(k)), tuple(x.astype(np.int64) for x in b.cells(k)), rep.nb, rep.off, swap=swap, **o)


def _compare(label, got, info, want):
    for f in sd.FIELDS:
        assert getattr(got, f).dtype == getattr(want, f).dtype and getattr(got, f).shape == getattr(want, f).shape, (label, f)
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (label, f, getattr(got, f), getattr(want, f))
    for f in sd.INTS:
        assert getattr(info, f) == want.info[f], (label, f, getattr(info, f), want.info[f])
    assert _bits(info.scc) == _bits(want.info["scc"]), (label, info.scc, want.info["scc"])


def _check(label, a, b, k, rep, **opts):
    info = a.scc(b, k, **opts)
    got = a.scc_result(k)
    want = _want(a, b, k, rep, **opts)
    _compare(f"{label} {opts}", got, info, want)
    return got, info, want


def _all_bytes(a, b, k, **opts):
    info = a.scc(b, k, **opts)
    return b"".join([x.tobytes() for x in a.scc_result(k)] + [_bits(info.scc)])


# ---- 1. chunk edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", si.CHUNK_BINS)
def test_chunk_edges(nc):
    _need_gpu()
    rep = si.chunk_edges(nc)
    with _loaded(rep.ttext, rep.text_a) as a, _loaded(rep.ttext, rep.text_b) as b:
        assert (np.stack(a.cells(0), axis=1) == rep.cells_a).all() and (np.stack(b.cells(0), axis=1) == rep.cells_b).all()
        got, info, want = _check(f"chunks {nc}", a, b, 0, rep, h=si.CHUNK_H, max_diag=si.CHUNK_MAX_DIAG)
        assert info.strata == 4 and got.n_cand.tolist() == [max(nc - d, 0) for d in range(4)]
        if nc >= 255:
            assert info.scored == 4 and -1.0 < info.scc < 1.0
        f, s = a.scc_timing_ms(0)
        assert f > 0 and s > 0


# ---- 2. window edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", si.WINDOW_HS)
def test_window_edges(h):
    _need_gpu()
    full, only0, only1 = si.window_edges()
    o = dict(h=h, max_diag=si.WINDOW_MAX_DIAG)
    D = si.WINDOW_MAX_DIAG + 1
    with _loaded(full.ttext, full.text_a) as a, _loaded(full.ttext, full.text_b) as b:
        got, info, want = _check("window", a, b, 0, full, **o)
        assert info.n_chrom == 2 and info.strata == D and (got.n[D + 7:] == 0).all() and np.isnan(got.rho[D + 7:]).all()      # d >= n_c
        assert not np.isnan(got.rho[:max(2 * h, 1)]).any() and got.n_scored[0] == D                 # strata where the window crosses the diagonal are scored
        strata = [getattr(got, f) for f in sd.STRATA]
    for c, only in enumerate((only0, only1)):                                    # trans cells and the neighbour's cells never enter
        with _loaded(only.ttext, only.text_a) as a, _loaded(only.ttext, only.text_b) as b:
            alone, _, _ = _check(f"window, chromosome {c} alone", a, b, 0, only, **o)
            for f, x in zip(sd.STRATA, strata):
                assert getattr(alone, f)[c * D:(c + 1) * D].tobytes() == x[c * D:(c + 1) * D].tobytes(), (c, f)
            assert alone.n[(1 - c) * D:(2 - c) * D].sum() == 0


# ---- 3. weights and masks ----------------------------------------------------------------------------------------------------------------
def test_weights_and_masks():
    _need_gpu()
    rep, bare_a, bare_b = si.masked()
    with _loaded(rep.ttext, rep.text_a) as a, _loaded(rep.ttext, rep.text_b) as b:
        a.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        b.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        assert np.flatnonzero(np.isnan(a.weights(0))).tolist() == bare_a and np.flatnonzero(np.isnan(b.weights(0))).tolist() == bare_b
        for o in (dict(h=3, max_diag=15), dict(h=1, min_diag=2, max_diag=40, weighting="var"), dict(h=0)):
            got, info, want = _check("masked", a, b, 0, rep, use_weights=1, **o)
            raw = a.scc(b, 0, **o)
            assert info.candidates < raw.candidates and info.scored > 3 and info.count_a < raw.count_a


# ---- 4. used and scored --------------------------------------------------------------------------------------------------------------------
def test_used_and_scored():
    _need_gpu()
    rep = si.used_and_scored()
    with _loaded(rep.ttext, rep.text_a) as a, _loaded(rep.ttext, rep.text_b) as b:
        got, info, want = _check("used", a, b, 0, rep, **si.USED_OPTS)
        assert 0 < got.n[0] < got.n_cand[0] and np.isnan(got.rho[1]) and got.w[1] == 0 and got.n[2] == 2 and np.isnan(got.rho[2]) and info.scored == 2
        got, info, want = _check("used", a, b, 0, rep, **dict(si.USED_OPTS, min_n=2))
        assert not np.isnan(got.rho[2]) and info.scored == 3                    # two positions are a line: |rho| is 1
        assert abs(abs(got.rho[2]) - 1.0) < 1e-12


# ---- 5. weighting and exchange ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["n", "var"])
def test_weighting_and_exchange(weighting):
    _need_gpu()
    full = si.window_edges()[0]
    o = dict(h=2, max_diag=si.WINDOW_MAX_DIAG, weighting=weighting)
    with _loaded(full.ttext, full.text_a) as a, _loaded(full.ttext, full.text_b) as b:
        ab, iab, _ = _check("ab", a, b, 0, full, **o)
        iba = b.scc(a, 0, **o)
        ba = b.scc_result(0)
        _compare("ba", ba, iba, _want(a, b, 0, full, swap=True, **o))             # x and y exchanged and nothing else
        for f, g in (("sx", "sy"), ("sy", "sx"), ("sxx", "syy"), ("syy", "sxx"), ("sxy", "sxy"), ("rho", "rho"), ("w", "w"), ("scc", "scc"), ("num", "num"), ("den", "den")):
            assert getattr(ab, f).tobytes() == getattr(ba, g).tobytes(), (f, g)
        assert _bits(iab.scc) == _bits(iba.scc) and (iab.count_a, iab.count_b) == (iba.count_b, iba.count_a) and iab.count_a != iab.count_b
        same = a.scc(a, 0, **o)                                                 # A and B may be the same object
        assert same.scored > 0 and abs(same.scc - 1.0) < 1e-12
        _compare("aa", a.scc_result(0), same, _want(a, a, 0, full, **o))
    if weighting == "var":
        assert ab.w.tobytes() != ab.n.astype(np.float64).tobytes()


# ---- 6. slabs and routes ---------------------------------------------------------------------------------------------------------------------
def test_slabs_and_routes():
    _need_gpu()
    rep = si.slabs()
    o = dict(h=5, max_diag=9)
    with _loaded(rep.ttext, rep.text_a) as a, _loaded(rep.ttext, rep.text_b) as b:
        got, info, want = _check("slabs", a, b, 0, rep, **o)
        first = _all_bytes(a, b, 0, **o)
        assert _all_bytes(a, b, 0, **o) == first                                # two calls in a row
        for slab in (256, 512, 1024, 0):
            assert _all_bytes(a, b, 0, slab_rows=slab, **o) == first, slab
        assert _all_bytes(a, b, 0, h=5) != first and info.scored >= 10          # every diagonal (max_diag 0) is another table
        _check("slabs, every diagonal", a, b, 0, rep, h=2, slab_rows=256)
    with _loaded(rep.ttext, rep.text_a, pieces=7919) as a, _loaded(rep.ttext, rep.text_b, pieces=104729) as b:
        assert _all_bytes(a, b, 0, **o) == first                                # pairs added in odd pieces


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_results_alone():
    _need_gpu()
    rep, _, _ = si.masked()
    other = si.slabs()
    o = dict(h=2, max_diag=10)
    with m.Matrix(rep.ttext, [si.R, 5 * si.R]) as a, _loaded(rep.ttext, rep.text_b, res=(5 * si.R, si.R)) as b, _loaded(other.ttext, other.text_a) as c, \
            m.Matrix(rep.ttext, [si.R]) as unrun:
        with pytest.raises(m.MktError, match="scc before run"):
            a.scc(b, 0)
        a.add(rep.text_a)
        a.run()
        with pytest.raises(m.MktError, match="scc before run of the second matrix"):
            a.scc(unrun, 0)
        with pytest.raises(m.MktError, match="scc first"):
            a.scc_result(0)
        assert a.scc_timing_ms(0) == (0.0, 0.0) and a.L.mkt_matrix_scc_timing(a.h, 2, None, None) != 0
        info = a.scc(b, 0, **o)                                                 # b holds the resolution at its index 1
        kept = b"".join(x.tobytes() for x in a.scc_result(0))
        _compare("index by value", a.scc_result(0), info, _want_mixed(a, b, rep, **o))
        call = lambda ra, other_h, rb, so: a._chk(a.L.mkt_matrix_scc(a.h, ra, other_h, rb, C.byref(so) if so is not None else None, None), "scc")
        so = m.SccOpts()
        a.L.mkt_scc_opts_default(C.byref(so))
        assert (so.h, so.min_diag, so.max_diag, so.use_weights, so.weighting, so.min_n, so.slab_rows, list(so.reserved)) == (5, 0, 0, 0, 0, 3, 0, [0, 0, 0])
        for ra, oh, rb, what in ((2, b.h, 1, "resolution index 2"), (0, b.h, 2, "resolution index 2 of 2 in the second matrix"), (0, b.h, 0, "resolution 1000 against resolution 5000"),
                                 (0, c.h, 0, "chromosome tables"), (0, None, 0, "NULL")):
            with pytest.raises(m.MktError, match=what):
                call(ra, oh, rb, so)
        for bad, what in ((dict(h=-1), "h -1"), (dict(h=17), "h 17"), (dict(min_diag=-1), "min_diag -1"), (dict(max_diag=-3), "max_diag -3"), (dict(min_diag=5, max_diag=4), "max_diag 4 is below min_diag 5"),
                          (dict(min_diag=1000), "is below min_diag 1000"), (dict(use_weights=2), "use_weights 2"), (dict(weighting=2), "weighting 2"), (dict(weighting=-1), "weighting -1"),
                          (dict(min_n=1), "min_n 1"), (dict(slab_rows=100), "slab_rows 100"), (dict(slab_rows=-256), "slab_rows -256")):
            with pytest.raises(m.MktError, match=what):
                a.scc(b, 0, **bad)
        for k in range(3):
            so.reserved[k] = 7
            with pytest.raises(m.MktError, match="reserved"):
                call(0, b.h, 1, so)
            so.reserved[k] = 0
        with pytest.raises(TypeError):
            a.scc(b, 0, window=3)
        with pytest.raises(ValueError):
            a.scc(b, 0, weighting="rank")
        with pytest.raises(m.MktError, match="no resolution"):
            a.scc(c, 1)
        with pytest.raises(m.MktError, match="balance first"):
            a.scc(b, 0, use_weights=1)
        a.balance(0, min_nnz=1, mad_max=0)
        with pytest.raises(m.MktError, match="scc first"):                       # a balance of A discards the results
            a.scc_result(0)
        info = a.scc(b, 0, **o)
        assert b"".join(x.tobytes() for x in a.scc_result(0)) == kept
        with pytest.raises(m.MktError, match="of the second matrix: balance first"):
            a.scc(b, 0, use_weights=1)
        with pytest.raises(m.MktError, match="scc strata"):
            a._chk(a.L.mkt_matrix_fetch_scc_strata(a.h, 0, 2 * 11 - 1, 2, *[None] * 9), "fetch")
        with pytest.raises(m.MktError, match="scc chromosomes"):
            a._chk(a.L.mkt_matrix_fetch_scc_chrom(a.h, 0, 2, 1, *[None] * 4), "fetch")
        a._chk(a.L.mkt_matrix_fetch_scc_strata(a.h, 0, 0, 22, *[None] * 9), "fetch")                # any pointer may be NULL
        a._chk(a.L.mkt_matrix_fetch_scc_chrom(a.h, 0, 0, 2, *[None] * 4), "fetch")
        one = np.zeros(1, np.float64)
        a._chk(a.L.mkt_matrix_fetch_scc_strata(a.h, 0, 13, 1, *[None] * 7, one.ctypes.data_as(C.c_void_p), None), "fetch")
        assert one.tobytes() == a.scc_result(0).rho[13:14].tobytes()
        assert b"".join(x.tobytes() for x in a.scc_result(0)) == kept           # every refused call left the results alone
        from microcket_amd.capi import _SccInfoC
        ic = _SccInfoC()
        a._chk(a.L.mkt_matrix_scc(a.h, 0, b.h, 1, None, C.byref(ic)), "scc")     # NULL options: the defaults
        d = _want_mixed(a, b, rep)
        assert (ic.strata, ic.used, ic.scored) == (60, d.info["used"], d.info["scored"]) and _bits(ic.scc) == _bits(d.info["scc"])
        assert a.L.mkt_abi_version() == 9
        a.scc(b, 0, **o)
        b.run()                                                                 # a snapshot: a run of B leaves the results on A alone
        b.balance(1, min_nnz=1, mad_max=0)
        assert b"".join(x.tobytes() for x in a.scc_result(0)) == kept and a.scc_timing_ms(0)[1] > 0
        a.scc(b, 0, use_weights=1, **o)                                         # both balanced now
        assert a.scc_result(0).n_cand.sum() < info.candidates
        line = rep.text_a.splitlines(keepends=True)[0]
        for what, again in (("run", lambda: a.run()), ("add", lambda: a.add(line))):
            a.run()
            assert a.scc(b, 0, **o).used > 0
            again()
            with pytest.raises(m.MktError, match="scc first" if what == "run" else "scc first|before run"):
                a.scc_result(0)
            assert a.scc_timing_ms(0) == (0.0, 0.0), what


def _want_mixed(a, b, rep, **opts):
    """a holds the resolution at index 0, b at index 1"""
    return sd.scc(tuple(x.astype(np.int64) for x in a.cells(0)), tuple(x.astype(np.int64) for x in b.cells(1)), rep.nb, rep.off, **opts)


# ---- 8. the executable ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("balance", [False, True])
def test_executable_writes_the_comparison(tmp_path, balance):
    _need_gpu()
    rep, _, _ = si.masked()
    (tmp_path / "g.sizes").write_bytes(rep.ttext)
    (tmp_path / "a.pairs").write_bytes(rep.text_a)
    (tmp_path / "b.pairs").write_bytes(rep.text_b)
    for d in "xy":
        os.makedirs(tmp_path / d)
    bal = ["--balance", "--min-nnz", "1", "--mad-max", "0"] if balance else []
    run = lambda d, *x: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", str(si.R), "-o", str(tmp_path / d / "o"), *bal, *x, str(tmp_path / "a.pairs")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    sub = ["--scc-h", "2", "--scc-min-dist", str(si.R), "--scc-max-dist", str(20 * si.R), "--scc-weighting", "var"]
    runs = [run("x"), run("y", "--compare", str(tmp_path / "b.pairs"), *sub)]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted(os.listdir(tmp_path / "x"))
    assert sorted(os.listdir(tmp_path / "y")) == sorted(plain + [f"o.{si.R}.scc.tsv", "o.scc.stat"])
    for f in plain:                                                             # the flag changes none of the other bytes
        assert open(tmp_path / "x" / f, "rb").read() == open(tmp_path / "y" / f, "rb").read(), f
    assert run("x", "--scc-h", "2").returncode == 2                             # a sub-option without --compare
    assert run("x", "--compare", str(tmp_path / "b.pairs"), "--scc-h", "17").returncode == 12
    assert run("x", "--compare", str(tmp_path / "b.pairs"), "--scc-max-dist", "1500").returncode == 12
    with _loaded(rep.ttext, rep.text_a) as a, _loaded(rep.ttext, rep.text_b) as b:
        if balance:
            a.balance(0, min_nnz=1, mad_max=0)
            b.balance(0, min_nnz=1, mad_max=0)
        info = a.scc(b, 0, h=2, min_diag=1, max_diag=20, weighting="var", use_weights=int(balance))
        res = a.scc_result(0)
    num = lambda x: "nan" if x != x else "%.17g" % x
    names = [ln.split(b"\t")[0].decode() for ln in rep.ttext.splitlines()]
    lines = ["chrom\tdiag\tdist_bp\tn_cand\tn\tsx\tsy\tsxx\tsyy\tsxy\trho\tw\n"]
    for c, name in enumerate(names):
        for k in range(20):
            at = c * 20 + k
            lines.append("\t".join([name, str(k + 1), str((k + 1) * si.R), str(res.n_cand[at]), str(res.n[at])] + [num(float(getattr(res, f)[at])) for f in sd.STRATA[2:]]) + "\n")
    assert open(tmp_path / "y" / f"o.{si.R}.scc.tsv", "rb").read() == "".join(lines).encode()
    stat = [f"{si.R}\tchrom\t{name}\t{res.n_scored[c]}\t{num(float(res.num[c]))}\t{num(float(res.den[c]))}\t{num(float(res.scc[c]))}\n" for c, name in enumerate(names)]
    stat.append(f"{si.R}\tgenome\t{info.n_chrom}\t{info.strata}\t{info.candidates}\t{info.used}\t{info.scored}\t{info.count_a}\t{info.count_b}\t{num(info.scc)}\n")
    assert open(tmp_path / "y" / "o.scc.stat", "rb").read() == "".join(stat).encode()
    assert info.scored > 10 and -1 < info.scc < 1
