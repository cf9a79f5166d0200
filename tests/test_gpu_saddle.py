"""Saddle tables and compartment strength on the GPU (mkt_matrix_saddle, Matrix.saddle / saddle_eigs, pairs2matrix --saddle) against the
definition restated in tests/saddledef.py, fed the GPU's own cells, weights and expected tables.  The summation order is part of the
definition, so there is no tolerance: the five tables, the groups, the edges, the profile and the info scores must be the same bytes.
Parity with cooltools saddle is unpinned (it is not run)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import eigs_inputs as gi
import loops_inputs as li
import microcket_amd as m
import saddle_inputs as si
import saddledef as sd
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
INTS = ("n_groups", "candidates", "kept", "cells_used", "chunks", "corner")


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
        self.nb, self.off, self.ex = nb, off, ex
        self.w = mx.weights(k) if use_weights else None

    def want(self, track, **opts):
        return sd.saddle(self.b1, self.b2, self.cnt, self.nb, self.off, track, weights=self.w, expected=self.ex.genome.expected,
                         expected_smooth=self.ex.genome.expected_smooth, trans_expected=self.ex.trans.expected, **opts)


def _bits(x):
    return struct.pack("<d", x)


def _compare(label, mx, k, info, want):
    got = mx.saddle_result(k)
    for f in sd.FIELDS:
        assert getattr(got, f).dtype == getattr(want, f).dtype and getattr(got, f).shape == getattr(want, f).shape, (label, f)
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), (label, f)
    for f in INTS:
        assert getattr(info, f) == want.info[f], (label, f, getattr(info, f), want.info[f])
    for f in sd.SCORES:
        assert _bits(getattr(info, f)) == _bits(want.info[f]), (label, f, getattr(info, f), want.info[f])
    for f in sd.TABLES:
        assert getattr(got, f).tobytes() == np.ascontiguousarray(getattr(got, f).T).tobytes(), (label, f)
    return got


def _check(label, mx, k, ref, track, **opts):
    want = ref.want(track, **opts)
    return _compare(f"{label} {opts}", mx, k, mx.saddle(k, track, **opts), want), want


def _all_bytes(mx, k, track, **opts):
    info = mx.saddle(k, track, **opts)
    return b"".join([getattr(mx.saddle_result(k), f).tobytes() for f in sd.FIELDS] + [_bits(getattr(info, f)) for f in sd.SCORES])


def _result_bytes(mx, k):
    return b"".join(getattr(mx.saddle_result(k), f).tobytes() for f in sd.FIELDS)


# ---- 1. chunk edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", sorted(si.CHUNK_CASES))
def test_chunk_edges(ncells):
    _need_gpu()
    ttext, text, off, nb, cells, track = si.chunk_matrix(ncells)
    with _loaded(text, [si.R], ttext) as mx:
        assert (np.stack(mx.cells(0), axis=1) == cells).all() and mx.info(0)[1] == ncells
        for balanced in (False, True) if ncells > 1 else (False,):
            if balanced:
                mx.balance(0, min_nnz=1, mad_max=0)
            ref = Ref(mx, 0, nb, off, mx.expected(0, use_weights=balanced), balanced)
            for ci, contact in enumerate(sd.CONTACTS):
                for kind in sd.KINDS:
                    o = dict(n_groups=5, trim_lo=0, trim_hi=0, contact=contact, kind=kind, min_diag=si.CHUNK_MIN_DIAG)
                    got, want = _check(f"chunks {ncells} balanced={balanced}", mx, 0, ref, track, **o)
                    assert want.info["chunks"] == (ncells + sd.CHUNK - 1) // sd.CHUNK
                    if not balanced:                                          # every bin is valid: what the builder counted
                        assert si.chunk_entry_spans(cells, want.groups, off, nb, contact, 5) == si.CHUNK_CASES[ncells][ci]
                        assert want.info["cells_used"] == int(((cells[:, 1] >= 100) if ci else ((cells[:, 1] < 100) & (cells[:, 1] - cells[:, 0] >= 2))).sum())
                    elif ncells >= 4095:
                        assert want.info["cells_used"] > 1000
            s, t = mx.saddle_timing_ms(0)
            assert s > 0 and t > 0


# ---- 2. groups -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [2, 3, 5, 50, 63, 64])
def test_groups(Q):
    _need_gpu()
    ttext, text, off, nb, cells, _ = li.edge_matrix(False)
    tracks = si.group_tracks()
    every = np.ones(nb, dtype=bool)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        ref = Ref(mx, 0, nb, off, mx.expected(0, use_weights=False), False)
        for name, track in tracks.items():
            for tl, th in ((0, 0), (250, 250), (4000, 4500)):
                for contact in ("cis", "trans") if (name, tl) == ("full", 0) else ("cis",):
                    got, want = _check(f"{name} Q={Q}", mx, 0, ref, track, n_groups=Q, trim_lo=tl, trim_hi=th, contact=contact, min_diag=1)
                empty = si.empty_groups(track, every, Q, tl, th)
                assert int((got.group_bins == 0).sum()) == empty
                if name == "nan":                                             # no candidate: zero tables, NaN means and scores, and no error
                    assert want.info["kept"] == 0 and empty == Q and (got.groups == 255).all()
                    assert not got.n.any() and not got.nnz.any() and not got.vsum.any() and np.isnan(got.mean).all() and np.isnan(got.strength).all()
                elif name == "few":
                    assert want.info["candidates"] == 40 and (empty > 0) == (want.info["kept"] < Q or Q > 40)
                    assert Q < 50 or empty >= Q - 40
                elif name == "full" and tl == 4000:
                    assert want.info["kept"] == 181 - 72 - 81 and (Q < 50 or empty > 0)      # 28 bins: K < Q
                elif name in ("constant", "zeros") and tl == 0:
                    assert want.info["kept"] == nb and want.info["cells_used"] > 4000
                    g = got.groups.astype(np.int64)
                    if name == "constant":
                        assert (np.diff(g) >= 0).all()                        # one long tie: the groups follow the bins
                    else:
                        z = np.flatnonzero(track == 0)
                        assert (np.diff(g[z]) >= 0).all() and g[5] == 0 and g[77] == Q - 1      # -0.0 and 0.0 are one tie; the infinities at the ends


# ---- 3. chromosome edges and diagonals -------------------------------------------------------------------------------------------------
def test_chromosome_edges_and_diagonals():
    _need_gpu()
    ttext, text, off, nb, cells, _ = li.edge_matrix(False)
    track = si.group_tracks()["full"]
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        ref = Ref(mx, 0, nb, off, mx.expected(0, use_weights=False), False)
        seen = set()
        for mn in (0, 1, 2):
            for mxd in (0, 1, 11, 12):
                if mxd and mxd < mn:
                    continue
                got, want = _check("edges", mx, 0, ref, track, n_groups=4, trim_lo=0, trim_hi=0, min_diag=mn, max_diag=mxd, kind="oe_smooth")
                brute = si.brute_positions(got.groups, off, nb, 4, "cis", mn, mxd)
                assert np.array_equal(np.triu(got.n), brute) and (got.nnz <= got.n).all() and brute.sum() > 0
                seen.add(int(brute.sum()))
        assert len(seen) == 11
        got, want = _check("edges", mx, 0, ref, track, n_groups=4, trim_lo=0, trim_hi=0, contact="trans")
        assert np.array_equal(np.triu(got.n), si.brute_positions(got.groups, off, nb, 4, "trans", 0, 0)) and got.nnz.sum() >= 3
        assert got.groups[0] != 255 and (got.groups[1:13] != 255).sum() == 11      # the one-bin and the 12-bin chromosome are ranked


# ---- 4. masked bins ---------------------------------------------------------------------------------------------------------------------
def test_masked_bins():
    _need_gpu()
    ttext, text, off, nb, cells, empty = li.edge_matrix(True)
    track = np.random.default_rng(41).standard_normal(nb)
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0)
        w = mx.weights(0)
        assert set(np.flatnonzero(np.isnan(w)).tolist()) == empty and len(empty) >= 5
        first, last = {off[c] for c in li.MASKED_LOCAL}, {off[c] + li.EDGE_BINS[c] - 1 for c in li.MASKED_LOCAL}
        assert empty & first and empty & last and empty - first - last        # first, last and interior bins
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        for o in (dict(n_groups=3, trim_lo=0, trim_hi=0, min_diag=0), dict(n_groups=6, min_diag=2, max_diag=30, kind="oe_smooth"), dict(n_groups=3, trim_lo=0, trim_hi=0, contact="trans")):
            got, want = _check("masked", mx, 0, ref, track, **o)
            assert (got.groups[sorted(empty)] == 255).all() and want.info["candidates"] == nb - len(empty)
            c = "trans" if o.get("contact") == "trans" else "cis"
            brute = si.brute_positions(got.groups, off, nb, o["n_groups"], c, o.get("min_diag", 2), o.get("max_diag", 0))
            assert np.array_equal(np.triu(got.n), brute)
            unmasked = sd.groups(track, np.ones(nb, dtype=bool), o["n_groups"], o.get("trim_lo", 250), o.get("trim_hi", 250))[0]
            assert si.brute_positions(unmasked, off, nb, o["n_groups"], c, o.get("min_diag", 2), o.get("max_diag", 0)).sum() > brute.sum()


# ---- 5. exact sanity ------------------------------------------------------------------------------------------------------------------------
def test_flat_matrix_is_one_everywhere():
    _need_gpu()
    ttext, text, off, nb, cells, track = si.flat()
    with _loaded(text, [li.R_EDGE], ttext) as mx:
        ref = Ref(mx, 0, nb, off, mx.expected(0, use_weights=False), False)
        for Q, mn in ((2, 0), (5, 2), (7, 1)):
            for kind in sd.KINDS:
                got, want = _check("flat", mx, 0, ref, track, n_groups=Q, trim_lo=0, trim_hi=0, min_diag=mn, kind=kind)
                assert (got.n > 0).sum() >= Q * Q - 2 and (got.mean[got.n > 0] == 1.0).all() and np.isnan(got.mean[got.n == 0]).all()
                for x in (got.strength, got.aa_ab, got.bb_ab):
                    assert (x[~np.isnan(x)] == 1.0).all()
                assert got.strength[-1] == 1.0


def test_planted_compartments():
    _need_gpu()
    ttext, text, off, nb, cells, track = gi.planted()
    with _loaded(text, [gi.R], ttext) as mx:
        mx.balance(0)
        ref = Ref(mx, 0, nb, off, mx.expected(0), True)
        e = mx.eigs(0, phasing=track)
        for Q in (4, 5):
            o = dict(n_groups=Q, trim_lo=0, trim_hi=0)
            info = mx.saddle_eigs(0, 0, **o)
            by_eigs = _result_bytes(mx, 0) + b"".join(_bits(getattr(info, f)) for f in sd.SCORES)
            res = mx.saddle_result(0)
            assert info.kept >= 64 + 128 - 4 and (res.aa_ab > 1).all() and (res.bb_ab > 1).all() and (res.strength > 1).all(), (Q, res.strength, res.aa_ab, res.bb_ab)
            assert info.aa_ab > 1 and info.bb_ab > 1 and info.strength > 1
            assert _all_bytes(mx, 0, e.vectors[0], **o) == by_eigs            # the same bytes as saddle() with the fetched vector
            _compare("planted", mx, 0, mx.saddle(0, e.vectors[0], **o), ref.want(e.vectors[0], **o))
        with pytest.raises(m.MktError):
            mx.saddle_eigs(0, 7)                                              # no such vector


# ---- 6. the same bits on a second call, by the device-text route and in a fresh process ---------------------------------------------------
def test_same_bits_by_every_route(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells, track = si.chunk_matrix(8193)
    o = dict(n_groups=7, contact="trans")
    with _loaded(text, [si.R], ttext) as mx:
        mx.balance(0, min_nnz=1, mad_max=0)
        mx.expected(0)
        first = _all_bytes(mx, 0, track, **o)
        assert _all_bytes(mx, 0, track, **o) == first and mx.saddle_result(0).nnz.sum() > 5000
    from microcket_amd import capi
    hip = C.CDLL(capi.hip_runtimes()[0])                                      # the runtime the library itself uses
    d_text = C.c_void_p()
    with m.Matrix(ttext, [si.R], device=0) as mx:
        assert hip.hipMalloc(C.byref(d_text), C.c_size_t(len(text))) == 0
        try:
            assert hip.hipMemcpy(d_text, text, C.c_size_t(len(text)), 1) == 0 # hipMemcpyHostToDevice
            mx.add_device(d_text.value, len(text))
        finally:
            hip.hipFree(d_text)
        mx.run()
        mx.balance(0, min_nnz=1, mad_max=0)
        mx.expected(0)
        assert _all_bytes(mx, 0, track, **o) == first
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    np.save(tmp_path / "track.npy", track)
    script = ("import sys, struct, numpy as np, microcket_amd as m\n"
              "mx = m.Matrix(open(sys.argv[1], 'rb').read(), [%d])\n"
              "mx.add(open(sys.argv[2], 'rb').read()); mx.run(); mx.balance(0, min_nnz=1, mad_max=0); mx.expected(0)\n"
              "info = mx.saddle(0, np.load(sys.argv[3]), n_groups=7, contact='trans')\n"
              "r = mx.saddle_result(0)\n"
              "parts = [a.tobytes() for a in r] + [struct.pack('<d', x) for x in (info.strength, info.aa_ab, info.bb_ab)]\n"
              "open(sys.argv[4], 'wb').write(b''.join(parts)); mx.close()\n" % si.R)
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", script, str(tmp_path / "g.sizes"), str(tmp_path / "in.pairs"), str(tmp_path / "track.npy"), str(tmp_path / "out")], env=env,
                       cwd=util.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "out", "rb").read() == first


# ---- 7. state, argument and discard errors -------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
    _need_gpu()
    ttext, text, off, nb, cells = li.band_matrix()
    track = np.random.default_rng(3).standard_normal(nb)
    with m.Matrix(ttext, [li.R_EDGE, 5 * li.R_EDGE]) as mx:
        with pytest.raises(m.MktError, match="saddle before run"):
            mx.saddle(0, track)
        mx.add(text)
        mx.run()
        with pytest.raises(m.MktError, match="expected first"):
            mx.saddle(0, track)
        with pytest.raises(m.MktError, match="saddle first"):
            mx.saddle_result(0)
        assert mx.saddle_timing_ms(0) == (0.0, 0.0)
        assert mx.L.mkt_matrix_saddle_timing(mx.h, 2, None, None) != 0         # a bad index, without a message
        mx.balance(0, min_nnz=1)
        ex = mx.expected(0)
        ref = Ref(mx, 0, nb, off, ex, True)
        o = dict(n_groups=6, trim_lo=100, trim_hi=0)
        info = mx.saddle(0, track, **o)
        kept = _result_bytes(mx, 0)
        assert info.cells_used > 1000
        with pytest.raises(m.MktError, match="expected first"):
            mx.saddle(1, np.zeros(mx.info(1)[0]))                             # the other resolution has no tables
        with pytest.raises(m.MktError, match="resolution index"):
            mx._chk(mx.L.mkt_matrix_saddle(mx.h, 2, None, track.ctypes.data_as(C.c_void_p), None), "saddle")
        for bad, what in ((dict(n_groups=1), "n_groups 1"), (dict(n_groups=65), "n_groups 65"), (dict(trim_lo=-1), "trim_lo -1"), (dict(trim_hi=-2), "trim_hi -2"),
                          (dict(trim_lo=5000, trim_hi=5000), "leaves nothing"), (dict(contact=2), "contact 2"), (dict(contact=-1), "contact -1"), (dict(kind=0), "kind 0"),
                          (dict(kind="balanced"), "kind 0"), (dict(kind=3), "kind 3"), (dict(corner=-1), "corner -1"), (dict(corner=26), "corner 26"),
                          (dict(n_groups=5, corner=3), "corner 3"), (dict(min_diag=-1), "min_diag -1"), (dict(max_diag=-2), "max_diag -2"),
                          (dict(min_diag=5, max_diag=4), "max_diag 4 is below min_diag 5")):
            with pytest.raises(m.MktError, match=what):
                mx.saddle(0, track, **bad)
        with pytest.raises(TypeError):
            mx.saddle(0, track, window=3)
        with pytest.raises(ValueError):
            mx.saddle(0, track, kind="raw")
        with pytest.raises(ValueError):
            mx.saddle(0, track[:-1])
        so = m.SaddleOpts()
        mx.L.mkt_saddle_opts_default(C.byref(so))
        pt = track.ctypes.data_as(C.c_void_p)
        so.reserved = 3
        with pytest.raises(m.MktError, match="reserved"):
            mx._chk(mx.L.mkt_matrix_saddle(mx.h, 0, C.byref(so), pt, None), "saddle")
        with pytest.raises(m.MktError, match="NULL"):
            mx._chk(mx.L.mkt_matrix_saddle(mx.h, 0, None, None, None), "saddle")
        assert _result_bytes(mx, 0) == kept                                   # a refused call leaves the results alone
        with pytest.raises(m.MktError, match="saddle groups of bins"):
            mx._chk(mx.L.mkt_matrix_fetch_saddle_groups(mx.h, 0, nb - 1, 2, None), "fetch")
        two = (C.c_uint8 * 2)()
        mx._chk(mx.L.mkt_matrix_fetch_saddle_groups(mx.h, 0, nb - 2, 2, two), "fetch")
        assert list(two) == mx.saddle_result(0).groups[-2:].tolist()
        mx._chk(mx.L.mkt_matrix_fetch_saddle(mx.h, 0, None, None, None, None, None), "fetch")      # any pointer may be NULL
        mx._chk(mx.L.mkt_matrix_fetch_saddle_edges(mx.h, 0, None, None, None), "fetch")
        mx._chk(mx.L.mkt_matrix_fetch_saddle_profile(mx.h, 0, None, None, None), "fetch")
        from microcket_amd.capi import _SaddleInfoC
        ic = _SaddleInfoC()
        mx._chk(mx.L.mkt_matrix_saddle(mx.h, 0, None, pt, C.byref(ic)), "saddle")                   # NULL options: the defaults
        want = ref.want(track)
        assert (ic.n_groups, ic.corner, ic.kept, ic.cells_used) == (50, 10, want.info["kept"], want.info["cells_used"]) and _bits(ic.strength) == _bits(want.info["strength"])
        mx._chk(mx.L.mkt_matrix_saddle(mx.h, 0, None, pt, None), "saddle")                          # ... and no info
        assert mx.L.mkt_abi_version() == 9
        _compare("defaults", mx, 0, mx.saddle(0, track), want)
        # loops, eigs, insulation, pileup and saddle of one resolution do not disturb each other
        a = np.arange(40, 340, 3)

        def other_bytes():
            v = np.zeros((2, nb), np.float64)
            for j in range(2):
                mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, j, 0, nb, v[j].ctypes.data_as(C.c_void_p)), "fetch")
            return b"".join([x.tobytes() for x in mx.loop_cells(0)] + [mx.loop_hist(0).tobytes(), v.tobytes(), mx.values(0, "oe").tobytes()] +
                            [getattr(mx.insulation_track(0, j), f).tobytes() for j in range(3) for f in m.InsulationTrack._fields] +
                            [getattr(mx.pileup_result(0), f).tobytes() for f in m.Pileup._fields])
        mx.saddle(0, track, **o)
        assert _result_bytes(mx, 0) == kept
        mx.loops(0)
        mx.eigs(0, n_eigs=2)
        mx.insulation(0)
        mx.pileup(0, a, a + 5, flank=3, corner=1)
        assert _result_bytes(mx, 0) == kept                                   # ... by loops, eigenvectors, insulation scores and a pileup
        others = other_bytes()
        mx.saddle(0, track, n_groups=3, contact="trans")
        mx.saddle_eigs(0, 1, n_groups=4)
        assert other_bytes() == others                                        # ... and those not by a saddle
        # a later balance, expected, run or add of that resolution discards the results
        line = text.splitlines(keepends=True)[0]
        for what, again in (("balance", lambda: mx.balance(0, min_nnz=1)), ("expected", lambda: mx.expected(0, use_weights=False)), ("run", lambda: mx.run()), ("add", lambda: mx.add(line))):
            mx.run()
            mx.balance(0, min_nnz=1)
            mx.expected(0)
            assert mx.saddle(0, track).cells_used > 1000 and mx.saddle_timing_ms(0)[1] > 0
            again()
            with pytest.raises(m.MktError, match="saddle first"):
                mx.saddle_result(0)
            assert mx.saddle_timing_ms(0) == (0.0, 0.0), what


# ---- 8. the executable ---------------------------------------------------------------------------------------------------------------------------
def test_executable_writes_the_saddle(tmp_path):
    _need_gpu()
    ttext, text, off, nb, cells, track = gi.planted()
    (tmp_path / "g.sizes").write_bytes(ttext)
    (tmp_path / "in.pairs").write_bytes(text)
    for d in "ab":
        os.makedirs(tmp_path / d)
    run = lambda d, *a: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", str(gi.R), "-o", str(tmp_path / d / "o"), "--eigs", *a, str(tmp_path / "in.pairs")],
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    sub = ["--saddle-groups", "5", "--saddle-trim", "0,100", "--saddle-kind", "oe-smooth", "--saddle-min-dist", str(3 * gi.R), "--saddle-max-dist", str(60 * gi.R), "--saddle-corner", "2"]
    runs = [run("a"), run("b", "--saddle", *sub)]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted(os.listdir(tmp_path / "a"))
    assert f"o.{gi.R}.eigs.tsv" in plain and not any("saddle" in f for f in plain)      # without the flag no new file appears ...
    assert sorted(os.listdir(tmp_path / "b")) == sorted(plain + [f"o.{gi.R}.saddle.tsv", "o.saddle.stat"])
    for f in plain:                                                           # ... and the flag changes none of the other bytes
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read(), f
    num = lambda s: float(s)                                                  # "nan" round-trips through float()
    with _loaded(text, [gi.R], ttext) as mx:
        mx.expected(0, use_weights=False)
        mx.eigs(0)
        info = mx.saddle_eigs(0, 0, n_groups=5, trim_lo=0, trim_hi=100, kind="oe_smooth", min_diag=3, max_diag=60, corner=2)
        res = mx.saddle_result(0)
    lines = open(tmp_path / "b" / f"o.{gi.R}.saddle.tsv", "rb").read().decode().splitlines()
    assert lines[0].split("\t") == ["a", "b", "n", "nnz", "csum", "vsum", "mean"] and len(lines) == 1 + 15
    t = [x.split("\t") for x in lines[1:]]
    pairs = [(a, b) for a in range(5) for b in range(a, 5)]
    assert [(int(x[0]), int(x[1])) for x in t] == pairs
    for col, arr in ((2, res.n), (3, res.nnz), (4, res.csum)):
        assert [int(x[col]) for x in t] == [int(arr[a][b]) for a, b in pairs], col
    for col, arr in ((5, res.vsum), (6, res.mean)):                           # %.17g round-trips
        assert np.array([num(x[col]) for x in t]).tobytes() == np.array([arr[a][b] for a, b in pairs]).tobytes(), col
    stat = [x.split("\t") for x in open(tmp_path / "b" / "o.saddle.stat", "rb").read().decode().splitlines()]
    assert [x[1] for x in stat] == ["info"] + ["group"] * 5 + ["profile"] * 2 and all(x[0] == str(gi.R) for x in stat)
    assert [int(x) for x in stat[0][2:8]] == [info.n_groups, info.candidates, info.kept, info.cells_used, info.chunks, info.corner]
    assert b"".join(_bits(num(x)) for x in stat[0][8:]) == b"".join(_bits(getattr(info, f)) for f in sd.SCORES)
    assert [int(x[3]) for x in stat[1:6]] == res.group_bins.tolist() and [int(x[2]) for x in stat[1:6]] == list(range(5))
    assert np.array([num(x[4]) for x in stat[1:6]]).tobytes() == res.group_lo.tobytes() and np.array([num(x[5]) for x in stat[1:6]]).tobytes() == res.group_hi.tobytes()
    assert [int(x[2]) for x in stat[6:]] == [1, 2]
    for col, arr in ((3, res.strength), (4, res.aa_ab), (5, res.bb_ab)):
        assert np.array([num(x[col]) for x in stat[6:]]).tobytes() == arr.tobytes()
    assert info.corner == 2 and info.cells_used > 1000 and info.strength > 1
