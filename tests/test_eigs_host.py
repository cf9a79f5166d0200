"""The compartment-eigenvector checker itself (tests/eigsdef.py) and its inputs, without a GPU: apply against the dense product, the
conditions every planted input has to meet, and the binding of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import eigs_inputs as gi
import eigsdef as gd
import expecteddef as ed
from test_loops_host import _small

PLANTED_OPTS = (dict(), dict(n_eigs=1), dict(clip=1.5), dict(ignore_diags=0))


@pytest.mark.parametrize("ig", [0, 1, 2, 3])
@pytest.mark.parametrize("clip", [0.0, 1.2])
def test_apply_against_the_dense_product(ig, clip):
    dense, b1, b2, cnt, off, nb, w = _small(2, (0, 17, 39, 41))
    E = ed.expected(b1, b2, cnt, nb, off, weights=w).genome.expected_smooth
    chs = gd.chromosomes(b1, b2, cnt, nb, off, E, weights=w, ignore_diags=ig, clip=clip, min_good=9)
    assert [c.skipped for c in chs] == [False, True, False] and not chs[0].good[[0, 17, 39]].any() and chs[0].good.sum() == 37
    x = np.random.default_rng(ig).standard_normal((nb, 8))
    y = gd.apply(chs, nb, x, ignore_diags=ig)
    bound = gd.apply_bound(chs, nb, x, ignore_diags=ig)
    for ch in chs:
        want = np.zeros((ch.hi - ch.lo, 8)) if ch.skipped else ch.A @ np.where(ch.good[:, None], x[ch.lo:ch.hi], 0.0)
        assert (ch.A == ch.A.T).all() and (ch.A[~ch.good] == 0).all()
        assert (np.abs(y[ch.lo:ch.hi] - want) <= bound[ch.lo:ch.hi]).all()
        assert (y[ch.lo:ch.hi][~ch.good] == 0).all()
        if clip > 0 and not ch.skipped:
            assert ch.A.max() <= clip - 1.0 and (ch.S == clip).any()
    assert (np.abs(gd.apply(chs, nb, x[:, 0], ignore_diags=ig) - y[:, 0]) <= bound[:, 0]).all()      # one column alone


@pytest.mark.parametrize("opts", PLANTED_OPTS, ids=str)
def test_planted_inputs_meet_the_conditions(opts):
    ttext, text, off, nb, cells, track = gi.planted()
    b1, b2, c = cells[:, 0], cells[:, 1], cells[:, 2]
    E = ed.expected(b1, b2, c, nb, off).genome.expected_smooth
    o = gd.options(**opts)
    ne = o["n_eigs"]
    chs = gd.chromosomes(b1, b2, c, nb, off, E, **opts)
    assert [ch.skipped for ch in chs] == [False, True, False]
    for ch in chs:
        if ch.skipped:
            continue
        lam, vec = gd.reference_eigs(ch, ne, track)
        a = np.abs(lam)
        assert all(a[j] >= 1.25 * a[j + 1] for j in range(ne)), lam[:5]
        assert a[ne - 1] >= 1.5 * a[8], lam[:9]
        it, conv, l2, V = gd.block_iteration(ch, **o)
        assert conv and it <= o["max_iters"] // 4, it
        assert np.allclose(np.abs(l2), a[:ne], rtol=1e-6)
        p, g = track[ch.lo:ch.hi], ch.good
        have = g & ~np.isnan(p)
        for j in range(ne):
            assert abs(np.corrcoef(vec[j][have], p[have])[0, 1]) >= 0.1
            top = np.sort(np.abs(vec[j][g]))[-2:]
            assert top[1] >= top[0] * (1 + 1e-6)
            plain = gd.orient(vec[j], g)
            assert plain[int(np.nanargmax(np.abs(plain)))] > 0 and np.sum(vec[j][have] * (p[have] - p[have].mean())) > 0


def test_orientation_rule():
    g = np.array([True, True, False, True])
    x = np.array([0.5, -0.5, np.nan, 0.25])
    assert gd.orient(x, g)[0] == 0.5 and gd.orient(-x, g)[0] == 0.5          # ties go to the lowest bin
    p = np.array([0.0, 1.0, 5.0, np.nan])
    assert gd.orient(x, g, p)[1] == 0.5                                       # the sum over bins 0 and 1 is negative: flipped
    assert gd.orient(x, g, np.full(4, np.nan))[0] == 0.5                      # no term: the fall-back
    assert gd.orient(x, g, np.array([1.0, 1.0, 0.0, 1.0]))[0] == 0.5          # exactly 0: the fall-back


def test_binding_lists_the_entry_points():
    from microcket_amd import capi
    names = ["mkt_eigs_opts_default", "mkt_matrix_eigs", "mkt_matrix_fetch_eigvecs", "mkt_matrix_fetch_eigvals", "mkt_matrix_eigs_apply", "mkt_matrix_eigs_timing"]
    assert all(n in capi.EXPORTS for n in names)
    o = capi.EigsOpts
    assert [(f[0], getattr(o, f[0]).offset) for f in o._fields_] == [("n_eigs", 0), ("ignore_diags", 4), ("min_good", 8), ("max_iters", 12), ("tol", 16), ("clip", 24),
                                                                       ("reserved", 32)]
    assert C.sizeof(o) == 40 and C.sizeof(capi._EigsInfoC) == 20
    assert all(hasattr(capi.Matrix, n) for n in ("eigs", "eigs_apply", "eigs_timing_ms"))
