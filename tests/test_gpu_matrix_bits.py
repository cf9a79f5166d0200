"""The bits of the matrix analyses (balance, expected, values, loops, eigs) against tests/golden/matrix_bits.json: sha256 digests of the
raw bytes of every output, recorded once by tests/golden/make_matrix_bits.py.  The tests of balance and eigs allow a rounding bound, so
this is what pins the order of the shared reduction trees, the grouping and the cell layout: a change that keeps the definitions but
moves one addition shows here.

The inputs are drawn here from a seed, the smallest that reach every shared path:
  width  five densities on one 200-bin table of two chromosomes: the two lane-width rules, 2 nnz / nbins (bins) and
         nnz / (nbins + nchr (nchr - 1) / 2) (segments), differ by a factor of two on one table, so four densities cannot put both into all
         four classes; five do (the test checks it);
  long   a chromosome of 1 100 bins whose bin 0 has a cell with every bin (row + column above 1 024: the long-bin workgroups of balance
         and eigs), a second one of 70 bins dense against the first 70 bins of the first (a trans segment of more than 4 096 cells: a long
         segment of two chunks), and five bins with one contact each, which the default balance masks (NaN weights);
  band   the band of the loop tests (loops_inputs.band_matrix) with its isolated peak of 3 000 contacts: the only input whose counts
         reach a threshold, so the only one that pins the enriched list, the gather of the peaks and the clustering (the test checks
         that it calls a loop).
Every input runs the same sequence on one matrix object: raw counts first (use_weights = 0), where the loops are called before anything
has built the transposed half of the layout, then the default balance and everything again with the weights."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import expected_inputs as xi
import loops_inputs as li

R = 1000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_bits.json")
WIDTH_BINS = [150, 50]
WIDTH_CELLS = {"width_1000": 1000, "width_2000": 2000, "width_3500": 3500, "width_7000": 7000, "width_12000": 12000}
LONG_BINS = [1100, 70]
LONG_MASKED = (600, 601, 602, 603, 604)
CASES = sorted(WIDTH_CELLS) + ["long", "band"]
EIGS_OPTS = dict(max_iters=40)


def lanes(avg):
    return 64 if avg >= 48 else 32 if avg >= 24 else 16 if avg >= 12 else 8


def _finish(bins, cell):
    rows, ttext, trows = li.table_of(bins, R)
    off, nb = xi.offsets(R, trows)
    keys = sorted(cell)
    text = li.text_of(rows, R, off, [k[0] for k in keys], [k[1] for k in keys], [cell[k] for k in keys])
    return ttext, text, nb, len(bins), len(keys)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> (table text, .pairs text, nbins, chromosomes, cells)"""
    if case == "band":
        ttext, text, _off, nb, cells = li.band_matrix()
        return ttext, text, nb, 1, len(cells)
    if case == "long":
        rng = np.random.default_rng(41)
        n0, n1 = LONG_BINS
        cell = {}
        for x in range(n0 + n1):
            if x in LONG_MASKED:
                continue
            end = n0 if x < n0 else n0 + n1
            for y in range(x, min(end, x + 13)):
                if y not in LONG_MASKED and rng.random() < 0.8:
                    cell[(x, y)] = int(rng.integers(1, 5))
        for y in range(n0 + n1):                                             # bin 0 with every bin
            cell[(0, y)] = int(rng.integers(1, 4))
        for x in range(70):                                                  # one trans block of 4 900 cells
            for y in range(n0, n0 + n1):
                cell[(x, y)] = int(rng.integers(1, 3))
        return _finish(LONG_BINS, cell)
    rng = np.random.default_rng(1000 + WIDTH_CELLS[case])
    nb = sum(WIDTH_BINS)
    i, j = np.triu_indices(nb)
    pick = rng.choice(i.size, WIDTH_CELLS[case], replace=False)
    cnt = rng.integers(1, 4, pick.size)
    return _finish(WIDTH_BINS, {(int(i[p]), int(j[p])): int(c) for p, c in zip(pick.tolist(), cnt.tolist())})


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digests(case):
    """{output: sha256 of its raw bytes} of one input, raw counts first and then with the weights"""
    import microcket_amd as m
    ttext, text, nb, _nchr, nnz = inputs(case)
    out = {}
    with m.Matrix(ttext, [R], device=0) as mx:
        mx.add(text)
        mx.run()
        assert mx.info(0)[:2] == (nb, nnz)
        for tag, use_weights in (("raw", False), ("w", True)):
            if use_weights:
                mx.balance(0)
                out["weights"] = _sha(mx.weights(0))
                if case == "long":
                    assert np.isnan(mx.weights(0)[list(LONG_MASKED)]).all()
            ex = mx.expected(0, use_weights=use_weights)
            out[tag + ".cis"] = _sha(*ex.cis)
            out[tag + ".trans"] = _sha(*ex.trans)
            out[tag + ".genome"] = _sha(*ex.genome)
            out[tag + ".oe_smooth"] = _sha(mx.values(0, "oe_smooth"))
            lp = mx.loops(0)                                                 # raw: no balance and no eigs has run yet, the row pointers alone
            if case == "band":
                assert len(lp.loops) > 0 and lp.info.enriched > 0
            out[tag + ".loop_cells"] = _sha(*mx.loop_cells(0))
            out[tag + ".loop_hist"] = _sha(mx.loop_hist(0))
            out[tag + ".loop_thresholds"] = _sha(mx.loop_thresholds(0))
            out[tag + ".loops"] = _sha(np.array([[x.cell, x.bin1, x.bin2, x.count, x.window, x.n_cells, *x.box] for x in lp.loops], dtype=np.uint64),
                                       np.array([x.r for x in lp.loops], dtype=np.float64))
            eg = mx.eigs(0, **EIGS_OPTS)
            out[tag + ".eigvecs"] = _sha(eg.vectors)
            out[tag + ".eigvals"] = _sha(eg.lambdas)
            out[tag + ".resid"] = _sha(eg.resid)
    return out


def test_inputs_reach_every_width():
    """both lane-width rules land in all four classes, and the long input has its long bin, its long segment and its masked bins"""
    bins, segs = set(), set()
    for case in CASES:
        _t, _x, nb, nchr, nnz = inputs(case)
        bins.add(lanes(2 * nnz // nb))
        segs.add(lanes(nnz // (nb + nchr * (nchr - 1) // 2)))
    assert bins == {8, 16, 32, 64} and segs == {8, 16, 32, 64}
    assert sum(LONG_BINS) > 1024 and 70 * LONG_BINS[1] > 4096               # kBalLong; kExpChunk: two chunks


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_bits(case):
    import microcket_amd as m
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = digests(case)
    diff = sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))
    print(case, "differs in:", diff)
    assert got == want, diff
