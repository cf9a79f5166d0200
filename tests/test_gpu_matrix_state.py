"""Which results of a matrix object die when: the whole table at once, through the fetches.

    trigger          ends
    expected again   loops, eigs, pileup, saddle (the tables themselves are made anew)
    balance again    + the expected tables, insulation, scc (the weights themselves are made anew)
    add + run        + the weights, and the per-object viewpoint profile and .hic file

What a trigger does not end still fetches, with the bytes it had.  The per-analysis tests (test_gpu_loops, test_gpu_eigs, ...) pin
each "X first" message on its own; this one pins that no trigger takes too much or too little.  One matrix of 40 bins (chromosomes
of 25 and 15 bins, one resolution) with about 500 pairs near the diagonal and a dozen between the chromosomes: everything succeeds
on it, nothing is compared with a definition here."""
import ctypes as C

import numpy as np
import pytest

import microcket_amd as m

pytestmark = pytest.mark.gpu

R = 1000
BINS = (("a", 25), ("b", 15))
TABLE = "".join(f"{n}\t{k * R}\n" for n, k in BINS).encode()
NB = sum(k for _, k in BINS)
TRACK = np.sin(0.7 * np.arange(NB))


def _pairs():
    out = []
    for name, n in BINS:
        for i in range(n):
            for d in range(min(6, n - i)):
                out.append(f"q\t{name}\t{i * R + 7}\t{name}\t{(i + d) * R + 9}\t+\t-\n" * (1 + (3 * i + 5 * d) % 3 + (2 if d == 0 else 0)))
    for i in range(0, 24, 2):
        out.append(f"q\ta\t{i * R + 7}\tb\t{(4 * i) % 15 * R + 9}\t+\t-\n")
    return "".join(out).encode()


TEXT = _pairs()


def _flat(x):
    """the bytes of a result: an array, or a tuple of arrays and plain values"""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (tuple, list)):
        return b"|".join(_flat(y) for y in x)
    return repr(x).encode()


def _eigvec(mx):
    v = np.zeros(NB)
    mx._chk(mx.L.mkt_matrix_fetch_eigvecs(mx.h, 0, 0, 0, NB, v.ctypes.data_as(C.c_void_p)), "fetch")
    return v


def _tables(mx):
    cols = [np.zeros(NB, np.uint64), np.zeros(NB, np.uint64), np.zeros(NB, np.float64)]
    mx._chk(mx.L.mkt_matrix_fetch_expected_cis(mx.h, 0, 0, NB, *[a.ctypes.data_as(C.c_void_p) for a in cols]), "fetch")
    return cols


# name -> (the fetch, the message of a fetch without results, the timing getter or None)
FETCH = {
    "weights": (lambda mx: mx.weights(0), "balance first", lambda mx: mx.balance_timing_ms(0)),
    "tables": (_tables, "expected first", lambda mx: mx.expected_timing_ms(0)),
    "loops": (lambda mx: (mx.loop_hist(0), mx.loop_cells(0)), "loops first", lambda mx: mx.loops_timing_ms(0)),
    "eigs": (_eigvec, "eigs first", lambda mx: mx.eigs_timing_ms(0)),
    "insulation": (lambda mx: mx.insulation_track(0, 1), "insulation first", lambda mx: mx.insulation_timing_ms(0)),
    "pileup": (lambda mx: mx.pileup_result(0), "pileup first", lambda mx: mx.pileup_timing_ms(0)),
    "saddle": (lambda mx: mx.saddle_result(0), "saddle first", lambda mx: mx.saddle_timing_ms(0)),
    "scc": (lambda mx: mx.scc_result(0), "scc first", lambda mx: mx.scc_timing_ms(0)),
    "viewpoint": (lambda mx: mx.viewpoint_result()[:-1], "viewpoint first", lambda mx: mx.viewpoint_timing_ms()),
    "hic": (lambda mx: mx.hic_bytes(), "hic first", None),
    "cells": (lambda mx: (mx.cells(0), mx.text(0)), "fetch before run", None),
}
PER_RESOLUTION = ("tables", "loops", "eigs", "insulation", "pileup", "saddle", "scc")


def _compute_all(mx):
    mx.balance(0, min_nnz=1, mad_max=0.0)
    mx.expected(0)
    mx.loops(0)
    mx.eigs(0, n_eigs=1, min_good=4)                                          # small chromosomes: a small min_good
    mx.insulation(0, windows=(2, 4))
    mx.pileup(0, [5, 28], [9, 31], flank=2, corner=1)
    mx.saddle(0, TRACK, n_groups=4)
    mx.scc(mx, 0, h=1)
    mx.viewpoint("a")
    mx.hic()
    return {k: _flat(f(mx)) for k, (f, _, _) in FETCH.items()}


def _check(mx, what, before, gone):
    for k, (f, msg, timing) in FETCH.items():
        if k in gone:
            with pytest.raises(m.MktError, match=msg):
                f(mx)
            if timing is not None:
                assert not any(timing(mx)), (what, k)
        elif k in before:
            assert _flat(f(mx)) == before[k], (what, k)
        else:
            f(mx)                                                             # made anew by the trigger itself: it fetches


def test_the_invalidation_table():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    with m.Matrix(TABLE, [R]) as mx:
        mx.add(TEXT)
        pairs, skipped = mx.run()
        assert (pairs, skipped) == (TEXT.count(b"\n"), 0) and mx.info(0)[0] == NB
        before = _compute_all(mx)
        for k, (_, _, timing) in FETCH.items():
            assert len(before[k]) > 0
            print(k, len(before[k]), timing(mx) if timing else "")

        mx.expected(0)
        kept = {k: v for k, v in before.items() if k != "tables"}
        _check(mx, "expected", kept, gone=("loops", "eigs", "pileup", "saddle"))
        assert _flat(_tables(mx)) == before["tables"]                         # the same weights, the same cells: the same tables

        before = _compute_all(mx)
        mx.balance(0, min_nnz=1, mad_max=0.0)
        kept = {k: v for k, v in before.items() if k in ("cells", "viewpoint", "hic")}
        _check(mx, "balance", kept, gone=PER_RESOLUTION)
        assert _flat(mx.weights(0)) == before["weights"]

        before = _compute_all(mx)
        mx.add(TEXT.splitlines(keepends=True)[0])
        mx.run()
        _check(mx, "add + run", {}, gone=PER_RESOLUTION + ("weights", "viewpoint", "hic"))
        assert _flat(FETCH["cells"][0](mx)) != before["cells"]                # one more pair
