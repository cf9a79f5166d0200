"""Contact-matrix binning (mkt_matrix.hip and the radix passes it shares with the duplicate marker) at the steps of its own
constants: key widths around whole 7-bit digits and 2^k - 1 / 2^k bins, the 256 / 2048-key head tiles, the 1024-cell text
workgroups and the 8192-record radix tiles, a full name table whose probe chains wrap, positions around 2^32, 2^40 and 2^64,
line shapes and the carry of a partial line, every digit count of the COO text, and the key route with a partial table.

The inputs and the restated constants are in matrix_edge_cases.py (with a pointer to each source line); its builders assert what
the definition (matrixdef.py) says about a case before it is run here, and test_matrix_edges_host.py runs them without a GPU.
Every comparison is exact: cells, COO bytes, pairs, skipped, info()."""
import ctypes as C

import numpy as np
import pytest

import matrix_edge_cases as ec
import matrixdef as md
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu


def _fetch(mx, case):
    """[(cells, text)] per resolution, with the invariants of test_gpu_matrix._fetch and nbins"""
    out = []
    for k, r in enumerate(case.res):
        b1, b2, c = mx.cells(k)
        cells = np.stack([b1, b2, c], axis=1).astype(np.uint64) if b1.size else np.zeros((0, 3), dtype=np.uint64)
        text = mx.text(k)
        nbins, nnz, tb = mx.info(k)
        assert nbins == case.nbins[r] and nnz == cells.shape[0] and tb == len(text), (r, nbins, nnz, tb)
        assert text == md.coo_text(cells), r                                # the arrays and the device-made text say the same
        if nnz:
            key = cells[:, 0] * np.uint64(1 << 32) + cells[:, 1]
            assert (key[1:] > key[:-1]).all() and (cells[:, 0] <= cells[:, 1]).all() and int(cells[:, 1].max()) < nbins and int(cells[:, 2].min()) >= 1
        out.append((cells, text))
    return out


def _check(mx, case, ran):
    """(pairs, skipped) of run(), the cells and the bytes against the definition; returns the COO texts"""
    pairs, skipped = ran
    got = _fetch(mx, case)
    assert (pairs, skipped) == (case.pairs, case.skipped)
    for k, r in enumerate(case.res):
        cells, sk = case.want[r]
        assert sk == skipped and int(got[k][0][:, 2].sum()) + skipped == pairs, r
        assert got[k][0].shape == cells.shape and (got[k][0] == cells).all(), (r, got[k][0][:5].tolist(), cells[:5].tolist())
        assert got[k][1] == md.coo_text(cells), r
    return [t for _, t in got]


def _run(case, pieces=None, again=False):
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    with m.Matrix(case.table, case.res, device=0) as mx:
        for p in (pieces if pieces is not None else [case.text]):
            mx.add(p)
        texts = _check(mx, case, mx.run())
        if again:                                                           # a second run of the same object: the same bytes
            assert mx.run() == (case.pairs, case.skipped) and [mx.text(k) for k in range(len(case.res))] == texts
    return texts


# ---- 1. key width -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ec.KEY_WIDTH_K)
def test_key_width_steps(k):
    for nbins in ec.key_width_nbins(k):
        _run(ec.key_width_case(nbins))


def test_sixteen_resolutions_share_one_record_list():
    _run(ec.many_resolutions_case(), again=True)


# ---- 2. tiles -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", ec.TILE_NV)
def test_tile_steps(nv):
    for extra in ec.TILE_EXTRA:
        for shape in ec.TILE_SHAPES:
            _run(ec.tile_case(nv, extra, shape), again=True)


@pytest.mark.parametrize("nnz", ec.TEXT_NNZ)
def test_text_workgroup_steps(nnz):
    _run(ec.text_nnz_case(nnz), again=True)


# ---- 3. the name table --------------------------------------------------------------------------------------------------------------
def test_full_name_table_with_wrapping_probe_chains():
    nc = ec.name_table_case()
    _run(nc.case)
    with pytest.raises(m.MktError, match="8192"):
        m.Matrix(nc.case.table + b"one_more\t10\n", [1000])


# ---- 4. positions and resolutions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(ec.POSITION_TABLES))
def test_positions_around_the_number_formats(which):
    _run(ec.positions_case(which))


# ---- 5. line shapes and carry ---------------------------------------------------------------------------------------------------------
def test_line_shapes_in_every_chunking():
    case = ec.line_shapes_case()
    texts = None
    for name, pieces in ec.chunkings(case.text).items():
        got = _run(case, pieces)
        texts = texts or got
        assert got == texts, name


def test_carry_across_runs_and_device_text():
    case = ec.line_shapes_case()
    text = case.text
    cut = text.index(b"id20\t")
    nothing = b"#only a header\nz\tchrQ\t1\tchrB\t1\nz\tchrB\t0\tchrB\t1\t+\t-"          # two skipped pairs, the second without its newline
    first = ec.text_case(ec.LINES_TABLE, case.res, nothing)
    both = ec.text_case(ec.LINES_TABLE, case.res, nothing + b"\n" + text[:cut])
    whole = ec.text_case(ec.LINES_TABLE, case.res, nothing + b"\n" + text)
    assert (first.pairs, first.skipped) == (2, 2) and first.want[100][0].shape[0] == 0 and whole.pairs == case.pairs + 2
    with m.Matrix(case.table, case.res, device=0) as mx:
        mx.add(nothing)
        assert mx.run() == (2, 2)                                           # a run that bins nothing (and flushes a line without newline)
        assert _check(mx, first, (2, 2)) == [b"", b""]
        mx.add(text[:cut - 3])                                              # ends inside a line
        mx.add(text[cut - 3:cut])
        _check(mx, both, mx.run())
        mx.add(text[cut:])                                                  # the last line has no newline: run() flushes it
        _check(mx, whole, mx.run())
        _check(mx, whole, mx.run())
    # device text: the same bytes; behind an incomplete host line: an error
    from microcket_amd import capi
    hip = C.CDLL(capi.hip_runtimes()[0])
    d_text = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_text), C.c_size_t(len(text))) == 0
    try:
        assert hip.hipMemcpy(d_text, text, C.c_size_t(len(text)), 1) == 0   # hipMemcpyHostToDevice
        with m.Matrix(case.table, case.res, device=0) as mx:
            mx.add_device(d_text.value, len(text))
            assert _check(mx, case, mx.run()) == _run(case)
        with m.Matrix(case.table, case.res, device=0) as mx:
            mx.add(b"id\tchrB\t5")
            with pytest.raises(m.MktError, match="incomplete host line"):
                mx.add_device(d_text.value, len(text))
    finally:
        hip.hipFree(d_text)


def test_crlf_lines():
    case = ec.line_shapes_case()
    seven = b"".join(l + b"\n" for l in case.text.split(b"\n") if l.startswith(b"#") or len(l.split(b"\t")) >= 7)
    unix = ec.text_case(ec.LINES_TABLE, case.res, seven)
    dos = ec.text_case(ec.LINES_TABLE, case.res, seven.replace(b"\n", b"\r\n"))
    assert unix.pairs == dos.pairs == 20 and unix.skipped == dos.skipped and unix.want[100][0].shape[0] > 5
    assert _run(unix) == _run(dos)
    five = case.text.replace(b"\n", b"\r\n")                                # pos2 of a five-column line ends in '\r': not a number
    with pytest.raises(ValueError):
        md.definition(case.table, case.res, five)
    with m.Matrix(case.table, case.res, device=0) as mx:
        mx.add(five)
        with pytest.raises(m.MktError, match="not .pairs text"):
            mx.run()


# ---- 6. the digits of the COO text ----------------------------------------------------------------------------------------------------
def test_coo_digits_and_text_alignment():
    case, starts = ec.coo_digits_case()
    text = _run(case)[0]
    lines = text.split(b"\n")
    assert [len(b"\n".join(lines[:g * ec.MX_CPW])) + (1 if g else 0) for g in range(len(starts))] == starts


# ---- 7. the key route with a table that lacks chromosomes ------------------------------------------------------------------------------
def test_context_keys_with_a_partial_table():
    from test_gpu_matrix import HG38
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    res = [100000, 1000]
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS) as c:
        p, _s, st, _log = c.run_bytes(util.synth("unc", 67, 6000), chunk=1 << 20)
        rows, halved, gone = ec.partial_table([(nm.encode(), L) for nm, L in HG38], p)
        total, dups, flags = c.ext_dedup(True)
        for fl in (None, flags):
            case = ec.text_case(rows, res, p)
            want = md.definition(case.table, res, p, fl)
            n = md.n_pairs(p, fl)
            sk = want[res[0]][1]
            assert n == st.pairs - (dups if fl is not None else 0) and 0 < sk < n and n > 1000      # some skipped, most binned
            case = case._replace(want=want, pairs=n, skipped=sk)
            with m.Matrix(case.table, res, device=0) as mx:
                mx.add_keys(c, True, fl)
                _check(mx, case, mx.run())
