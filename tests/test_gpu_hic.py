"""The .hic container from the GPU (mkt_matrix_hic, Matrix.hic / hic_bytes / write_hic, pairs2matrix --hic) against tests/hicdef.py.
One rule for every case (_check): the file parses with every position, size and nBytes accounted for; the header and the matrix records
apart from positions and sizes, every INFLATED payload, the footer keys and the vectors are hicdef.build's byte for byte; every stream
inflates with zlib and with tests/inflatedef.py; the decoded cells are Matrix.cells(res).  The deflated bytes themselves are the GPU's
own (a greedy one-pass parse) and are only required to inflate to the payload.
Not covered here: a pair with cells at one resolution only (an object bins the same pairs at every resolution; tests/test_hic_host.py
has it), and a payload so random that whole pieces are stored at level 2 (a count is that many input lines; the stored form inside a
stream is pinned on the 4-byte last piece of the 65284-byte payload instead)."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import microcket_amd as m
import util
import hic_cases as hc
import hicdef as hd
import inflatedef

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
MKT_E_ARG = -1


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")


def _loaded(case):
    mx = m.Matrix(case.table, case.resolutions, device=0)
    mx.add(case.text())
    mx.run()
    return mx


def _streams(stream):
    """a zlib stream of the GPU: header, deflate blocks by inflatedef, trailer; returns (blocks, payload)"""
    assert stream[:2] == b"\x78\x9c"
    blocks, out = inflatedef.inflate(stream[2:-4])
    assert struct.unpack(">I", stream[-4:])[0] == zlib.adler32(out)
    assert [b.bfinal for b in blocks] == [0] * (len(blocks) - 1) + [1]
    assert blocks[-1].btype == 1 and blocks[-1].tokens == [], "the stream ends with the empty fixed block 03 00"
    return blocks, bytes(out)


def _check(mx, case, weights=None, **more):
    opts = dict(case.opts, **more)
    info = mx.hic(**opts)
    got = mx.hic_bytes()
    assert len(got) == info["file_bytes"]
    cells = [list(zip(*[a.tolist() for a in mx.cells(k)])) for k in range(len(case.resolutions))]
    want = hd.build(case.chroms, case.resolutions, cells, weights, {k: v for k, v in opts.items() if k != "level"})
    P, Q = hd.parse(got), hd.parse(want)
    assert P["header"]["bytes"][:8] + P["header"]["bytes"][16:] == Q["header"]["bytes"][:8] + Q["header"]["bytes"][16:]       # (all but footerPosition)
    assert P["footer"]["keys"] == Q["footer"]["keys"]
    assert [(a, b, c, d) for a, b, c, d, _, _ in P["footer"]["index"]] == [(a, b, c, d) for a, b, c, d, _, _ in Q["footer"]["index"]]
    assert [v["raw"] for v in P["vectors"]] == [v["raw"] for v in Q["vectors"]]
    assert len(P["matrices"]) == len(Q["matrices"]) == info["matrices"]
    nblocks = nfloat = raw = deflated = pieces = 0
    for a, b in zip(P["matrices"], Q["matrices"]):
        assert (a["c1"], a["c2"]) == (b["c1"], b["c2"])
        for za, zb in zip(a["res"], b["res"]):
            assert [za[k] for k in ("zoom", "bin_size", "bb", "bcc")] == [zb[k] for k in ("zoom", "bin_size", "bb", "bcc")]
            assert struct.pack("<f", za["sum"]) == struct.pack("<f", zb["sum"])
            assert [x["number"] for x in za["blocks"]] == [x["number"] for x in zb["blocks"]]
            for x, y in zip(za["blocks"], zb["blocks"]):
                assert x["payload"] == y["payload"], (a["c1"], a["c2"], za["bin_size"], x["number"])
                blocks, out = _streams(x["stream"])
                assert out == x["payload"]
                nblocks += 1
                nfloat += 1 - x["head"]["useShort"]
                raw += len(x["payload"])
                deflated += x["size"]
                pieces += (len(x["payload"]) + hd.PIECE - 1) // hd.PIECE
    assert (info["blocks"], info["float_blocks"], info["raw_bytes"], info["deflated_bytes"], info["pieces"]) == (nblocks, nfloat, raw, deflated, pieces)
    for k, r in enumerate(case.resolutions):
        assert hd.cells_of(P, case.chroms, r) == cells[k] == [tuple(c) for c in case.cells[k]]
    return got, P, info


@pytest.fixture(scope="module")
def geo():
    _need_gpu()
    case = hc.geometry()
    with _loaded(case) as mx:
        yield case, mx


def test_block_geometry(geo):
    case, mx = geo
    got, P, info = _check(mx, case)
    assert [(a["c1"], a["c2"]) for a in P["matrices"]] == [(0, 0), (0, 1), (0, 3), (1, 1), (3, 3)]          # no chrB x chrC, nothing of chrNone
    assert P["header"]["genome"] == b"toy1" and not P["vectors"]
    fine = P["matrices"][0]["res"][1]
    assert fine["bin_size"] == 10 and fine["bcc"] == 4 and [b["number"] for b in fine["blocks"]] == [0, 4, 5, 8, 9, 10, 12, 13, 14, 15]
    assert info["float_blocks"] == 0 and info["blocks"] > 20


@pytest.fixture(scope="module", params=["exact", "four_more", "triangle", "noisy"])
def big(request):
    _need_gpu()
    case = dict(exact=lambda: hc.payload_of(16316), four_more=lambda: hc.payload_of(16317), triangle=hc.triangle, noisy=hc.noisy)[request.param]()
    with _loaded(case) as mx:
        yield request.param, case, mx


@pytest.mark.parametrize("level", [0, 1, 2])
def test_piece_boundaries(big, level):
    name, case, mx = big
    got, P, info = _check(mx, case, level=level)
    blk = P["matrices"][0]["res"][0]["blocks"]
    assert len(blk) == 1 and info["blocks"] == 1
    size = len(blk[0]["payload"])
    assert size == dict(exact=65280, four_more=65284, triangle=132624, noisy=16 + 4 * 17114)[name]
    assert info["pieces"] == dict(exact=1, four_more=2, triangle=3, noisy=2)[name]
    blocks, _ = _streams(blk[0]["stream"])
    stored = [b.stored_len for b in blocks if b.btype == 0 and b.stored_len]
    if level == 0:
        assert stored == [min(hd.PIECE, size - k) for k in range(0, size, hd.PIECE)]
    else:
        if name == "four_more":
            assert stored == [4], "a piece that does not shrink is one stored block inside the stream"
        if name != "noisy":                                                        # (regular payloads: coded, and smaller)
            assert blocks[0].btype == level and info["deflated_bytes"] < info["raw_bytes"]


def test_count_width():
    _need_gpu()
    case = hc.widths()
    with _loaded(case) as mx:
        got, P, info = _check(mx, case)
        blocks = {b["number"]: b for b in P["matrices"][0]["res"][0]["blocks"]}
        bcc = 160 // 10 // 4 + 1
        fl, sh = blocks[0 * bcc + 0], blocks[1 * bcc + 1]
        assert fl["head"]["useShort"] == 0 and (1, 2, 32768) in fl["records"] and len(fl["payload"]) == 16 + 4 * 2 + 6 * 2
        assert sh["head"]["useShort"] == 1 and (4, 5, 32767) in sh["records"] and len(sh["payload"]) == 16 + 4 * 2 + 4 * 2
        assert info["float_blocks"] == 1 and info["blocks"] == 2


def test_empty_object():
    _need_gpu()
    with m.Matrix(hc.geometry().table, [10, 25]) as mx:
        mx.run()
        info = mx.hic(block_bins=4)
        P = hd.parse(mx.hic_bytes())
        assert P["matrices"] == [] and P["footer"]["keys"] == [] and P["vectors"] == []
        assert mx.hic_bytes() == hd.build(hc.GEO_CHROMS, [10, 25], [[], []], None, dict(block_bins=4))
        assert info["matrices"] == info["blocks"] == info["pieces"] == 0


def test_vectors(geo):
    case, mx = geo
    st = mx.balance(0, min_nnz=1, mad_max=0, ignore_diags=0, max_iters=50)
    w = mx.weights(0)
    assert np.isnan(w).any() and np.isfinite(w).any()                              # chrNone has no contacts: masked
    try:
        got, P, info = _check(mx, case, weights=[w.tolist(), None], norm_label=b"VC")
        assert len(P["vectors"]) == len(case.chroms) and {v["type"] for v in P["vectors"]} == {b"VC"} and {v["bin_size"] for v in P["vectors"]} == {10}
        flat = np.array([x for v in P["vectors"] for x in v["values"]])
        assert np.array_equal(np.isnan(flat), np.isnan(w)) and flat[~np.isnan(w)].tobytes() == (1.0 / w[~np.isnan(w)]).tobytes()
        _, P0, _ = _check(mx, case, weights=[w.tolist(), None], norm=False)
        assert P0["vectors"] == []
    finally:
        mx.run()                                                                   # the shared object without weights again
    _, P1, _ = _check(mx, case)
    assert P1["vectors"] == []


_CHILD = """
import sys
sys.path.insert(0, %r)
import microcket_amd as m
import hic_cases as hc
case = hc.geometry()
with m.Matrix(case.table, case.resolutions) as mx:
    mx.add(case.text()); mx.run(); mx.hic(**case.opts)
    sys.stdout.buffer.write(mx.hic_bytes())
"""


def test_sameness(geo):
    case, mx = geo
    mx.hic(**case.opts)
    first = mx.hic_bytes()
    mx.hic(**case.opts)
    assert mx.hic_bytes() == first
    with m.Matrix(case.table, case.resolutions) as other:                          # another object, the text in other pieces and order
        text = case.text()
        lines = text.split(b"\n")[:-1]
        shuffled = b"\n".join(lines[:1] + lines[:0:-1]) + b"\n"
        for p in range(0, len(shuffled), 777):
            other.add(shuffled[p:p + 777])
        other.run()
        other.hic(**case.opts)
        assert other.hic_bytes() == first
    r = subprocess.run([sys.executable, "-c", _CHILD % os.path.join(util.ROOT, "tests")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, PYTHONPATH=util.ROOT), timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == first


def test_text_route_and_key_list_route_agree():
    _need_gpu()
    import test_gpu_matrix as tm
    tt = tm._table(tm.HG38)
    sam = util.synth("unc", 61, 20000)
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS) as c:
        pairs_text = c.run_bytes(sam, chunk=1 << 20)[0]
        with m.Matrix(tt, [1000000, 5000000]) as kx, m.Matrix(tt, [1000000, 5000000]) as tx:
            kx.add_keys(c, True)
            kx.run()
            tx.add(pairs_text)
            tx.run()
            ik, it = kx.hic(block_bins=16), tx.hic(block_bins=16)
            assert ik == it and ik["blocks"] > 10
            assert kx.hic_bytes() == tx.hic_bytes()
            hd.parse(kx.hic_bytes())


def test_limits_and_state(geo):
    case, mx = geo
    import ctypes as C
    from microcket_amd import capi
    o = capi.HicOpts()
    mx.L.mkt_hic_opts_default(C.byref(o))
    assert (o.block_bins, o.level, o.norm, o.genome_id, o.norm_label) == (1000, 2, 1, None, None)
    assert mx.L.mkt_matrix_hic(mx.h, None, None) == 0                              # NULL options: the defaults
    for bb in (0, 32768):
        o.block_bins = bb
        assert mx.L.mkt_matrix_hic(mx.h, C.byref(o), None) == MKT_E_ARG
        assert b"block_bins %d" % bb in mx.L.mkt_matrix_error(mx.h)
        with pytest.raises(m.MktError, match="block_bins %d" % bb):
            mx.hic(block_bins=bb)
    mx.hic(block_bins=32767)
    hd.parse(mx.hic_bytes())
    with pytest.raises(m.MktError, match="level"):
        mx.hic(level=3)
    with pytest.raises(TypeError):
        mx.hic(blocks=4)
    with m.Matrix(case.table, [10]) as fresh:
        with pytest.raises(m.MktError, match="hic before run"):
            fresh.hic()
        fresh.run()
        with pytest.raises(m.MktError, match="hic first"):
            fresh.hic_bytes()
    with m.Matrix(case.table, [10, 10]) as twice:
        twice.run()
        with pytest.raises(m.MktError, match="twice"):
            twice.hic()


def test_executable(tmp_path, geo):
    case, mx = geo
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()
    (tmp_path / "t.sizes").write_bytes(case.table)
    (tmp_path / "in.pairs").write_bytes(case.text())
    pre = str(tmp_path / "out")
    r = subprocess.run([EXE, "-g", str(tmp_path / "t.sizes"), "-r", "10,25", "-o", pre, "--hic", "--hic-block-bins", "4", "--hic-genome", "toy1", "--hic-level", "1", str(tmp_path / "in.pairs")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    info = mx.hic(level=1, **case.opts)
    assert (tmp_path / "out.hic").read_bytes() == mx.hic_bytes()
    stat = dict(ln.split("\t") for ln in (tmp_path / "out.hic.stat").read_text().splitlines())
    assert int(stat["FileBytes"]) == info["file_bytes"] and int(stat["Blocks"]) == info["blocks"] and stat["Level"] == "1" and stat["BlockBins"] == "4"
    mx.write_hic(str(tmp_path / "py.hic"), level=1, **case.opts)
    assert (tmp_path / "py.hic").read_bytes() == mx.hic_bytes()
    # with --balance the vectors are in the file; a sub-option without --hic is a usage error
    r = subprocess.run([EXE, "-g", str(tmp_path / "t.sizes"), "-r", "10", "-o", pre + "b", "--hic", "--hic-block-bins", "4", "--balance", "--min-nnz", "1", "--mad-max", "0",
                        "--ignore-diags", "0", "--hic-norm-label", "VC", str(tmp_path / "in.pairs")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    P = hd.parse((tmp_path / "outb.hic").read_bytes())
    assert len(P["vectors"]) == len(case.chroms) and P["vectors"][0]["type"] == b"VC"
    r = subprocess.run([EXE, "-g", str(tmp_path / "t.sizes"), "-r", "10", "-o", pre + "c", "--hic-level", "1", str(tmp_path / "in.pairs")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 2 and not os.path.exists(pre + "c.hic")
