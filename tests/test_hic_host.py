"""tests/hicdef.py on its own (no GPU): parse(build(...)) gives the inputs back, and one block is checked against bytes written by hand."""
import math
import struct
import zlib

import pytest

import hicdef as hd
import hic_cases as hc


def test_a_two_cell_block_by_hand():
    # block_bins 4: the cells (x 1, y 2, count 3) and (x 2, y 2, count 5) of block 0
    want = bytes([2, 0, 0, 0,  0, 0, 0, 0,  0, 0, 0, 0,  1, 1,  1, 0,      # nRecords, xOff, yOff, useShort, matrixType, rowCount
                  2, 0, 2, 0,                                           # row y - yOff = 2 with 2 records
                  1, 0, 3, 0,  2, 0, 5, 0])                             # x - xOff, count
    assert hd.block_payload([(2, 2, 5), (1, 2, 3)], 0, 0) == want
    # the same block one to the right and one down, with a count that needs the float form
    got = hd.block_payload([(5, 6, 32768), (6, 6, 5)], 4, 4)
    assert got == bytes([2, 0, 0, 0,  4, 0, 0, 0,  4, 0, 0, 0,  0, 1,  1, 0,  2, 0, 2, 0,  1, 0]) + struct.pack("<f", 32768.0) + bytes([2, 0]) + struct.pack("<f", 5.0)
    # ... and in a file: one chromosome of 8 bins at 10 bp, blocks of 4 bins
    f = hd.build([(b"c", 80)], [10], [[(1, 2, 3), (2, 2, 5)]], None, dict(block_bins=4))
    p = hd.parse(f)
    head = b"HIC\0" + struct.pack("<iq", 8, p["footer"]["position"]) + b"\0" + struct.pack("<i", 1) + b"software\0microcket-mi355x\0" + struct.pack("<i", 1) + b"c\0" + struct.pack("<i", 80) + \
        struct.pack("<iii", 1, 10, 0)
    assert f.startswith(head) and p["header"]["bytes"] == head
    stream = zlib.compress(want)
    rec = struct.pack("<iii", 0, 0, 1) + b"BP\0" + struct.pack("<iffffiiii", 0, 8.0, 0, 0, 0, 10, 4, 80 // 10 // 4 + 1, 1) + struct.pack("<iqi", 0, len(head) + 12 + 39 + 16, len(stream))
    foot = struct.pack("<i", 1) + b"0_0\0" + struct.pack("<qi", len(head), len(rec) + len(stream)) + struct.pack("<iii", 0, 0, 0)
    assert f == head + rec + stream + struct.pack("<i", len(foot)) + foot


@pytest.mark.parametrize("name", sorted(hc.HOST_CASES))
def test_round_trip(name):
    case = hc.HOST_CASES[name]()
    f = hd.build(case.chroms, case.resolutions, case.cells, case.weights, case.opts)
    p = hd.parse(f)
    assert p["header"]["chroms"] == case.chroms and p["header"]["genome"] == case.opts.get("genome_id", b"")
    assert p["header"]["resolutions"] == sorted(case.resolutions, reverse=True)
    for k, r in enumerate(case.resolutions):
        assert hd.cells_of(p, case.chroms, r) == sorted((int(a), int(b), int(c)) for a, b, c in case.cells[k]), r
    pairs = sorted({(hc.chrom_of(case, r, a), hc.chrom_of(case, r, b)) for k, r in enumerate(case.resolutions) for a, b, _ in case.cells[k]})
    assert [(m["c1"], m["c2"]) for m in p["matrices"]] == pairs
    assert p["footer"]["keys"] == [b"%d_%d" % pr for pr in pairs]
    want = []
    for r in sorted(case.resolutions, reverse=True):
        w = case.weights[case.resolutions.index(r)] if case.weights else None
        if w is not None and case.opts.get("norm", True):
            off, nb = hd.offsets([L for _, L in case.chroms], r)
            for c in range(len(case.chroms)):
                want.append((c, r, list(w[off[c]:off[c + 1] if c + 1 < len(off) else nb])))
    assert [(v["chr"], v["bin_size"]) for v in p["vectors"]] == [(c, r) for c, r, _ in want]
    for v, (_, _, w) in zip(p["vectors"], want):
        assert v["type"] == case.opts.get("norm_label", b"ICE") and len(v["values"]) == len(w)
        for a, b in zip(v["values"], w):
            assert (math.isnan(a) and math.isnan(b)) or a == 1.0 / b


def test_parse_refuses_what_does_not_add_up():
    case = hc.HOST_CASES["geometry"]()
    f = hd.build(case.chroms, case.resolutions, case.cells, case.weights, case.opts)
    with pytest.raises(AssertionError):
        hd.parse(f + b"\0")                                              # something behind the end
    fp = struct.unpack_from("<q", f, 8)[0]
    with pytest.raises(AssertionError):
        hd.parse(f[:fp] + struct.pack("<i", struct.unpack_from("<i", f, fp)[0] + 1) + f[fp + 4:])      # nBytes
    with pytest.raises((AssertionError, zlib.error, struct.error)):
        hd.parse(f[:fp - 1] + f[fp:])                                    # a byte missing in the last block
