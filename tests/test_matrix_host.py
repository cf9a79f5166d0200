"""Contact-matrix binning (mkt_matrix_*, bin/pairs2matrix): what can be checked without a GPU.
The definition restated in tests/matrixdef.py against a hand-computed literal, and the executable's argument / input handling."""
import os
import subprocess

import numpy as np

import matrixdef as md
import microcket_amd as m
import util

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")


def _built():
    from microcket_amd import build
    build.build_lib()
    build.build_pairs2matrix()
    return EXE


def test_definition_against_hand_computed_literal():
    # table chrB 1000 / chrA 250 / chrC 10 (not in bytewise order), r = 100: 10 + 3 + 1 bins
    table = md.parse_table(md.HAND_TABLE)
    assert table == [(b"chrB", 1000), (b"chrA", 250), (b"chrC", 10)]
    off, n, nbins = md.bin_layout(table, 100)
    assert (off, n, nbins) == ([0, 10, 13], [10, 3, 1], 14)
    got = md.definition(md.HAND_TABLE, [100], md.HAND_PAIRS)
    cells, skipped = got[100]
    # 13 pairs; skipped: pos = L + 1 (r3), pos = 0 (r4), unknown name (r5), pos > L of chrC (r12), pos > L of chrA (r13)
    assert md.n_pairs(md.HAND_PAIRS) == 13 and skipped == 5
    assert cells.tolist() == [[0, 10, 1],      # r1: chrA:1 (bin 10) - chrB:1 (bin 0), swapped on bin ids
                              [1, 9, 3],       # r7, r8, r9
                              [9, 9, 1],       # r2: pos = L = 1000 -> the last bin of chrB
                              [10, 13, 1],     # r10: chrA:100 (bin 10) - chrC:10 (bin 13)
                              [11, 13, 1],     # r11: chrA:101 (bin 11) - chrC:1
                              [12, 12, 1]]     # r6: chrA:250 and chrA:201, both in the partial last bin
    assert int(cells[:, 2].sum()) + skipped == 13
    assert md.HAND_CELLS == [tuple(c) for c in cells.tolist()] and (md.HAND_PAIRS_N, md.HAND_SKIPPED) == (13, 5)
    assert md.coo_text(cells) == b"0\t10\t1\n1\t9\t3\n9\t9\t1\n10\t13\t1\n11\t13\t1\n12\t12\t1\n" == md.HAND_COO
    assert (md.cells_of_text(md.HAND_COO) == cells).all()
    assert md.bins_bed(md.HAND_TABLE, 100).split(b"\n")[9:15] == [b"chrB\t900\t1000", b"chrA\t0\t100", b"chrA\t100\t200", b"chrA\t200\t250", b"chrC\t0\t10", b""]
    assert md.bins_bed(md.HAND_TABLE, 100) == md.HAND_BED
    assert md.stat_text(13, 5, [(100, 6)]) == b"Pairs\t13\nBinned\t8\nSkipped\t5\nnnz.100\t6\n" == md.HAND_STAT
    # other resolutions of the same pairs: one bin per chromosome, and one bin per base
    big = md.definition(md.HAND_TABLE, [1000, 1], md.HAND_PAIRS)
    assert big[1000][0].tolist() == [[0, 0, 4], [0, 1, 1], [1, 1, 1], [1, 2, 2]] and big[1000][1] == 5
    assert big[1][0].shape[0] == 8 and big[1][0][0].tolist() == [0, 1000, 1]            # chrB:1 is bin 0, chrA:1 is bin 1000
    # input order does not matter; flags leave lines out
    lines = md.HAND_PAIRS.splitlines(keepends=True)
    assert (md.definition(md.HAND_TABLE, [100], b"".join(reversed(lines)))[100][0] == cells).all()
    flags = [0] * 13
    flags[7] = flags[2] = 1                                                             # r8 (binned) and r3 (skipped) left out
    c2, s2 = md.definition(md.HAND_TABLE, [100], md.HAND_PAIRS, flags)[100]
    assert s2 == 4 and c2.tolist()[1] == [1, 9, 2] and md.n_pairs(md.HAND_PAIRS, flags) == 11
    assert isinstance(cells, np.ndarray) and cells.dtype == np.uint64


def test_pairs2matrix_without_gpu(tmp_path):
    exe = _built()
    table = tmp_path / "g.sizes"
    table.write_bytes(md.HAND_TABLE)
    pairs = tmp_path / "in.pairs"
    pairs.write_bytes(md.HAND_PAIRS)
    out = tmp_path / "out" / "o"
    os.makedirs(out.parent)
    run = lambda *a: subprocess.run([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, stdin=subprocess.DEVNULL)
    r = run()
    assert r.returncode == 2 and b"Usage" in r.stderr
    r = run("-g", str(table), "-r", "100")                                              # no -o
    assert r.returncode == 2
    r = run("-g", str(table), "-r", "100", "-o", str(out), str(tmp_path / "missing.pairs"))
    assert r.returncode == 10
    r = run("-g", str(tmp_path / "missing.sizes"), "-r", "100", "-o", str(out), str(pairs))
    assert r.returncode == 10
    bad = tmp_path / "bad.sizes"
    bad.write_bytes(b"chrB\t1000\nchrA\nchrC\t10\n")                                   # a line without a length
    r = run("-g", str(bad), "-r", "100", "-o", str(out), str(pairs))
    assert r.returncode == 12 and b"line 2" in r.stderr
    for rl in ("0", "5000,abc", "5000,,100", "", "100,100", ",".join(str(k + 1) for k in range(17))):
        r = run("-g", str(table), "-r", rl, "-o", str(out), str(pairs))
        assert r.returncode == 12, rl
    if m.device_count() == 0:
        r = run("-g", str(table), "-r", "100,10", "-o", str(out), str(pairs))
        assert r.returncode == 20 and r.stdout == b""                                   # no GPU: loud failure ...
        assert os.listdir(out.parent) == []                                             # ... and no output files left behind
        import pytest
        with pytest.raises(m.MktError, match="(?i)no usable HIP device"):
            m.Matrix(md.HAND_TABLE, [100])
