"""Contact-matrix binning on the GPU (mkt_matrix_*, bin/pairs2matrix) against the definition restated in tests/matrixdef.py.
Every comparison is exact: integers and bytes.  Parity with juicer_tools / cooler is unpinned (neither is run)."""
import os
import random
import subprocess

import numpy as np
import pytest

import matrixdef as md
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
RES = [2500000, 100000, 7777, 5000, 1000, 1]

# names and lengths of mkt_synth.h (syn_chrom): anno/hg38.info and anno/mm10.info
HG38 = [("chr1", 248956422), ("chr10", 133797422), ("chr11", 135086622), ("chr12", 133275309), ("chr13", 114364328), ("chr14", 107043718),
        ("chr15", 101991189), ("chr16", 90338345), ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr2", 242193529),
        ("chr20", 64444167), ("chr21", 46709983), ("chr22", 50818468), ("chr3", 198295559), ("chr4", 190214555), ("chr5", 181538259),
        ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636), ("chr9", 138394717), ("chrM", 16569), ("chrX", 156040895),
        ("chrY", 57227415)]
MM10 = [("chr1", 195471971), ("chr10", 130694993), ("chr11", 122082543), ("chr12", 120129022), ("chr13", 120421639), ("chr14", 124902244),
        ("chr15", 104043685), ("chr16", 98207768), ("chr17", 94987271), ("chr18", 90702639), ("chr19", 61431566), ("chr2", 182113224),
        ("chr3", 160039680), ("chr4", 156508116), ("chr5", 151834684), ("chr6", 149736546), ("chr7", 145441459), ("chr8", 129401213),
        ("chr9", 124595110), ("chrM", 16299), ("chrX", 171031299), ("chrY", 91744698)]


def _table(rows) -> bytes:
    return "".join(f"{n}\t{l}\n" for n, l in rows).encode()


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _pieces(data: bytes, seed):
    """irregular chunks that split lines: sizes from 1 byte to 1 MiB"""
    rnd = random.Random(seed)
    pos = 0
    while pos < len(data):
        k = rnd.choice((1, 2, 7, 61, 4093, 65537, 300001, 1 << 20))
        yield data[pos:pos + k]
        pos += k


def _fetch(mx, nres):
    """[(cells (k, 3) uint64, text)] per resolution; the arrays and the device-made text must say the same"""
    out = []
    for k in range(nres):
        b1, b2, c = mx.cells(k)
        cells = np.stack([b1, b2, c], axis=1).astype(np.uint64) if b1.size else np.zeros((0, 3), dtype=np.uint64)
        text = mx.text(k)
        nbins, nnz, tb = mx.info(k)
        assert nnz == cells.shape[0] and tb == len(text)
        assert text == md.coo_text(cells)                                   # mkt_matrix_fetch agrees with mkt_matrix_fetch_text
        if nnz:
            key = cells[:, 0] * np.uint64(1 << 32) + cells[:, 1]
            assert (key[1:] > key[:-1]).all() and (cells[:, 0] <= cells[:, 1]).all() and int(cells[:, 1].max()) < nbins and int(cells[:, 2].min()) >= 1
        out.append((cells, text))
    return out


def _gpu_text(table, res, data, seed=None):
    """data through Matrix.add (whole, or in irregular pieces) -> (pairs, skipped, [(cells, text)])"""
    with m.Matrix(table, res, device=0) as mx:
        if seed is None:
            mx.add(data)
        else:
            for p in _pieces(data, seed):
                mx.add(p)
        pairs, skipped = mx.run()
        got = _fetch(mx, len(res))
    for cells, _ in got:
        assert int(cells[:, 2].sum()) + skipped == pairs                    # nothing passes by binning next to nothing
    return pairs, skipped, got


def _check(want, res, pairs_n, got):
    pairs, skipped, per = got
    assert pairs == pairs_n
    for k, r in enumerate(res):
        cells, sk = want[r]
        assert skipped == sk
        assert per[k][0].shape == cells.shape and (per[k][0] == cells).all(), (r, per[k][0][:5], cells[:5])
        assert per[k][1] == md.coo_text(cells)


def _cli(tmp_path, table, rlist, inputs, stdin=None):
    t = tmp_path / "genome.sizes"
    t.write_bytes(table)
    files = []
    for k, data in enumerate(inputs):
        p = tmp_path / f"in{k}.pairs"
        p.write_bytes(data)
        files.append(str(p))
    pre = tmp_path / "o"
    r = subprocess.run([EXE, "-g", str(t), "-r", rlist, "-o", str(pre), *files], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r, pre


def _oracle_inputs():
    """(name, table, .pairs text, cap on the definition's skipped share)"""
    hg, mm = _table(HG38), _table(MM10)
    return [
        ("unc/hg38/150", hg, util.oracle_run(util.synth("unc", 61, 20000), "unc", 4, 0.5, 10, False)[0], 0.0),
        ("flash/hg38", hg, util.oracle_run(util.synth("flash", 61, 20000), "flash", 4, 0.5, 10, False)[0], 0.0),
        ("unc/mm10/100/4 lanes", mm, util.oracle_run(util.synth("unc", 61, 20000, read_len=100, genome="mm10", lanes=4), "unc", 4, 0.5, 10, False)[0], 0.0),
        ("stress", hg, util.oracle_run(util.synth("stress", 61, 20000), "unc", 4, 0.5, 10, False)[0], 0.10),
    ]


# ---- 1. the hand example -------------------------------------------------------------------------------------------------
def test_hand_example_through_the_library_and_the_executable(tmp_path):
    _need_gpu()
    pairs, skipped, per = _gpu_text(md.HAND_TABLE, [100], md.HAND_PAIRS)
    assert (pairs, skipped) == (13, 5)
    assert per[0][0].tolist() == [[0, 10, 1], [1, 9, 3], [9, 9, 1], [10, 13, 1], [11, 13, 1], [12, 12, 1]]
    assert per[0][1] == b"0\t10\t1\n1\t9\t3\n9\t9\t1\n10\t13\t1\n11\t13\t1\n12\t12\t1\n"
    with m.Matrix(md.HAND_TABLE, [100, 1000]) as mx:
        assert mx.info(0)[0] == 14 and mx.info(1)[0] == 3                   # nbins are known before run
    r, pre = _cli(tmp_path, md.HAND_TABLE, "100,1000", [md.HAND_PAIRS])
    assert r.returncode == 0, r.stderr
    assert open(f"{pre}.100.coo", "rb").read() == md.HAND_COO
    assert open(f"{pre}.100.bins.bed", "rb").read() == md.HAND_BED
    assert open(f"{pre}.1000.coo", "rb").read() == b"0\t0\t4\n0\t1\t1\n1\t1\t1\n1\t2\t2\n"
    assert open(f"{pre}.1000.bins.bed", "rb").read() == b"chrB\t0\t1000\nchrA\t0\t250\nchrC\t0\t10\n"
    assert open(f"{pre}.matrix.stat", "rb").read() == b"Pairs\t13\nBinned\t8\nSkipped\t5\nnnz.100\t6\nnnz.1000\t4\n"
    # the same pairs from stdin and split over two files, the first without its final newline
    lines = md.HAND_PAIRS.splitlines(keepends=True)
    r, pre = _cli(tmp_path, md.HAND_TABLE, "100", [b"".join(lines[:6])[:-1], b"".join(lines[6:])])
    assert r.returncode == 0 and open(f"{pre}.100.coo", "rb").read() == md.HAND_COO
    r, pre = _cli(tmp_path, md.HAND_TABLE, "100", [], stdin=md.HAND_PAIRS)
    assert r.returncode == 0 and open(f"{pre}.100.coo", "rb").read() == md.HAND_COO and open(f"{pre}.matrix.stat", "rb").read() == md.HAND_STAT


# ---- 2. oracle-made pairs as text ------------------------------------------------------------------------------------------
def test_oracle_pairs_as_text_chunked_and_shuffled():
    _need_gpu()
    for name, table, pairs_text, cap in _oracle_inputs():
        want = md.definition(table, RES, pairs_text)
        n = md.n_pairs(pairs_text)
        sk = want[RES[0]][1]
        assert n >= 5000 and sk <= cap * n, (name, n, sk)                   # the definition's own skipped share, before the GPU is asked
        if cap:
            assert sk > 0, name                                             # the one input that exercises the skip rule
        whole = _gpu_text(table, RES, pairs_text)
        _check(want, RES, n, whole)
        chunked = _gpu_text(table, RES, pairs_text, seed=len(pairs_text))
        lines = pairs_text.splitlines(keepends=True)
        random.Random(5).shuffle(lines)
        shuffled = _gpu_text(table, RES, b"".join(lines), seed=7)
        for k in range(len(RES)):                                           # same bytes out, whatever the chunking and the order
            assert chunked[2][k][1] == whole[2][k][1] and shuffled[2][k][1] == whole[2][k][1], (name, RES[k])
        assert chunked[:2] == whole[:2] == shuffled[:2]


# ---- 3. the same pairs straight from a context's key list ---------------------------------------------------------------------
def _ctx_run(mode, sam_text, lanes=False):
    ext = m.EXT_KEYS | (m.EXT_LANES if lanes else 0)
    c = m.Context(mode, 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=ext)
    p, _s, st, _log = c.run_bytes(sam_text, chunk=1 << 20)
    return c, p, st


def test_pairs_from_context_keys_with_and_without_duplicates():
    _need_gpu()
    hg, mm = _table(HG38), _table(MM10)
    cases = [("unc", util.synth("unc", 61, 20000), hg, 0.0, False), ("flash", util.synth("flash", 61, 20000), hg, 0.0, False),
             ("unc", util.synth("unc", 61, 20000, read_len=100, genome="mm10", lanes=4), mm, 0.0, True), ("unc", util.synth("stress", 61, 20000), hg, 0.10, False)]
    for mode, sam_text, table, cap, lanes in cases:
        c, p, st = _ctx_run(mode, sam_text, lanes)
        try:
            want = md.definition(table, RES, p)
            n = md.n_pairs(p)
            assert n == st.pairs and n >= 5000 and want[RES[0]][1] <= cap * n
            with m.Matrix(table, RES) as mx:
                mx.add_keys(c, True)
                pairs, skipped = mx.run()
                got = _fetch(mx, len(RES))
            _check(want, RES, n, (pairs, skipped, got))
            text_route = _gpu_text(table, RES, p, seed=3)                   # ... and equal to the text route on the context's own .pairs
            for k in range(len(RES)):
                assert got[k][1] == text_route[2][k][1]
            # without the duplicates: the flags of ext_dedup leave pairs out
            total, dups, flags = c.ext_dedup(True)
            assert total == n and len(flags) == n
            want2 = md.definition(table, RES, p, flags)
            with m.Matrix(table, RES) as mx:
                mx.add_keys(c, True, flags)
                pairs2, skipped2 = mx.run()
                got2 = _fetch(mx, len(RES))
            _check(want2, RES, n - dups, (pairs2, skipped2, got2))
            with m.Matrix(table, RES) as mx:
                with pytest.raises(m.MktError, match="flags"):
                    mx.add_keys(c, True, flags[:-1])
        finally:
            c.close()
    # two contexts (one stitched, one unstitched) and a piece of text into ONE matrix = the definition over everything
    c1, p1, _ = _ctx_run("flash", util.synth("flash", 62, 9000))
    c2, p2, _ = _ctx_run("unc", util.synth("unc", 63, 9000))
    try:
        want = md.definition(hg, RES, p1 + p2 + md.HAND_PAIRS)
        with m.Matrix(hg, RES) as mx:
            mx.add_keys(c1, True)
            mx.add(md.HAND_PAIRS)
            mx.add_keys(c2, True)
            pairs, skipped = mx.run()
            got = _fetch(mx, len(RES))
        _check(want, RES, md.n_pairs(p1) + md.n_pairs(p2) + 13, (pairs, skipped, got))
    finally:
        c1.close(); c2.close()
    with m.Context("unc", 0.5, 10, False, 4, device=0) as c3, m.Matrix(hg, [5000]) as mx:   # a context without the key list
        with pytest.raises(m.MktError, match="MKT_EXT_KEYS"):
            mx.add_keys(c3, True)


# ---- 4. scale: many tiles, several digits ------------------------------------------------------------------------------------
def _generated(n, seed, table_rows):
    """n pairs inside the tabulated lengths: (ia, pa, ib, pb) and their .pairs text; two thirds cis within 2 Mb"""
    rng = np.random.default_rng(seed)
    L = np.array([l for _, l in table_rows], dtype=np.int64)
    w = L / L.sum()
    ia = rng.choice(len(L), size=n, p=w)
    ib = np.where(rng.random(n) < 0.67, ia, rng.choice(len(L), size=n, p=w))
    pa = 1 + (rng.random(n) * L[ia]).astype(np.int64)
    pa = np.minimum(pa, L[ia])
    near = np.clip(pa + rng.integers(-2_000_000, 2_000_000, size=n), 1, L[ia])
    far = np.minimum(1 + (rng.random(n) * L[ib]).astype(np.int64), L[ib])
    pb = np.where(ia == ib, near, far)
    names = [nm for nm, _ in table_rows]
    text = "".join(f"q\t{names[a]}\t{p}\t{names[b]}\t{q}\t+\t-\n" for a, p, b, q in zip(ia.tolist(), pa.tolist(), ib.tolist(), pb.tolist())).encode()
    return ia, pa, ib, pb, text


def test_two_million_pairs_against_numpy():
    _need_gpu()
    n = (1 << 21) + 12345
    ia, pa, ib, pb, text = _generated(n, 11, HG38)
    res = [5000, 2500000]
    want = md.definition_arrays([(nm.encode(), l) for nm, l in HG38], res, ia, pa, ib, pb)
    assert want[5000][1] == 0                                               # drawn inside the tabulated lengths
    with m.Matrix(_table(HG38), res) as mx:
        for k in range(0, len(text), 32 << 20):
            mx.add(text[k:k + (32 << 20)])
        pairs, skipped = mx.run()
        got = _fetch(mx, 2)
        _check(want, res, n, (pairs, skipped, got))
        assert got[0][0].shape[0] > (1 << 20) and got[1][0].shape[0] > 100000 and int(got[1][0][:, 2].max()) > 8
        # 6. again in the same process: the same bytes (nothing depends on the order atomics or workgroups ran in)
        mx.run()
        again = _fetch(mx, 2)
        assert again[0][1] == got[0][1] and again[1][1] == got[1][1]
    with m.Matrix(_table(HG38), res) as mx:
        mx.add(text)
        assert mx.run() == (n, 0)
        assert mx.text(0) == got[0][1] and mx.text(1) == got[1][1]


# ---- 5. one hot cell, empty input, header, malformed lines ---------------------------------------------------------------------
def test_hot_cell_spanning_many_workgroups():
    _need_gpu()
    hot = b"h\tchr7\t5000001\tchr7\t5004999\t+\t-\n" * 250000
    ia, pa, ib, pb, bg = _generated(60000, 12, HG38)
    bgl = bg.splitlines(keepends=True)
    data = b"".join(bgl[:30000]) + hot[:len(hot) // 2] + b"".join(bgl[30000:]) + hot[len(hot) // 2:]
    res = [5000, 1, 2500000]
    want = md.definition(_table(HG38), res, data)
    got = _gpu_text(_table(HG38), res, data, seed=9)
    _check(want, res, 310000, got)
    assert int(got[2][0][0][:, 2].max()) >= 250000 and int(got[2][1][0][:, 2].max()) == 250000


def test_empty_input_header_and_malformed_lines(tmp_path):
    _need_gpu()
    hg = _table(HG38)
    with m.Matrix(hg, [5000, 1000]) as mx:
        assert mx.run() == (0, 0)
        assert mx.info(0)[1:] == (0, 0) and mx.text(0) == b"" and mx.cells(1)[0].size == 0
    r, pre = _cli(tmp_path, hg, "5000", [b""])
    assert r.returncode == 0, r.stderr
    assert open(f"{pre}.5000.coo", "rb").read() == b"" and open(f"{pre}.matrix.stat", "rb").read() == b"Pairs\t0\nBinned\t0\nSkipped\t0\nnnz.5000\t0\n"
    assert open(f"{pre}.5000.bins.bed", "rb").read() == md.bins_bed(hg, 5000)
    # a 4DN header in front: '#' lines are not pairs
    header = b"## pairs format v1.0\n#sorted: chr1-chr2-pos1-pos2\n#shape: upper triangle\n#chromsize: chr1 248956422\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    body = util.oracle_run(util.synth("unc", 64, 3000), "unc", 4, 0.5, 10, False)[0]
    want = md.definition(hg, [5000], header + body)
    got = _gpu_text(hg, [5000], header + body, seed=2)
    _check(want, [5000], md.n_pairs(body), got)
    assert got[2][0][1] == _gpu_text(hg, [5000], body)[2][0][1]
    # all skipped: pairs are counted, nothing is binned
    assert _gpu_text(md.HAND_TABLE, [100], b"a\tchr1\t5\tchr1\t9\t+\t-\n" * 3)[:2] == (3, 3)
    # a four-column line, a non-decimal position: run fails with a message; the executable exits 21
    for bad in (b"r\tchr1\t100\tchr2\n", b"r\tchr1\t1x0\tchr2\t5\t+\t-\n", b"r\tchr1\t\tchr2\t5\t+\t-\n", b"no tabs here\n"):
        with m.Matrix(hg, [5000]) as mx:
            mx.add(body[:5000].rsplit(b"\n", 1)[0] + b"\n" + bad)
            with pytest.raises(m.MktError, match="not .pairs text"):
                mx.run()
        with pytest.raises(ValueError):
            md.definition(hg, [5000], bad)
    r, pre = _cli(tmp_path, hg, "5000", [body + b"r\tchr1\t100\tchr2\n"])
    assert r.returncode == 21 and b"not .pairs text" in r.stderr


def test_limits_are_errors_with_a_message():
    _need_gpu()
    for table, res, what in ((b"chr1\t100\nchr1\t50\n", [10], "twice"), (b"chr1\n", [10], "no length"), (b"", [10], "no chromosome"),
                             (b"chr1\t100\n", [], "resolutions"), (b"chr1\t100\n", list(range(1, 18)), "resolutions"), (b"chr1\t100\n", [0], "is 0"),
                             (b"x" * 64 + b"\t100\n", [10], "63 bytes"), (b"a\t4294967295\nb\t4294967295\n", [1], "2\\^32 bins")):
        with pytest.raises(m.MktError, match=what):
            m.Matrix(table, res)
    with m.Matrix(b"chr1\t100\n", [10]) as mx:
        with pytest.raises(m.MktError, match="before run"):
            mx._chk(mx.L.mkt_matrix_fetch(mx.h, 0, 0, 0, None, None, None), "mkt_matrix_fetch")
        with pytest.raises(m.MktError, match="resolution index"):
            mx._chk(mx.L.mkt_matrix_fetch_text(mx.h, 3, 0, None, 0), "mkt_matrix_fetch_text")
