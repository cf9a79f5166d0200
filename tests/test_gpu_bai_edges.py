"""The BAI index of sam2bam (k_bai, k_bai_heads, bai_assemble in mkt_bam.hip) on inputs aimed at its edges: bin boundaries of every
level, the ends of the linear index, waves that mix references, bin runs that start on wave / workgroup edges, records on BGZF
block edges, and merge windows that cut inside a run, at a bin change and at a reference change.  Every case goes through
check_bam, whose index check is exact (tests/baidef.py, DESIGN.md "The index, exactly"); levels 0 and 2 because the compressed
offsets differ."""
import functools
import random

import pytest

import baidef
import bamio
from test_gpu_bam import check_bam

pytestmark = pytest.mark.gpu

LEVELS = [0, 2]
HD = "@HD\tVN:1.6\tSO:coordinate\n"


def line(name, pos1, cigar="3M", flag=0, rname="chr1", seq=None, qual=None):
    """a SAM line; SEQ defaults to the bases of a short nM CIGAR, and to * for any other"""
    if seq is None:
        short = cigar[:-1].isdigit() and cigar[-1] == "M" and int(cigar[:-1]) <= 8
        seq = "ACGTACGT"[:int(cigar[:-1])] if short else "*"
    if qual is None:
        qual = "*" if seq == "*" else "I" * len(seq)
    return f"{name}\t{flag}\t{rname}\t{pos1}\t60\t{cigar}\t*\t0\t0\t{seq}\t{qual}"


def no_coor(name):
    return f"{name}\t4\t*\t0\t0\t*\t*\t0\t0\tACG\tIII"


def sq(refs):
    return "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs).encode()


def run(refs, lines, level, hdr_extra=b"", shuffle=0):
    """refs [(name, LN)], SAM lines (shuffled first with a seed, if given) -> (bamio.Bam, bamio.Bai) after check_bam"""
    import microcket_amd as m
    if shuffle:
        lines = list(lines)
        random.Random(shuffle).shuffle(lines)
    hdr = sq(refs) + hdr_extra
    body = ("\n".join(lines) + "\n").encode() if lines else b""
    bam_b, bai_b, n = m.sam_to_bam(hdr + body, sorted=True, level=level)
    bam = check_bam(hdr, body, bam_b, bai_b, n, True, [r[0] for r in refs], [r[1] for r in refs])
    return bam, bamio.Bai(bai_b)


def bin_level(b):
    return sum(b >= first for first in (1, 9, 73, 585, 4681))


@pytest.mark.parametrize("level", LEVELS)
def test_bin_ladder(level):
    """records that end at, start at and straddle (by one base each side) the first, an inner and the last boundary of every bin
    level, on a reference of the largest length a BAI can hold"""
    LN = 1 << 29
    lines = []
    for s in (14, 17, 20, 23, 26):
        nb = LN >> s
        for k in (1, (nb // 3) | 1, nb - 1):
            B = k << s
            for i in range(40):                                    # (several of each, so that their runs have more than one record)
                lines.append(line(f"e{s}_{k}_{i}", B - 3 + 1, "3M"))          # [B - 3, B)
                lines.append(line(f"s{s}_{k}_{i}", B + 1, "3M"))              # [B, B + 3)
                lines.append(line(f"x{s}_{k}_{i}", B - 1 + 1, "2M"))          # [B - 1, B + 1)
    lines.append(line("last", LN, "1M"))                                       # the last base: [2^29 - 1, 2^29)
    lines.append(line("gap", (1 << 26) - 10 + 1, "5M20N5M", seq="ACGTACGTAC"))  # the N gap crosses 2^26: bin 0
    bam, bai = run([("chr1", LN)], lines, level, shuffle=5)
    bins = bai.refs[0][0]
    assert {bin_level(b) for b in bins} == {0, 1, 2, 3, 4, 5}
    assert 0 in bins and 4681 + (LN >> 14) - 1 in bins and len(bai.refs[0][1]) == LN >> 14


@pytest.mark.parametrize("level", LEVELS)
def test_linear_index_windows(level):
    """LN no multiple of 16384; records in windows 3, 4 and the last only, one over five windows, one on the last base, one in the
    slack window past LN; a second reference used in its window 0 only"""
    LN = 20 * 16384 + 1000
    rng = random.Random(9)
    lines = []
    for w in (3, 4):
        lines += [line(f"w{w}_{i}", w * 16384 + rng.randrange(0, 16384 - 3) + 1) for i in range(1200)]
    lines += [line(f"w20_{i}", 20 * 16384 + rng.randrange(0, 1000 - 3) + 1) for i in range(600)]
    lines.append(line("five", 3 * 16384 + 100 + 1, "70000M"))                 # [49252, 119252): windows 3 .. 7
    lines.append(line("lastbase", LN, "1M"))
    lines.append(line("slack", 21 * 16384 + 5 + 1, "1M"))                     # past LN, inside the index's last window
    lines += [line(f"o{i}", rng.randrange(0, 16384 - 3) + 1, rname="chr2") for i in range(300)]
    bam, bai = run([("chr1", LN), ("chr2", 50000)], lines, level, shuffle=3)
    lin = bai.refs[0][1]
    assert len(lin) == 22 and len(bai.refs[1][1]) == 1
    assert lin[0] == lin[1] == lin[2] == lin[3] == bam.records[0][0]         # empty leading windows take the next one's offset
    assert lin[8:20] == [lin[20]] * 12 and lin[7] < lin[20] < lin[21]
    assert lin[4] == lin[5] == lin[6] == lin[7]                               # (the 70000M record is the first one of each)


def MANY_COUNT(t):
    return 0 if t < 3 or 150 <= t < 153 or t >= 297 else t % 4


@functools.lru_cache(maxsize=None)
def many_references():
    """300 references; 0 to 3 records on each, none on the first, middle and last three; one record in eight placed with FLAG 4;
    200 records without coordinates.  In file order every wave of 64 records holds about 40 references."""
    refs = [(f"c{t:03d}", 100000) for t in range(300)]
    rng = random.Random(17)
    lines, i = [], 0
    for t in range(300):
        for _ in range(MANY_COUNT(t)):
            pos1 = rng.randrange(1, 99000)
            lines.append(line(f"u{i}", pos1, "*", flag=4, rname=refs[t][0], seq="ACG") if i % 8 == 0 else line(f"p{i}", pos1, rname=refs[t][0]))
            i += 1
    lines += [no_coor(f"n{k}") for k in range(200)]
    return refs, lines


@pytest.mark.parametrize("level", LEVELS)
def test_many_references_in_a_wave(level):
    refs, lines = many_references()
    bam, bai = run(refs, lines, level, shuffle=11)
    assert bai.n_no_coor == 200
    assert [t for t in range(300) if bai.refs[t][2] is not None] == [t for t in range(300) if MANY_COUNT(t)]
    assert [sum(m[1]) if m else 0 for _, _, m in bai.refs] == [MANY_COUNT(t) for t in range(300)]
    assert sum(m[1][1] for _, _, m in bai.refs if m) == sum(1 for ln in lines if ln[0] == "u")
    tids = [r["tid"] for _, _, r in bam.records[:64]]
    assert len(set(tids)) > 20


@pytest.mark.parametrize("level", LEVELS)
def test_runs_and_launch_edges(level):
    """runs of one bin of 255, 256, 1, 63, 64, 65, 257 and 5000 records, separated by single records of another bin (a read
    straddling a 16 KiB boundary lands one level up): runs start at records 255 (last lane of the first workgroup), 256 and 512
    (first lane of a workgroup).  On a second reference two bins alternate for 600 records: 300 chunks each."""
    lens = [255, 256, 1, 63, 64, 65, 257, 5000]
    lines = []
    for j, n in enumerate(lens):
        base = (j + 1) * 16384 + 100
        lines += [line(f"r{j}_{i}", base + i + 1) for i in range(n)]
        if j + 1 < len(lens):
            lines.append(line(f"sep{j}", (j + 2) * 16384 - 1 + 1))             # [B - 1, B + 2)
    for i in range(600):
        lines.append(line(f"a{i}", 10 + 10 * i + 1, "20000M" if i % 2 else "3M", rname="alt"))
    bam, bai = run([("chr1", 1000000), ("alt", 100000)], lines, level)
    heads = [i for i, (_, _, r) in enumerate(bam.records) if i == 0 or (r["tid"], r["bin"]) != (bam.records[i - 1][2]["tid"], bam.records[i - 1][2]["bin"])]
    assert heads[:6] == [0, 255, 256, 512, 513, 514] and len(heads) == 15 + 600
    bins = bai.refs[0][0]
    assert all(len(bins[4682 + j]) == 1 for j in range(8)) and sum(len(c) for c in bins.values()) == 15
    assert len(bai.refs[1][0][4681]) == 300 and len(bai.refs[1][0][585]) == 300


REC = 52                # bytes of line("r%05d" % i, pos): 4 + 32 fixed, 7 name, 4 CIGAR, 2 SEQ, 3 QUAL


def padded(refs, nbytes_before_target):
    """an @CO header line that puts the uncompressed offset (header + nbytes_before_target) on a BGZF block boundary"""
    fixed = 12 + len(HD) + len(sq(refs)) + sum(9 + len(n) for n, _ in refs) + 5
    return b"@CO\t" + b"x" * (-(fixed + nbytes_before_target) % 0xff00) + b"\n"


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("case", ["record", "first_without_coordinates", "data_end", "long_record"])
def test_block_edges(case, level):
    refs = [("chr1", 1000000)]
    lines = [line("r%05d" % i, 1 + i * 300) for i in range(3000)]
    if case == "record":                  # record 1500 starts a block, so record 1499 ends on the boundary in mid-file
        lines += [no_coor("n%05d" % i) for i in range(10)]
        bam, bai = run(refs, lines, level, padded(refs, 1500 * REC))
        assert bam.records[1500][0] & 0xFFFF == 0 and bam.records[1500][0] >> 16 > 0 and bam.records[1500][2]["qname"] == "r01500"
    elif case == "first_without_coordinates":
        lines += [no_coor("n%05d" % i) for i in range(10)]
        bam, bai = run(refs, lines, level, padded(refs, 3000 * REC))
        assert bam.records[3000][0] & 0xFFFF == 0 and bam.records[3000][2]["tid"] < 0
        assert max(c1 for cs in bai.refs[0][0].values() for _, c1 in cs) == bam.records[3000][0] == bai.refs[0][2][0][1]
    elif case == "data_end":              # the last record ends the last full block: off_end is the EOF marker block
        bam, bai = run(refs, lines, level, padded(refs, 3000 * REC))
        assert bam.raw_len % 0xff00 == 0
        assert max(c1 for cs in bai.refs[0][0].values() for _, c1 in cs) == (bam.compressed - 28) << 16 == bai.refs[0][2][0][1]
    else:                                 # 150 kB in one record: it spans three blocks and ends on a block boundary
        seq = "ACGT" * 25000
        big = line("big", 200001, "100000M", seq=seq, qual="F" * 100000)
        big_bytes = 4 + 32 + 4 + 4 + 50000 + 100000
        k = 200000 // 300 + 1             # records before it in file order (positions 0, 300, .. 199800)
        lines += [big] + [no_coor("n%05d" % i) for i in range(3)]
        bam, bai = run(refs, lines, level, padded(refs, k * REC + big_bytes), shuffle=2)
        v0, v1, r = bam.records[k]
        assert r["qname"] == "big" and v1 & 0xFFFF == 0 and bam.records[k + 1][0] == v1
        assert bai.refs[0][0][73] == [(v0, v1)] and r["bin"] == 73
        data, _ = baidef.block_table(bam)
        coffs = [c for c, _ in data]
        assert coffs.index(v1 >> 16) - coffs.index(v0 >> 16) == 3                # it starts inside a block and fills the next two


@pytest.mark.parametrize("level", LEVELS)
def test_degenerate(level):
    refs = [("chr1", 1000000), ("chr2", 5000)]
    n = 1000
    bam, bai = run(refs, [no_coor("n%05d" % i) for i in range(n)], level)     # nothing placed
    assert bai.refs == [({}, [], None)] * 2 and bai.n_no_coor == n
    bam, bai = run(refs, [], level)                                            # header only
    assert bai.refs == [({}, [], None)] * 2 and bai.n_no_coor == 0
    bam, bai = run(refs, [line("one", 4000, rname="chr2")], level)             # one record
    v0, v1, _ = bam.records[0]
    end = baidef.voff_fn(bam)[0](bam.raw_len)
    assert bai.refs == [({}, [], None), ({4681: [(v0, end)]}, [v0], [(v0, end), (1, 0)])]
    assert end & 0xFFFF == bam.raw_len and end >> 16 == v0 >> 16 == 0              # inside the only data block, not the EOF block


def _spread(lines):
    """the lines in an order that spreads every sorted run of the input over the whole file"""
    lines = list(lines)
    random.Random(1).shuffle(lines)
    return lines


@functools.lru_cache(maxsize=None)
def merge_input(kind):
    n = 22000                                                                   # > 1 MiB of records of 52 (some: 47) bytes
    if kind == "one_bin":                 # every window cut falls inside a run
        return [("chr1", 1000000)], _spread([line("r%05d" % i, 16384 + 5 + i % 16000) for i in range(n)])
    if kind == "alternating_bins":        # (position, strand) order: at every position a 3M read, then a reverse read over two windows
        lines = []
        for i in range(n // 2):
            lines += [line("f%05d" % i, 5 + i), line("b%05d" % i, 5 + i, "20000M", flag=16)]
        return [("chr1", 1000000)], _spread(lines)
    if kind == "cycling_references":      # record i on reference i % 300
        refs = [(f"c{t:03d}", 100000) for t in range(300)]
        return refs, [line("r%05d" % i, 1 + (i * 37) % 90000, rname=refs[i % 300][0]) for i in range(n)]
    if kind == "one_record_per_reference":
        refs = [(f"c{t:05d}", 100000) for t in range(n)]
        return refs, _spread([line("r%05d" % t, 1 + (t * 37) % 90000, rname=refs[t][0]) for t in range(n)])
    refs, lines = many_references()
    return refs, _spread(lines)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("kind", ["one_bin", "alternating_bins", "cycling_references", "one_record_per_reference", "many_references"])
def test_across_merge_windows(kind, level, tmp_path):
    """The out-of-core path reduces the index once per merge window and hands the last record over (`prev`).  With run_bytes =
    len(body) // 40 the merge works in its smallest windows (64 KiB of records over all runs), about twenty rounds for these inputs,
    and the runs interleave over the whole file.  The number of windows and where they cut is not exposed: that every cut falls
    inside a run (one_bin), at a bin change (alternating_bins) or at a reference change (one_record_per_reference) follows from the
    inputs' construction, it is not observed.  A sorted file keeps a reference's records together, so with 300 references
    (cycling_references: record i on reference i % 300 in the input) only some cuts can fall at a reference change; the input with
    as many references as records makes every cut one.  many_references is the small input of test_many_references_in_a_wave with
    its 200 trailing records without coordinates (a dozen records per run)."""
    import microcket_amd as m
    refs, lines = merge_input(kind)
    hdr = sq(refs)
    body = ("\n".join(lines) + "\n").encode()
    assert kind == "many_references" or len(lines) == 22000
    ref = m.sam_to_bam(hdr + body, sorted=True, level=level)
    st = {}
    got = m.sam_to_bam(hdr + body, sorted=True, level=level, run_bytes=len(body) // 40, tmp=tmp_path / "w", stats=st, piece=1 << 16)
    assert st["runs"] >= 20
    assert got[2] == ref[2] == len(lines)
    assert got[0] == ref[0]
    assert got[1] == ref[1], baidef.explain(got[1], baidef.bai_definition(bamio.Bam(ref[0])))
    if kind == "many_references":
        check_bam(hdr, body, ref[0], ref[1], ref[2], True, [r[0] for r in refs], [r[1] for r in refs])
    else:                                 # (the exact index only: the region queries of check_bam take minutes on 20 000 chunks)
        bam = bamio.Bam(ref[0])
        want = baidef.bai_definition(bam)
        assert baidef.bai_bytes(want) == ref[1], baidef.explain(ref[1], want)
        assert len(bam.records) == len(lines) and [r[0] for r in bam.refs] == [r[0] for r in refs]
        us = baidef._uoffs(bam)
        assert us[-1] - us[0] >= 1 << 20                                         # record bytes: what the merge windows count
