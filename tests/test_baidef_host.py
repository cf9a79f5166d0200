"""tests/baidef.py (the index definition of DESIGN.md, "The index, exactly") checked on its own, no GPU: on a BAM assembled here with
struct + zlib the builder must give the index written out below by hand, and the exact comparison must reject every wrong index that
the older, one-sided checks of tests/test_gpu_bam.py (check_index_loose) let through."""
import copy
import struct
import zlib

import pytest

import baidef
import bamio
from test_gpu_bam import check_index_loose

REFS = [("A", 200000), ("B", 50000), ("C", 100000)]
# (reference, 0-based position, FLAG, CIGAR): 13 records in file order
RECS = [
    (0, 40000, 0, [(10, 0)]),          # 0  window 2 (windows 0 and 1 stay empty), bin 4683
    (0, 40100, 16, [(10, 0)]),         # 1  the same bin: one run with record 0
    (0, 49150, 0, [(10, 0)]),          # 2  [49150, 49160) straddles 3 << 14: windows 2 and 3, bin 585
    (0, 49200, 0, [(10, 0)]),          # 3  window 3, bin 4684
    (0, 49300, 4, [(10, 0)]),          # 4  placed, FLAG 4: one base, bin 4684, counted as unmapped
    (0, 50000, 0, [(40000, 0)]),       # 5  [50000, 90000): windows 3, 4, 5; bin 585 again (second chunk, not adjacent to the first)
    (0, 50100, 0, [(10, 0)]),          # 6  bin 4684 again (second chunk)
    (0, 150000, 0, [(5, 0), (5, 3), (5, 0)]),   # 7  window 9 (6, 7, 8 stay empty), bin 4690
    (2, 100, 0, [(10, 0)]),            # 8  reference B has no record
    (2, 200, 0, [(10, 0)]),            # 9
    (2, 20000, 0, [(10, 0)]),          # 10 window 1, bin 4682
    (-1, -1, 4, []),                   # 11 without coordinates
    (-1, -1, 4, []),                   # 12
]
# The index by hand.  s(i): the virtual offset where record i starts; `END` is off_end, the start of record 11 or, without the two
# trailing records, the data end.
END = 11
WANT = [
    (  # A
        {585: [(2, 3), (5, 6)], 4683: [(0, 2)], 4684: [(3, 5), (6, 7)], 4690: [(7, 8)]},
        [0, 0, 0, 2, 5, 5, 7, 7, 7, 7],
        ((0, 8), (7, 1)),
    ),
    ({}, [], None),  # B
    (  # C
        {4681: [(8, 10)], 4682: [(10, END)]},
        [8, 10],
        ((8, END), (3, 0)),
    ),
]


def bgzf(raw: bytes, level) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    d = c.compress(raw) + c.flush()
    out = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(raw), len(raw))
    assert len(out) <= 65536
    return out


def make_bam(tail: bool, on_boundary: bool):
    """-> (BAM bytes, [uncompressed start of record 0 .. n-1, data end], [compressed offset of block 0 .. the EOF block]).
    Record 6 carries 100 000 bases (150 kB), so it spans at least three blocks.  An @CO line pads the
    header: with on_boundary the data end is a multiple of 0xff00; otherwise record 3 starts exactly on the first block boundary (so
    record 2 ends on it) and the data end lies inside the last block."""
    recs = RECS if tail else RECS[:11]

    def assemble(pad):
        text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in REFS) + "@CO\t" + "x" * pad + "\n"
        raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(REFS))
        for n, ln in REFS:
            raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
        us = []
        for i, (tid, pos, flag, cig) in enumerate(recs):
            name = b"r%02d" % i
            l_seq = 100000 if i == 6 else 4
            rlen = sum(l for l, o in cig if o in (0, 2, 3, 7, 8))
            span = 1 if flag & 4 or rlen == 0 else rlen
            b = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 30, bamio.reg2bin(pos, pos + span), len(cig), flag, l_seq, -1, -1, 0)
            b += name + b"\0" + b"".join(struct.pack("<I", l << 4 | o) for l, o in cig) + b"\x12\x48" * (l_seq // 4) + b"I" * l_seq
            us.append(len(raw))
            raw += struct.pack("<i", len(b)) + b
        us.append(len(raw))
        return raw, us

    _, us = assemble(0)
    raw, us = assemble(-us[-1 if on_boundary else 3] % 0xff00)
    assert (us[-1] % 0xff00 == 0) == on_boundary and (on_boundary or us[3] == 0xff00)
    assert us[6] // 0xff00 + 2 <= (us[7] - 1) // 0xff00                       # record 6 spans at least three blocks
    data, coffs = b"", []
    for k in range(0, len(raw), 0xff00):
        coffs.append(len(data))
        data += bgzf(raw[k:k + 0xff00], (0, 6, 1)[len(coffs) % 3])
    coffs.append(len(data))
    return data + bamio.EOF_BLOCK, us, coffs


def by_hand(us, coffs, tail, eof_for_inner_end=False):
    """WANT with the record numbers replaced by virtual offsets computed here from the layout make_bam chose"""
    def s(i):
        u = us[min(i, len(us) - 1)]                   # (END without the tail: the data end)
        k, w = divmod(u, 0xff00)
        if u == us[-1] and w and eof_for_inner_end:
            return coffs[-1] << 16                    # (the mutant: the EOF block although the data end lies inside a block)
        return coffs[k] << 16 | w
    out = baidef.BaiDef()
    for bins, lin, meta in WANT:
        out.append(({b: [(s(a), s(e)) for a, e in cs] for b, cs in bins.items()}, [s(i) for i in lin],
                    None if meta is None else ((s(meta[0][0]), s(meta[0][1])), meta[1])))
    out.n_no_coor = 2 if tail else 0
    return out


@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("on_boundary", [False, True])
def test_builder_gives_the_index_written_by_hand(tail, on_boundary):
    data, us, coffs = make_bam(tail, on_boundary)
    bam = bamio.Bam(data)
    assert bam.nblocks == len(coffs) and bam.nblocks >= 3 and len(bam.records) == (13 if tail else 11)
    assert (bam.raw_len % 0xff00 == 0) == on_boundary
    got = baidef.bai_definition(bam)
    want = by_hand(us, coffs, tail)
    assert list(got) == list(want) and got.n_no_coor == want.n_no_coor
    assert baidef.bai_bytes(got) == baidef.bai_bytes(want) and baidef.explain(baidef.bai_bytes(got), want) == ""
    # the serialisation reads back through the independent reader
    bai = bamio.Bai(baidef.bai_bytes(want))
    assert bai.refs == [(b, l, None if m is None else list(m)) for b, l, m in want] and bai.n_no_coor == want.n_no_coor
    check_index_loose(bam, baidef.bai_bytes(want))
    if not tail:
        # the data end: inside the last data block it is (that block, its length), on a boundary the EOF block; bamio.Bam.voff says
        # "EOF block" for both
        last = want[2][0][4682][0][1]
        assert last == ((coffs[-1] << 16) if on_boundary else (coffs[-2] << 16 | us[-1] % 0xff00))
        assert bam.voff(bam.raw_len) == coffs[-1] << 16
    if not on_boundary:
        assert us[3] == 0xff00 and want[0][0][4684][0][0] == coffs[1] << 16      # a record that starts a block


def test_no_index_cases():
    """a reference longer than 2^29, a record ending past 2^29, a record in a window >= (LN >> 14) + 2"""
    def bam_of(refs, recs):
        text = "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
        raw = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
        for n, ln in refs:
            raw += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
        for pos, m in recs:
            b = struct.pack("<iiBBHHHiiii", 0, pos, 2, 0, bamio.reg2bin(pos, pos + m), 1, 0, 0, -1, -1, 0) + b"q\0" + struct.pack("<I", m << 4)
            raw += struct.pack("<i", len(b)) + b
        return bamio.Bam(bgzf(raw, 6) + bamio.EOF_BLOCK)
    assert baidef.bai_definition(bam_of([("a", (1 << 29) + 1)], [(5, 1)])) is None
    assert baidef.bai_definition(bam_of([("a", 1 << 29)], [((1 << 29) - 1, 2)])) is None
    assert baidef.bai_definition(bam_of([("a", 1 << 29)], [((1 << 29) - 1, 1)])) is not None
    ok = baidef.bai_definition(bam_of([("a", 1000)], [(0, 1), (999, 1), (4999, 1), (32767, 1)]))       # LN:1000: windows 0 and 1
    assert len(ok[0][1]) == 2 and sorted(ok[0][0]) == [4681, 4682]
    assert baidef.bai_definition(bam_of([("a", 1000)], [(0, 1), (32768, 1)])) is None
    assert baidef.bai_definition(bam_of([("a", 1000)], [(0, 32769)])) is None
    assert baidef.bai_bytes(None) == b"" and "none" in baidef.explain(b"BAI\1" + bytes(12), None)


def _mutants(want, bam, us, coffs, tail):
    """(name, wrong index, what explain() must name) for every wrong index the issue lists; the first four kinds (seven mutants) pass
    the one-sided checks"""
    first = {t: m[0][0] for t, (_, _, m) in enumerate(want) if m is not None}
    eof = coffs[-1] << 16
    off_end = want[2][0][4682][0][1]
    out = []

    def mut(name, needle, loose_ok, f):
        w = copy.deepcopy(want)
        w.n_no_coor = want.n_no_coor
        r = f(w)
        out.append((name, w if r is None else r, needle, loose_ok))

    def edit(t, fn):
        def f(w):
            bins, lin, meta = w[t]
            w[t] = fn(bins, lin, meta)
        return f
    # 1. linear index of zeros / of any smaller offset
    mut("lin zeros", "reference 0 window 0", True, edit(0, lambda b, l, m: (b, [0] * len(l), m)))
    mut("lin smaller", "reference 0 window 3", True, edit(0, lambda b, l, m: (b, [first[0]] * len(l), m)))
    # 2. one chunk [first record, end of data) per used bin / chunk ends that reach too far
    mut("one chunk per bin", "reference 0 bin 585: got 1 chunks, want 2", True, edit(0, lambda b, l, m: ({k: [(first[0], eof)] for k in b}, l, m)))
    mut("chunk ends too far", "reference 0 bin 585 chunk 0 of 2", True, edit(0, lambda b, l, m: ({k: [(c0, off_end) for c0, _ in cs] for k, cs in b.items()}, l, m)))
    # 3. a run split in two (records 0 and 1 of bin 4683)
    s1 = bam.records[1][0]
    mut("run split", "reference 0 bin 4683: got 2 chunks, want 1", True, edit(0, lambda b, l, m: ({**b, 4683: [(b[4683][0][0], s1), (s1, b[4683][0][1])]}, l, m)))
    # 4. pseudo-bin end too large
    mut("pseudo-bin end", "reference 0: pseudo-bin file range", True, edit(0, lambda b, l, m: (b, l, ((m[0][0], eof), m[1]))))
    mut("pseudo-bin end, last reference", "reference 2: pseudo-bin file range", True, edit(2, lambda b, l, m: (b, l, ((m[0][0], eof + (1 << 16)), m[1]))))
    # 5. n_intv longer than the last window touched
    mut("n_intv longer", "reference 2: n_intv: got 3, want 2", True, edit(2, lambda b, l, m: (b, l + [l[-1]], m)))
    # and: adjacent chunks of a bin merged, pseudo-bin dropped, n_intv / n_no_coor off by one
    mut("chunks merged", "reference 0 bin 4684: got 1 chunks, want 2", True, edit(0, lambda b, l, m: ({**b, 4684: [(b[4684][0][0], b[4684][1][1])]}, l, m)))
    mut("pseudo-bin dropped", "reference 2: bins differ: got 2, want 3", False, edit(2, lambda b, l, m: (b, l, None)))
    mut("n_intv short", "reference 0: n_intv: got 9, want 10", False, edit(0, lambda b, l, m: (b, l[:-1], m)))

    def nc(w):
        w.n_no_coor += 1
    mut("n_no_coor", "n_no_coor: got %d, want %d" % (want.n_no_coor + 1, want.n_no_coor), False, nc)
    if not tail and us[-1] % 0xff00:
        mut("last chunk ends at the EOF block", "reference 2 bin 4682 chunk 0 of 1", True, lambda w: by_hand(us, coffs, tail, eof_for_inner_end=True))
    return out


@pytest.mark.parametrize("tail,on_boundary", [(True, False), (False, False), (False, True)])
def test_exact_comparison_rejects_what_the_one_sided_checks_accept(tail, on_boundary):
    data, us, coffs = make_bam(tail, on_boundary)
    bam = bamio.Bam(data)
    want = baidef.bai_definition(bam)
    good = baidef.bai_bytes(want)
    muts = _mutants(want, bam, us, coffs, tail)
    assert len(muts) == (13 if not tail and not on_boundary else 12)
    for k, (name, w, needle, loose_ok) in enumerate(muts):
        b = baidef.bai_bytes(w)
        assert b != good, name                                           # the exact comparison rejects it ...
        msg = baidef.explain(b, want)
        assert needle in msg, (name, msg)                                # ... and says where
        if k < 7:
            assert loose_ok
        if loose_ok:
            check_index_loose(bam, b)                                    # the one-sided checks accept it: why the exact check exists
        else:
            with pytest.raises((AssertionError, TypeError)):
                check_index_loose(bam, b)
