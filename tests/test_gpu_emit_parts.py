"""The emit phase of the lean tile kernel (k_fast): several lanes write one .pairs line, a piece each (fast_emit_part in mkt_fast.h;
its pieces are pinned without a GPU in test_emit_parts_host.py).  Lean 48 KiB tiles forced, one block, any order; the .pairs bytes
against the oracle's as sorted lines, and no tile handed to the generic kernel, whose emitter is another one.  Texts of one to two
thousand lines; the oracle runs once per text."""
import collections

import pytest

import fast_edge_cases as ec
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

LETTERS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
_cache = {}


def _name(n, idx):
    """QNAME of n bytes, a different one for every (n, idx): idx in base 52"""
    s = b""
    for _ in range(n):
        s = LETTERS[idx % 52:idx % 52 + 1] + s
        idx //= 52
    assert idx == 0
    return s


def mixed_text():
    """case (a): two-line groups, both mates forward.  QNAMEs of 1 .. 12 bytes, chromosome names of 1, 4 and 5 bytes, positions of
    1 .. 9 digits; every sixth group is "1" against "2" with one-digit positions, with a one-byte QNAME the 14-byte line.  FLAG
    is written with ten digits: a lean line with a FLAG of more than four has that field end at byte 12 or later."""
    chrs = (b"1", b"chr1", b"chr10", b"2", b"chr2", b"chr11")
    t = ec.Text()
    for k in range(600):
        q = _name(1 + k % 12, k // 12)
        if k % 6 == 0:
            ra, rb, pa, pb = b"1", b"2", b"%d" % (1 + k % 7), b"%d" % (2 + k % 5)
        else:
            ra, rb = chrs[k % 6], chrs[(k // 6) % 6]
            pa, pb = b"%d" % (10 ** (k % 9) + k % 7), b"%d" % (10 ** ((k // 2) % 9) + 20000 * (k % 3) + k % 5)
        t.add(ec.pair(q, flag=b"0000000065", rname=ra, pos=pa, mate=dict(flag=b"0000000129", rname=rb, pos=pb)))
    return t.end()


def crowded_text():
    """case (b), flash mode: single-line fragments report a pair each.  128 lines per tile; five of eight lines report in the
    first two tiles (80 a tile: more work items than lanes at four lanes a line), three of eight in the next two (48 a tile)."""
    t = ec.Text()
    for k in range(4 * 128):
        reports = (k % 8) < (5 if k < 2 * 128 else 3)
        t.add(ec.line(b"sg%07d" % k, b"0", b"chr1" if k % 3 else b"chr12", b"%d" % (60000 + 13 * k), length=ec.PLAIN) if reports else ec.filtered(b"fg%07d" % k))
    return t.plain(6).end()


def one_pair_text():
    """case (c): the block's last tile holds filtered lines and ONE reporting group, the block's last.  (A run drops its last group,
    quirk Q1; the kernel writes it: the test reads the block's own output.)"""
    t = ec.Text().plain(64)
    assert t.n == ec.TILE
    t.add([ec.filtered(b"fa%07d" % k) for k in range(5)])
    return t.end(tail=ec.plain_group(64))


def _want(name, mode, sam):
    key = (name, mode, sam)
    if key not in _cache:
        text = {"mixed": mixed_text, "crowded": crowded_text}[name]()
        po, so, lo, st = util.oracle_run(text, mode, 4, 0.5, 10, sam)
        _cache[key] = (text, po, so, lo, st)
    return _cache[key]


def _pairs_per_tile(text, po):
    """reported pairs per lean tile: a group belongs to the tile its first line starts in (QNAMEs are unique)"""
    first = {}
    at = 0
    for ln in text.split(b"\n")[:-1]:
        first.setdefault(ln.split(b"\t", 1)[0], at)
        at += len(ln) + 1
    return collections.Counter(first[ln.split(b"\t", 1)[0]] // ec.TILE for ln in po.split(b"\n")[:-1])


def _run(text, mode, sam):
    if m.device_count() < 1:
        pytest.fail("no HIP device: the HIP path is the only path")
    with m.Context(mode, 0.5, 10, sam, 4, device=0, tiles=m.TILES_FAST) as c:
        p, s, st, log = c.run_bytes(text)
        tm = c.timing()
    return p, s, st, log, tm


def _check(name, mode, sam):
    text, po, so, lo, ost = _want(name, mode, sam)
    p, s, st, log, tm = _run(text, mode, sam)
    tag = (name, mode, sam, "tiles", tm.tiles, "deferred", tm.deferred_tiles)
    assert tm.tiles == ec.ntiles(text) and tm.deferred_tiles == 0, tag
    assert util.canon(p) == util.canon(po), tag
    assert util.canon(s) == util.canon(so), tag
    assert log == lo and (st.groups, st.pairs) == (ost.groups, ost.pairs), tag
    return text, po


def test_mixed_line_lengths():
    text, po = _check("mixed", "unc", False)
    lines = po.split(b"\n")[:-1]
    assert min(len(ln) + 1 for ln in lines) == 14 and {(len(ln) + 1) % 4 for ln in lines} == {0, 1, 2, 3}
    assert {len(ln.split(b"\t")[0]) for ln in lines} == set(range(1, 13))
    assert {len(f) for ln in lines for f in (ln.split(b"\t")[1], ln.split(b"\t")[3])} == {1, 4, 5}
    assert {len(f) for ln in lines for f in (ln.split(b"\t")[2], ln.split(b"\t")[4])} >= set(range(1, 10))


def test_more_pairs_in_a_tile_than_emitting_lanes():
    text, po = _check("crowded", "flash", False)
    per = _pairs_per_tile(text, po)
    assert any(32 < n <= 64 for n in per.values()) and any(64 < n <= ec.GCAP for n in per.values()), sorted(per.items())
    assert max(per.values()) <= ec.GCAP


def test_last_tile_reports_one_pair():
    text = one_pair_text()
    if "one_pair_block" not in _cache:                                           # (the oracle needs a group behind the block's last)
        _cache["one_pair_block"] = util.oracle_run(text + b"".join(ec.TAIL), "unc", 4, 0.5, 10, False)
    po, _, _, ost = _cache["one_pair_block"]
    per = _pairs_per_tile(text, po)
    assert ec.ntiles(text) == 2 and per[1] == 1 and per[0] == 64, sorted(per.items())
    if m.device_count() < 1:
        pytest.fail("no HIP device: the HIP path is the only path")
    with m.Context("unc", 0.5, 10, False, 4, device=0, tiles=m.TILES_FAST) as c:
        c.submit_device(c.device_text(text), len(text))
        st = c.finish(True)
        pairs, _ = c.fetch_last_block()
        tm = c.timing()
    assert tm.tiles == 2 and tm.deferred_tiles == 0, (tm.tiles, tm.deferred_tiles)
    assert util.canon(pairs) == util.canon(po)
    assert st.groups == ost.groups - 1


def test_sam_copy_behind_the_emit_phase():
    _check("mixed", "unc", True)
