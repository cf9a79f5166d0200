"""The lean tile kernel (k_fast) at its parser, window and capacity edges: every case of tests/fast_edge_cases.py on the GPU in
the forced 48 KiB geometry (MKT_TILES_FAST = the geometry of emulation config 10), one block, any order.  .log byte for byte,
.pairs and .sam as sorted lines, counters, and the number of tiles the lean kernel handed to the generic one against the
emulation's count for the same text: a case that k_tiles took proves nothing about k_fast, and a tile the two disagree about
is a finding.  What each case reaches, and which side of its limit it is on, is pinned without a GPU in test_fast_edges_host.py.
Oracle and emulation results are computed once per (case, mode, parameters)."""
import collections

import pytest

import fast_edge_cases as ec
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

PARAMS = ((4, 0.5, 10, True), (2, 0.8, 0, False))
NAMES = [c[0] for c in ec.cases()]
_cache = {}


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device: the HIP path is the only path")


def _want(name, mode, par):
    """(log, groups, pairs, sorted .pairs, sorted .sam, tiles, lean tiles) from the oracle and the emulation"""
    key = (name, mode, par)
    if key not in _cache:
        text = ec.case(name)[1]
        T, ratio, mapq, sam = par
        po, so, lo, st = util.oracle_run(text, mode, T, ratio, mapq, sam)
        es = util.emul_run(text, mode, T, ratio, mapq, sam, 10, 0)[3]
        _cache[key] = (lo, st.groups, st.pairs, util.canon(po), util.canon(so), es["tiles"], es["lean_tiles"])
    return _cache[key]


def _run(text, mode, par, tiles, block_bytes=0, ext=0):
    T, ratio, mapq, sam = par
    with m.Context(mode, ratio, mapq, sam, T, device=0, block_bytes=block_bytes, tiles=tiles, extensions=ext) as c:
        p, s, st, log = c.run_bytes(text)
        tm = c.timing()
        stat = c.ext_chrstat(True) if ext else None
    return p, s, st, log, tm, stat


def _same_outputs(got, want, tag):
    p, s, st, log = got[:4]
    lo, groups, pairs, cp, cs = want[:5]
    assert log == lo, tag
    assert (st.groups, st.pairs) == (groups, pairs), tag
    assert util.canon(p) == cp, tag
    assert util.canon(s) == cs, tag


@pytest.mark.parametrize("name", NAMES)
def test_case_in_the_lean_geometry(name):
    _need_gpu()
    _, text, modes, expect = ec.case(name)
    for mode in modes:
        for par in PARAMS:
            want = _want(name, mode, par)
            got = _run(text, mode, par, m.TILES_FAST)
            tm = got[4]
            tag = (name, mode, par, "tiles", tm.tiles, "deferred", tm.deferred_tiles, "emulation", want[5], want[5] - want[6])
            print(tag)
            _same_outputs(got, want, tag)
            assert tm.tiles == want[5], tag
            assert tm.deferred_tiles == want[5] - want[6], tag
            assert want[6] == (want[5] if expect == "all" else expect), tag      # (what test_fast_edges_host.py pins)


@pytest.mark.parametrize("name", NAMES)
def test_case_in_the_chosen_geometry(name):
    """MKT_TILES_AUTO: the tile follows the line length, so which tiles are deferred is not the case's to say; the outputs are"""
    _need_gpu()
    _, text, modes, _ = ec.case(name)
    for mode in modes:
        want = _want(name, mode, PARAMS[0])
        _same_outputs(_run(text, mode, PARAMS[0], m.TILES_AUTO), want, (name, mode))


@pytest.mark.parametrize("block", ec.BLOCK_SIZES)
@pytest.mark.parametrize("name", ec.MULTIBLOCK)
def test_several_blocks(name, block):
    """blocks of 4 KiB and of a tile and three lines: the window at a block's start and the block-end code many times over"""
    _need_gpu()
    _, text, modes, _ = ec.case(name)
    for mode in modes:
        for par in PARAMS:
            got = _run(text, mode, par, m.TILES_FAST, block_bytes=block)
            assert got[4].tile_launches > 1, (name, mode, block, got[4].tile_launches)
            _same_outputs(got, _want(name, mode, par), (name, mode, par, block))


@pytest.mark.parametrize("name", ec.BLOCK_END)
def test_reporting_line_at_the_end_of_the_block(name):
    """the block's own outputs hold its last group too (quirk Q1 drops it from the run's): the .sam copy's last vectors and bytes
    lie within 16 bytes of the end of the text"""
    _need_gpu()
    _, text, modes, _ = ec.case(name)
    for mode in modes:
        po, so, lo, ost = util.oracle_run(text + b"".join(ec.TAIL), mode, 4, 0.5, 10, True)      # (the oracle needs a group behind it)
        last = text[text.rindex(b"\n", 0, len(text) - 1) + 1:]
        assert last in so
        with m.Context(mode, 0.5, 10, True, 4, device=0, tiles=m.TILES_FAST) as c:
            c.submit_device(c.device_text(text), len(text))
            st = c.finish(True)
            pairs, sam = c.fetch_last_block()
            tm = c.timing()
        assert tm.deferred_tiles == 0 and tm.tiles == 1, (name, mode, tm.tiles, tm.deferred_tiles)
        assert util.canon(pairs) == util.canon(po), (name, mode)
        assert util.canon(sam) == util.canon(so), (name, mode)
        assert st.groups == ost.groups - 1, (name, mode)


def test_chromosome_counts_with_more_names_than_the_cache_holds():
    """ext_chrstat over 70 names of up to six bytes that crowd into few two-way sets of fast_chr_slot's cache, and three long ones:
    evictions and refills all the way, the counts are those of the oracle's .pairs lines"""
    _need_gpu()
    _, text, _, _ = ec.case("chr_cache")
    for mode in ("unc", "flash"):
        par = PARAMS[0]
        want = _want("chr_cache", mode, par)
        got = _run(text, mode, par, m.TILES_FAST, ext=m.EXT_KEYS)
        _same_outputs(got, want, ("chr_cache", mode))
        assert got[4].deferred_tiles == 0
        stat = collections.Counter()
        for ln in want[3].split(b"\n")[:-1]:
            f = ln.split(b"\t")
            stat[(f[1], f[3])] += 1
        assert len({a for a, _ in stat} | {b for _, b in stat}) >= 70
        assert got[5] == b"".join(a + b"\t" + b + b"\t" + str(n).encode() + b"\n" for (a, b), n in sorted(stat.items())), mode
