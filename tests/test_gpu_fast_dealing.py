"""The lean tile kernel's dealing of tiles: static rounds first, the block's last tiles by ticket (MKT_FAST_ROUNDS = rounds held back).

Sizes are chosen by tile count: the lean kernel runs 1024 workgroups, MKT_TILES_FAST fixes 48 KiB tiles, and a block of n bytes
holds ceil(n / 48 KiB) tiles.  One synthetic 150 bp text per mode and one oracle run per (mode, .sam, length) serve every case;
results are compared in canonical form (the line order of the any-order outputs is unspecified): .log byte for byte, counters, and the lines as a multiset (length + order-independent 64-bit checksum).
"""
import pytest

import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

TILE = 49152
WGS = 1024
TILES = 3 * WGS + 200                 # one block of three rounds and a partial one fits
_cache = {}


def _text(mode):
    if ("text", mode) not in _cache:
        if m.device_count() < 1:
            pytest.fail("no HIP device: the HIP path is the only path")
        pid = {"unc": 0, "flash": 1}[mode]
        with m.Context("unc", device=0) as c:
            ds = c.dataset(4242 + pid, pid, 1 << 19, 1 << 17, read_len=150)
            host = b"".join(c.copy_to_host(p, nb) for (p, nb, g) in ds.blocks)
            ds.close()
        want = TILES * TILE - TILE // 2
        assert len(host) > want, len(host)
        _cache["text", mode] = host[:host.rindex(b"\n", 0, want) + 1]
    return _cache["text", mode]


def _oracle(mode, sam, nbytes):
    """(log, groups, pairs, .pairs checksum, .sam checksum, .pairs bytes) of the first nbytes of the text"""
    key = ("oracle", mode, sam, nbytes)
    if key not in _cache:
        po, so, lo, st = util.oracle_run(_text(mode)[:nbytes], mode, 8, 0.5, 10, sam)
        _cache[key] = (lo, st.groups, st.pairs, (len(po),) + util.lines_checksum(po), (len(so),) + util.lines_checksum(so), po)
    return _cache[key]


def _run(monkeypatch, rounds, mode, sam, block_tiles, nbytes, ext=0):
    if rounds is None:
        monkeypatch.delenv("MKT_FAST_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("MKT_FAST_ROUNDS", str(rounds))
    text = _text(mode)[:nbytes]
    with m.Context(mode, 0.5, 10, sam, 8, device=0, block_bytes=block_tiles * TILE, tiles=m.TILES_FAST, extensions=ext) as c:
        p, s, st, log = c.run_bytes(text, chunk=16 << 20)
        tm = c.timing()
        extra = (c.ext_dedup(True), c.ext_chrstat(True)) if ext else None
    return p, s, st, log, tm, extra


def _check(monkeypatch, rounds, mode, sam, block_tiles, want_tiles, nbytes=None):
    text = _text(mode)
    nbytes = len(text) if nbytes is None else text.rindex(b"\n", 0, nbytes) + 1
    lo, groups, pairs, pck, sck, _ = _oracle(mode, sam, nbytes)
    p, s, st, log, tm, _ = _run(monkeypatch, rounds, mode, sam, block_tiles, nbytes)
    tag = (rounds, mode, sam, block_tiles, tm.tiles, tm.tile_launches, tm.deferred_tiles)
    assert tm.tiles == want_tiles, tag                                     # the tile counts the case is about
    assert tm.deferred_tiles * 20 < tm.tiles, tag                          # the lean kernel did the work
    assert log == lo, tag
    assert st.groups == groups and st.pairs == pairs, tag
    assert (len(p),) + util.lines_checksum(p) == pck, tag
    assert (len(s),) + util.lines_checksum(s) == sck, tag


@pytest.mark.parametrize("rounds", [1, "all"])
@pytest.mark.parametrize("ntiles", [WGS - 1, WGS, WGS + 1])
def test_blocks_around_one_round(monkeypatch, rounds, ntiles):
    """One block just below the grid, equal to it (nothing drawn) and one tile above it: the drawn range holds ONE tile, 1023
    workgroups draw and find nothing."""
    _check(monkeypatch, rounds, "unc", False, WGS + 400, ntiles, nbytes=ntiles * TILE - 3000)


@pytest.mark.parametrize("rounds", [1, 2, "all"])
def test_fewer_drawn_tiles_than_workgroups(monkeypatch, rounds):
    """One block of one round and 300 more tiles: most workgroups draw a tile, the others find the range empty."""
    n = (WGS + 300) * TILE - 5000
    _check(monkeypatch, rounds, "unc", False, WGS + 400, WGS + 300, nbytes=n)


@pytest.mark.parametrize("rounds", ["all", 1, None])
def test_two_blocks_of_more_than_one_round(monkeypatch, rounds):
    """Two consecutive blocks of 1024 + 90 tiles each (and a short third one): with "all", every tile but a workgroup's first is
    drawn, and the second block's ticket has to start from zero again."""
    per = WGS + 90
    text = _text("unc")
    n = text.rindex(b"\n", 0, (2 * per + 1) * TILE - TILE // 2) + 1
    lo, groups, pairs, pck, sck, _ = _oracle("unc", False, n)
    p, s, st, log, tm, _ = _run(monkeypatch, rounds, "unc", False, per, n)
    tag = (rounds, tm.tiles, tm.tile_launches, tm.deferred_tiles)
    assert tm.tile_launches == 3 and tm.tiles >= 2 * per + 1, tag           # (the host fills a block to its capacity: 1114, 1114, rest)
    assert tm.deferred_tiles * 20 < tm.tiles, tag
    assert log == lo and st.groups == groups and st.pairs == pairs, tag
    assert (len(p),) + util.lines_checksum(p) == pck, tag


@pytest.mark.parametrize("rounds", [1, 2, None, "all"])
def test_static_rounds_then_drawn_tiles(monkeypatch, rounds):
    """One block of three rounds and 200 more tiles, the shape of the benchmark's blocks in small: with one round held back a
    workgroup runs two static tiles and crosses to drawn ones inside its loop (the first ticket is drawn during its FIRST tile),
    with two held back (the default) it crosses after the first tile, with "all" it only ever draws."""
    _check(monkeypatch, rounds, "unc", False, TILES + 100, TILES, nbytes=TILES * TILE - 5000)


def test_switch_rejects_what_is_no_number(monkeypatch):
    monkeypatch.setenv("MKT_FAST_ROUNDS", "2x")
    with pytest.raises(Exception):
        m.Context("unc", device=0)


@pytest.mark.parametrize("mode,sam", [("unc", True), ("flash", False)])
def test_sam_output_and_flash_mode(monkeypatch, mode, sam):
    n = (WGS + 300) * TILE - 5000
    _check(monkeypatch, "all", mode, sam, WGS + 400, WGS + 300, nbytes=n)
    _check(monkeypatch, None, mode, sam, WGS + 400, WGS + 300, nbytes=n)


def test_key_extension_equals_static_dealing(monkeypatch):
    """Duplicate flags (input order of the key list) and chromosome-pair counts do not depend on the dealing."""
    text = _text("unc")
    n = text.rindex(b"\n", 0, (WGS + 300) * TILE - 5000) + 1
    ref = _run(monkeypatch, 0, "unc", False, WGS + 400, n, ext=m.EXT_KEYS)
    for rounds in ("all", None):
        got = _run(monkeypatch, rounds, "unc", False, WGS + 400, n, ext=m.EXT_KEYS)
        assert got[5] == ref[5], rounds
        assert got[3] == ref[3] and got[2].pairs == ref[2].pairs, rounds


def test_static_and_default_dealing_agree(monkeypatch):
    """MKT_FAST_ROUNDS=0 (every tile static, as before) and the default: the same sorted .pairs text and the same counters."""
    text = _text("unc")
    n = text.rindex(b"\n", 0, (WGS + 300) * TILE - 5000) + 1
    a = _run(monkeypatch, 0, "unc", False, WGS + 400, n)
    b = _run(monkeypatch, None, "unc", False, WGS + 400, n)
    assert util.canon(a[0]) == util.canon(b[0])
    assert a[3] == b[3]
    assert (a[2].groups, a[2].pairs) == (b[2].groups, b[2].pairs)
    assert (a[4].tiles, a[4].tile_launches) == (b[4].tiles, b[4].tile_launches)
