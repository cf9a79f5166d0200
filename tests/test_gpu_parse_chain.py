"""The lean tile kernel's parser behind the heads phase that now hands it every line's start (fast_head_line, lean_eq in
microcket_amd/csrc/mkt_fast.h; tests/host/parse_chain.cpp checks the same functions on the CPU): a handful of inputs of one or
two forced 48 KiB tiles through the library and through the oracle.  .pairs, .sam and .log byte for byte in ordered mode, as
line multisets in any-order mode, where no tile may be left to the generic kernel (a case that k_tiles took proves nothing
about k_fast).

The inputs, each checked here for what it claims before it is run:
  starts    two-line groups whose names run over 5 .. 62 bytes twice, once with the second line's name at the same byte of a
            dword as the first line's and once at another; the lines' lengths walk the newline in front of a line over all 16
            bytes of its vector
  seams     neighbouring groups whose names differ in ONE byte: the first, the last, every 8k-th and (8k + 7)-th (the steps of the
            compare are 8 and 16 bytes), for names of 17, 39 and 62 bytes
  prefixes  neighbouring groups where one name is the other plus one byte, around every step length, both ways round
  straddle  a group with its first line in tile 0 and its second in tile 1, and one of three lines cut after the second
The oracle's results are computed once per input."""
import collections

import pytest

import fast_edge_cases as ec
import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

BASE = 352          # bytes of a line: a window of 56 320 bytes holds at most 160 of them (the lean kernel takes 168)
_cache = {}


def _ln(q, second, k, length):
    if second:
        return ec.line(q, b"145", b"chr2" if k % 5 == 0 else b"chr1", b"%d" % (1020000 + 1001 * k), length=length, seqlen=100, cigar=b"100M")
    return ec.line(q, b"65", b"chr1", b"%d" % (1000000 + 1000 * k), length=length, seqlen=100, cigar=b"100M")


def _name(n, k):
    """n bytes, different for every k < 26^4, no byte <= 0x20"""
    tag = bytes(97 + (k // 26 ** j) % 26 for j in range(4))
    return (tag + b"Q" * n)[:n] if n >= 4 else tag[:n]


def _starts():
    lines = []
    for g in range(116):
        ql = 5 + g % 58
        same = g < 58
        l1 = BASE + 4 * (g % 4) + (0 if same else 1 + g % 3)
        l2 = BASE + (7 * g) % 16
        q = _name(ql, g)
        a, b = _ln(q, False, g, l1), _ln(q, True, g, l2)
        assert len(a) == l1 and len(b) == l2, (g, len(a), len(b))
        lines += [a, b]
    return lines


def _seam_names(ql):
    pos = sorted({0, ql - 1} | {p for k in range(8) for p in (8 * k, 8 * k + 7) if p < ql})
    name = bytearray(b"A00123:45:HXXXXXXXX:1:1101:10000:20000:ABCDEFGHIJKLMNOPQRSTUVWXYZ"[:ql])
    out = [bytes(name)]
    for p in pos:
        name[p] = name[p] + 1 if name[p] != ord(":") else ord(";")
        out.append(bytes(name))
    return out, pos


def _seams():
    lines, k = [], 0
    for ql in (17, 39, 62):
        names, pos = _seam_names(ql)
        for a, b, p in zip(names, names[1:], pos):
            assert len(a) == len(b) == ql and [j for j in range(ql) if a[j] != b[j]] == [p]
        for q in names:
            lines += [_ln(q, False, k, BASE + 16 + (5 * k) % 16), _ln(q, True, k, BASE + 16 + (11 * k) % 16)]
            k += 1
    return lines


def _prefixes():
    lines, k = [], 0
    for n in (5, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 61):
        short = _name(n, 1000 + n)
        for q in (short, short + b"x", short):            # shorter in front of longer, and longer in front of shorter
            lines += [_ln(q, False, k, BASE + 16 + (3 * k) % 16), _ln(q, True, k, BASE + 16 + (13 * k) % 16)]
            k += 1
    return lines


def _straddle():
    t = ec.Text()
    t.plain_until(ec.TILE - BASE)
    t.add([_ln(b"straddle2", False, 1, BASE), _ln(b"straddle2", True, 1, BASE + 5)])
    assert t.n - (BASE + 5) == ec.TILE                      # the second line is tile 1's first byte
    t.plain(4)
    t.add([_ln(b"straddle3", False, 2, BASE + 3), ec.filtered(b"straddle3", BASE + 9), _ln(b"straddle3", True, 2, BASE)])
    t.plain(6)
    return t.lines


def _text(name):
    lines = {"starts": _starts, "seams": _seams, "prefixes": _prefixes, "straddle": _straddle}[name]()
    t = ec.Text()
    if name != "straddle":
        t.plain(2)
    t.add(lines)
    if name != "straddle":
        t.plain(3)
    text = t.end()
    assert 1 <= ec.ntiles(text) <= 2 and max(ec.window_lines(text)) <= ec.LCAP, (name, len(text), ec.window_lines(text))
    return text


def _line_starts(text):
    out, at = [], 0
    for ln in text.split(b"\n")[:-1]:
        out.append((at, ln))
        at += len(ln) + 1
    return out


def test_inputs_are_what_they_claim():
    """no GPU work: the properties the inputs are built for"""
    ls = _line_starts(_text("starts"))
    assert {(at - 1) % 16 for at, _ in ls[1:]} == set(range(16))                    # the newline in front of a line: every byte of a vector
    assert {len(ln) % 16 for _, ln in ls} == set(range(16))                         # ... and the previous line's length, every residue
    seen = collections.defaultdict(set)
    for (a0, l0), (a1, l1) in zip(ls, ls[1:]):
        q0, q1 = l0.split(b"\t")[0], l1.split(b"\t")[0]
        if q0 == q1 and q0[4:5] in (b"Q", b""):
            seen[len(q1)].add((a0 & 3) == (a1 & 3))
    assert all(seen[n] == {True, False} for n in range(5, 63)), sorted((n, seen[n]) for n in range(5, 63) if seen[n] != {True, False})
    ls = _line_starts(_text("straddle"))
    first = [at for at, ln in ls if ln.startswith(b"straddle2\t")]
    assert first[0] < ec.TILE == first[1]
    assert ec.ntiles(_text("straddle")) == 2 and ec.ntiles(_text("starts")) == 2


def _want(name, mode):
    if (name, mode) not in _cache:
        text = _text(name)
        po, so, lo, st = util.oracle_run(text, mode, 4, 0.5, 10, True)
        _cache[(name, mode)] = (text, po, so, lo, st.groups, st.pairs)
    return _cache[(name, mode)]


@pytest.mark.parametrize("mode", ["unc", "flash"])
@pytest.mark.parametrize("name", ["starts", "seams", "prefixes", "straddle"])
def test_outputs_and_no_tile_left_to_the_generic_kernel(name, mode):
    if m.device_count() < 1:
        pytest.fail("no HIP device: the HIP path is the only path")
    text, po, so, lo, groups, pairs = _want(name, mode)
    for ordered in (True, False):
        with m.Context(mode, 0.5, 10, True, 4, device=0, tiles=m.TILES_FAST, ordered=ordered) as c:
            p, s, st, log = c.run_bytes(text)
            tm = c.timing()
        tag = (name, mode, "ordered" if ordered else "any order", "tiles", tm.tiles, "deferred", tm.deferred_tiles)
        print(tag)
        assert log == lo, tag
        assert (st.groups, st.pairs) == (groups, pairs), tag
        if ordered:
            assert p == po and s == so, tag
        else:
            assert util.canon(p) == util.canon(po) and util.canon(s) == util.canon(so), tag
            assert tm.tiles == ec.ntiles(text) and tm.deferred_tiles == 0, tag       # tiles_left_to_generic_kernel
