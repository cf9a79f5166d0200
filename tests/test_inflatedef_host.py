"""tests/inflatedef.py (the plain inflate that checks the GPU deflate's blocks) against zlib, on the byte strings of the GPU
deflate edge tests: stored, fixed-code and dynamic-code streams from zlib's own deflate, with and without matches."""
import zlib

import pytest

import deflate_inputs as di
import inflatedef

STREAMS = [("stored", 0, zlib.Z_DEFAULT_STRATEGY, {0}), ("fixed", 9, zlib.Z_FIXED, {0, 1}), ("huffman-only", 9, zlib.Z_HUFFMAN_ONLY, {0, 1, 2}),
           ("rle", 9, zlib.Z_RLE, {0, 1, 2}), ("default-1", 1, zlib.Z_DEFAULT_STRATEGY, {0, 1, 2}), ("default-9", 9, zlib.Z_DEFAULT_STRATEGY, {0, 1, 2})]


def deflate(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("kind,level,strategy,btypes", STREAMS, ids=[s[0] for s in STREAMS])
def test_inflatedef_equals_zlib(kind, level, strategy, btypes):
    seen = set()
    for name, data in di.host_strings():
        comp = deflate(data, level, strategy)
        assert zlib.decompress(comp, wbits=-15) == data
        blocks, out = inflatedef.inflate(comp)
        assert out == data, name
        assert inflatedef.replay([t for b in blocks for t in b.tokens]) == data, name      # the token walk reproduces the input
        assert blocks[-1].bfinal == 1 and all(b.bfinal == 0 for b in blocks[:-1])
        assert sum(b.nbits for b in blocks) <= 8 * len(comp) < sum(b.nbits for b in blocks) + 8
        for b in blocks:
            assert b.btype in btypes, (name, b.btype)
            seen.add(b.btype)
            if b.btype == 2:
                assert len(b.ll_lengths) >= 257 and 1 <= len(b.d_lengths) <= 30 and len(b.cl_lengths) == 19 and 4 <= b.n_cl_sent <= 19
                ll, d = inflatedef.histograms(b)
                assert all((c > 0) <= (s < len(b.ll_lengths) and b.ll_lengths[s] > 0) for s, c in enumerate(ll)), name      # every symbol used has a code
                assert all((c > 0) <= (s < len(b.d_lengths) and b.d_lengths[s] > 0) for s, c in enumerate(d)), name
            if kind in ("huffman-only", "stored"):
                assert not any(isinstance(t, tuple) for t in b.tokens)
            if kind == "rle":
                assert all(t[1] == 1 for t in b.tokens if isinstance(t, tuple))
    assert {"stored": 0, "fixed": 1}.get(kind, 2) in seen                     # (zlib stores what its fixed code would expand)


def _bits_to_bytes(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        out[i >> 3] |= b << (i & 7)
    return bytes(out)


def _num(v, n):
    return [(v >> i) & 1 for i in range(n)]


def _dynamic_header(cl_lens_in_order, hlit=257, hdist=1):
    return [1, 0, 1] + _num(hlit - 257, 5) + _num(hdist - 1, 5) + _num(len(cl_lens_in_order) - 4, 4) + [b for l in cl_lens_in_order for b in _num(l, 3)]


def test_inflatedef_names_what_is_wrong():
    good = deflate(b"abcabcabcabc" * 20, 9, zlib.Z_DEFAULT_STRATEGY)
    inflatedef.inflate(good)
    with pytest.raises(inflatedef.InflateError, match="trailing"):
        inflatedef.inflate(good + b"\x00")
    with pytest.raises(inflatedef.InflateError, match="ends inside"):
        inflatedef.inflate(good[:-2])
    # fixed block, "a" then a match of length 3 at distance 2: before the start
    a = format(0x30 + 0x61, "08b")
    m = format(257 - 256, "07b") + format(1, "05b")
    eob = "0000000"
    bits = [1, 1, 0] + [int(c) for c in a + m + eob]
    with pytest.raises(inflatedef.InflateError, match="before the start"):
        inflatedef.inflate(_bits_to_bytes(bits))
    bits = [1, 1, 0] + [int(c) for c in a + format(1, "07b") + format(0, "05b") + eob]      # the same at distance 1: fine
    assert inflatedef.inflate(_bits_to_bytes(bits))[1] == b"aaaa"
    bits = [1, 1, 0] + [int(c) for c in a + eob] + [0, 1]                                     # a set bit in the padding
    with pytest.raises(inflatedef.InflateError, match="not padding"):
        inflatedef.inflate(_bits_to_bytes(bits))
    with pytest.raises(inflatedef.InflateError, match="NLEN"):
        inflatedef.inflate(bytes([1, 3, 0, 0xFC, 0xFE, 1, 2, 3]))
    assert inflatedef.inflate(bytes([1, 3, 0, 0xFC, 0xFF, 1, 2, 3]))[1] == b"\x01\x02\x03"
    # code-length code (sent in the order 16 17 18 0 ...): three codes of one bit are over-subscribed; one code of one bit is incomplete
    with pytest.raises(inflatedef.InflateError, match="code-length code: over-subscribed"):
        inflatedef.inflate(_bits_to_bytes(_dynamic_header([1, 1, 1, 0]) + [0] * 64))
    with pytest.raises(inflatedef.InflateError, match="code-length code: incomplete"):
        inflatedef.inflate(_bits_to_bytes(_dynamic_header([1, 0, 0, 0]) + [0] * 64))
    # lengths 1 (code 0) and 2 ... for symbols 18 and 0/8: literal/length code of a single one-bit code for symbol 256 is incomplete
    # code-length code: symbol 18 -> 1 bit "0", symbol 0 -> 2 bits "10", symbol 1 (last in the order but one) -> 2 bits "11"
    order = inflatedef.CODELEN_ORDER
    cl = [0] * 19
    cl[18], cl[0], cl[1] = 1, 2, 2
    sent = [cl[s] for s in order]
    while sent[-1] == 0:
        sent.pop()
    z138 = [0] + _num(127, 7)                                   # 18: 138 zeros
    z118 = [0] + _num(118 - 11, 7)
    one, zero = [1, 1], [1, 0]
    body = z138 + z118 + one + zero                              # 256 zeros, length 1 for 256, one distance length 0
    with pytest.raises(inflatedef.InflateError, match="literal/length code: incomplete"):
        inflatedef.inflate(_bits_to_bytes(_dynamic_header(sent) + body + [0] * 32))
    body = z138 + z118[:1] + _num(116 - 11, 7) + one + one + one + zero      # 254 zeros, 1 1 1: over-subscribed
    with pytest.raises(inflatedef.InflateError, match="literal/length code: over-subscribed"):
        inflatedef.inflate(_bits_to_bytes(_dynamic_header(sent) + body + [0] * 32))
    # literals 0 and 1 and end of block... a complete two-code set with the single one-bit distance code the RFC allows
    body = z138 + z118[:1] + _num(117 - 11, 7) + one + one + one      # 255 zeros, 255 -> 1, 256 -> 1; distance 0 -> 1
    blocks, out = inflatedef.inflate(_bits_to_bytes(_dynamic_header(sent) + body + [0, 0, 1]))      # 255 255, end of block
    assert out == b"\xff\xff" and blocks[0].d_lengths == [1] and blocks[0].btype == 2
