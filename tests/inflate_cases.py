"""TEST INFRASTRUCTURE: directed BGZF files for the GPU inflate (mkt_bgzf_* of include/mkt.h), in families.

Each case is {"name", "family", "gz", "text" | None, "refused": None | reason}; `reason` is a key of csrc/mkt_inflate.h
(inf_reason_key).  A small bit writer turns (code lengths, tokens) into a deflate stream, so that codes and tokens zlib would never
choose can still be sent.  tests/test_inflate_cases_host.py proves without a GPU that every accepted case inflates to `text` by zlib
and by inflatedef and that every refused case is refused by inflatedef or px2def.bgzf_blocks for the matching reason.

BATCH is the kernel's token batch (kInfBatch of csrc/mkt_inflate.h): one token per lane of a wavefront."""
import gzip
import struct
import zlib

import inflatedef as D
import px2def

BATCH = 64
HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


# ---- framing -------------------------------------------------------------------------------------------------------------------------
def member(raw, text, crc=None, isize=None):
    """one BGZF member around the deflate stream `raw`"""
    assert len(raw) + 26 <= 0x10000
    return HEAD + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


def zraw(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(text) + co.flush()


# ---- the bit writer ------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.v = self.n = 0

    def put(self, value, nbits):
        """nbits of value, the least significant first (header fields, extra bits)"""
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def code(self, c):
        """a Huffman code (value, length): packed from its most significant bit"""
        value, nbits = c
        for k in range(nbits - 1, -1, -1):
            self.put(value >> k & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def codes(lengths):
    """{symbol: (code, length)} of the canonical code of 3.2.2 (no check of the Kraft sum: bad codes are sent on purpose)"""
    maxl = max(list(lengths) + [1])
    count = [0] * (maxl + 2)
    for l in lengths:
        if l:
            count[l] += 1
    nxt, c = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def complete(symbols, n):
    """lengths [n] of a complete code over `symbols` (one symbol: length 1)"""
    symbols = sorted(symbols)
    lens = [0] * n
    if len(symbols) == 1:
        lens[symbols[0]] = 1
        return lens
    k = (len(symbols) - 1).bit_length()
    short = (1 << k) - len(symbols)
    for i, s in enumerate(symbols):
        lens[s] = k - 1 if i < short else k
    return lens


def skewed(symbols, n):
    """lengths 1, 2, ..., 14, 15, 15 over 16 symbols: codes of 15 bits (as deflate_inputs.fibonacci_block's histograms give)"""
    assert len(symbols) == 16
    lens = [0] * n
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, 15)
    return lens


def len_sym(length):
    i = max(k for k, b in enumerate(D.LENGTH_BASE) if b <= length)
    if length == 258:
        i = 28
    return 257 + i, length - D.LENGTH_BASE[i], D.LENGTH_EXTRA[i]


def dist_sym(dist):
    i = max(k for k, b in enumerate(D.DIST_BASE) if b <= dist)
    return i, dist - D.DIST_BASE[i], D.DIST_EXTRA[i]


def put_tokens(w, ll, dc, tokens):
    """tokens: int literal | (length, distance) | ("L", ll symbol) | ("D", distance symbol, extra value) raw symbols; then end of block"""
    for t in tokens:
        if isinstance(t, int):
            w.code(ll[t])
        elif t[0] == "L":
            w.code(ll[t[1]])
        elif t[0] == "D":
            w.code(dc[t[1]])
            w.put(t[2], D.DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        else:
            s, x, nx = len_sym(t[0])
            w.code(ll[s])
            w.put(x, nx)
            s, x, nx = dist_sym(t[1])
            w.code(dc[s])
            w.put(x, nx)


CL_PLAIN = [4] * 16 + [0, 0, 0]                                  # lengths 0 .. 15 spelled out, no repeats: complete
CL_REPEATS = [5] * 16 + [3, 2, 3]                                # + 16 (3 bits), 17 (2 bits), 18 (3 bits): complete


def dynamic(w, ll_lens, d_lens, tokens, bfinal=1, cl_lens=CL_PLAIN, spell=None, hclen=19, eob=True, hlit=None, hdist=None):
    """a dynamic block.  spell: [(code-length symbol, extra value)] for the lengths (default: one symbol per length)"""
    hlit = len(ll_lens) if hlit is None else hlit
    hdist = len(d_lens) if hdist is None else hdist
    w.put(bfinal, 1); w.put(2, 2); w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[D.CODELEN_ORDER[k]], 3)
    cc = codes(cl_lens)
    if spell is None:
        spell = [(l, 0) for l in list(ll_lens) + list(d_lens)]
    for s, x in spell:
        w.code(cc[s])
        w.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    ll, dc = codes(ll_lens), codes(d_lens)
    put_tokens(w, ll, dc, tokens)
    if eob:
        w.code(ll[256])


def fixed(w, tokens, bfinal=1):
    w.put(bfinal, 1); w.put(1, 2)
    ll, dc = codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), codes([5] * 32)
    put_tokens(w, ll, dc, tokens)
    w.code(ll[256])


def auto_dynamic(tokens, **kw):
    """a dynamic block whose codes are complete over exactly the symbols the tokens use"""
    lls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lls.add(t)
        else:
            lls.add(len_sym(t[0])[0]); ds.add(dist_sym(t[1])[0])
    if len(lls) == 1:
        lls.add(0)
    ll_lens = complete(lls, max(lls) + 1 if max(lls) >= 257 else 257)
    d_lens = complete(ds, max(ds) + 1) if ds else [0]
    w = Bits()
    dynamic(w, ll_lens, d_lens, tokens, **kw)
    return w.bytes()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _rng_text(n, seed=1):
    """compressible and not trivial: words of a small alphabet from an LCG"""
    out, x = bytearray(), seed
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += b"chr%d\t%d\t" % (x % 23, x >> 8 & 0xFFFFF) + (b"+\n" if x & 1 else b"-\t")
    return bytes(out[:n])


def _noise(n, seed=7):
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out.append(x >> 56)
    return bytes(out)


def _ok(family, name, gz, text):
    return {"name": name, "family": family, "gz": gz, "text": text, "refused": None}


def _bad(name, gz, reason):
    return {"name": name, "family": "refused", "gz": gz, "text": None, "refused": reason}


def _tok_case(family, name, tokens, writer=auto_dynamic):
    text = D.replay(tokens)
    return _ok(family, name, member(writer(tokens), text) + px2def.BGZF_EOF, text)


def _fixed_bytes(tokens):
    w = Bits()
    fixed(w, tokens)
    return w.bytes()


def _block_kinds():
    F = "block_kinds"
    t = _rng_text(30000)
    out = [_ok(F, "stored_level0", member(zraw(t, 0), t) + px2def.BGZF_EOF, t),
           _ok(F, "fixed", member(zraw(t, 6, zlib.Z_FIXED), t) + px2def.BGZF_EOF, t)]
    for lv in (1, 6, 9):
        out.append(_ok(F, "dynamic_level%d" % lv, member(zraw(t, lv), t) + px2def.BGZF_EOF, t))
    # one member, several deflate blocks of mixed types: full flushes and Z_BLOCK between pieces (empty stored blocks too)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = co.compress(t[:9000]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(_noise(3000)) + co.flush(zlib.Z_BLOCK) + co.compress(t[9000:15000]) + co.flush(zlib.Z_FULL_FLUSH)
    raw += co.compress(b"aaaa" * 50) + co.flush()
    mixed = t[:9000] + _noise(3000) + t[9000:15000] + b"aaaa" * 50
    out.append(_ok(F, "mixed_blocks_in_one_member", member(raw, mixed) + px2def.BGZF_EOF, mixed))
    out.append(_ok(F, "isize_0_member", member(b"\x03\0", b"") + member(zraw(t[:100]), t[:100]) + px2def.BGZF_EOF, t[:100]))
    a, b = t[:5000], t[5000:7001]
    out.append(_ok(F, "eof_in_the_middle", member(zraw(a), a) + px2def.BGZF_EOF + member(zraw(b, 1), b) + px2def.BGZF_EOF, a + b))
    out.append(_ok(F, "no_eof_at_the_end", member(zraw(a), a) + member(zraw(b), b), a + b))
    out.append(_ok(F, "empty_file", b"", b""))
    out.append(_ok(F, "eof_only", px2def.BGZF_EOF, b""))
    out.append(_ok(F, "isize_1", member(zraw(b"x"), b"x") + px2def.BGZF_EOF, b"x"))
    big = _rng_text(0x10000, 3)
    out.append(_ok(F, "isize_ff00", member(zraw(big[:0xFF00]), big[:0xFF00]) + px2def.BGZF_EOF, big[:0xFF00]))
    out.append(_ok(F, "isize_65536", member(zraw(big), big) + px2def.BGZF_EOF, big))
    # the largest stored block a member holds: BSIZE counts at most 65536 bytes, 26 of them frame and 5 the block's header (a stored
    # block of 65535 bytes, the most LEN can say, does not fit into BGZF)
    n = _noise(65505)
    out.append(_ok(F, "stored_65505_fills_the_member", member(b"\x01" + struct.pack("<HH", 65505, 65505 ^ 0xFFFF) + n, n) + px2def.BGZF_EOF, n))
    many = b"".join(member(zraw(t[k:k + 997], 1 + k % 3), t[k:k + 997]) for k in range(0, 30000, 997))
    out.append(_ok(F, "many_members_odd_offsets", many + px2def.BGZF_EOF, t))
    return out


def _matches():
    F = "matches"
    lit = list(b"abcdefghijklmnopqrstuvwxyz0123456789")
    out = [_tok_case(F, "length_3_and_258", lit + [(3, 36), (258, 36), (3, 1)]),
           _tok_case(F, "dist_1_len_258", [120, (258, 1), (258, 1)])]
    for d in (1, 2, 3, 4, 63, 64, 65):
        head = [65 + k % 26 for k in range(d)]
        out.append(_tok_case(F, "overlap_dist_%d" % d, head + [(max(d + 1, 3), d), (258, d), (d + 70, d)]))
    base = list(_noise(32768, 11))
    w = Bits()
    w.put(0, 1); w.put(0, 2); w.put(0, 5)
    stored = w.bytes() + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + bytes(base)
    w = Bits()
    toks = [(258, 32768), 7, (100, 32768)]
    ll_lens = complete({7, 256, len_sym(258)[0], len_sym(100)[0]}, 286)
    dynamic(w, ll_lens, complete({29}, 30), toks)
    text = D.replay(base + toks)
    out.append(_ok(F, "dist_32768", member(stored + w.bytes(), text) + px2def.BGZF_EOF, text))
    out.append(_tok_case(F, "match_ends_at_isize", lit + [(200, 17)]))
    # the kernel's batch: a match as the first token behind each boundary, one as the last token in front of it whose bytes the next
    # batch reads at once, and a match whose source the previous token of the same batch wrote
    for at in (BATCH, 2 * BATCH):
        toks = [97 + k % 26 for k in range(at)] + [(40, 5), 33, (9, 3)]
        out.append(_tok_case(F, "match_first_of_batch_at_%d" % at, toks))
    toks = [97 + k % 26 for k in range(BATCH - 1)] + [(100, 7), (258, 100), 33] + [97 + k % 7 for k in range(BATCH - 3)] + [(50, 2), (51, 50)]
    out.append(_tok_case(F, "matches_across_the_batch_edge", toks))
    out.append(_tok_case(F, "source_written_by_previous_token", [50, 51, (30, 1), 52, (4, 1), (5, 4), (258, 5), (3, 258)]))
    out.append(_tok_case(F, "fixed_code_matches", lit + [(3, 1), (258, 36), (10, 297)], writer=_fixed_bytes))
    return out


def _codes():
    F = "codes"
    out = []
    # 15-bit literal and distance codes
    lsyms = [256, 97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 257 + 5, 110, 111]        # 110 and 111 get the two 15-bit codes
    dsyms = list(range(16))
    toks = [97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 110, 111, 111, 110] * 14 + [(8, D.DIST_BASE[s]) for s in (15, 14, 0, 1)] + [111, (8, D.DIST_BASE[15] + 3)]
    w = Bits()
    dynamic(w, skewed(lsyms, 286), skewed(dsyms, 30), toks)
    text = D.replay(toks)
    out.append(_ok(F, "15_bit_codes_hlit_286_hdist_30", member(w.bytes(), text) + px2def.BGZF_EOF, text))
    # one distance code of length 1 (an incomplete set that is allowed)
    toks = [65, 66, 67, (10, 3), 68, (3, 3)]
    w = Bits()
    dynamic(w, complete({65, 66, 67, 68, 256, len_sym(10)[0], len_sym(3)[0]}, 265), [0, 0, 1], toks)
    out.append(_ok(F, "single_distance_code", member(w.bytes(), D.replay(toks)) + px2def.BGZF_EOF, D.replay(toks)))
    # literals only: HDIST 1 with the one length 0
    toks = list(b"only literals here")
    out.append(_tok_case(F, "literals_only_no_distance_code", toks))
    # repeats 16 / 17 / 18 that run across the literal/distance boundary; HCLEN 19
    ll_lens = [0] * 97 + [2, 2] + [0] * 157 + [2] + [0] * 3 + [2]            # a, b, end of block, length symbol 260 (6): 261 lengths
    d_lens = [2, 2, 2, 2] + [0] * 20
    toks = [97, 98, 97, 98, 97, (6, 2), (6, 4), (6, 1)]
    w = Bits()
    dynamic(w, ll_lens, d_lens, toks, cl_lens=CL_REPEATS, spell=[(18, 86), (2, 0), (2, 0), (18, 127), (18, 19 - 11), (2, 0), (17, 0), (2, 0), (16, 1), (18, 20 - 11)])
    out.append(_ok(F, "repeats_across_the_boundary", member(w.bytes(), D.replay(toks)) + px2def.BGZF_EOF, D.replay(toks)))
    # HCLEN 5 (the fewest that can spell an end-of-block code): symbols 16, 17, 18, 0 and 8; 256 codes of 8 bits
    cl = [0] * 19
    cl[0], cl[8] = 1, 1
    toks = [1, 2, 3, 255, 254, 7]
    w = Bits()
    dynamic(w, [0] + [8] * 256, [0], toks, cl_lens=cl, hclen=5)
    out.append(_ok(F, "hclen_5", member(w.bytes(), bytes(toks)) + px2def.BGZF_EOF, bytes(toks)))
    return out


def _refused():
    t = _rng_text(4000, 5)
    good = member(zraw(t), t)
    out = [_bad("bad_magic", b"\x1f\x8b\x07\x04" + good[4:] + px2def.BGZF_EOF, "bad_magic"),
           _bad("bad_magic_second_member", good + b"BAM\1" + good[4:], "bad_magic"),
           _bad("plain_gzip", gzip.compress(t, mtime=0), "plain_gzip"),
           _bad("xlen_8", good[:10] + b"\x08\0BC\x02\0" + good[16:18] + b"\0\0" + good[18:], "xlen"),
           _bad("bsize_past_the_end", good + good[:16] + struct.pack("<H", len(good) + 9) + good[18:], "past_file"),
           _bad("truncated_inside_a_member", good + good[:len(good) // 2], "past_file")]

    def m(raw, text=b"", **kw):
        return good + member(raw, text, **kw) + px2def.BGZF_EOF          # a good member first: the offset of the refused one is not 0

    out.append(_bad("block_type_3", m(b"\x07"), "block_type_3"))
    out.append(_bad("stored_nlen", m(b"\x01\x05\x00\x00\x00hello", b"hello"), "stored_nlen"))
    out.append(_bad("stored_padding", m(b"\x09\x05\x00\xfa\xffhello", b"hello"), "stored_padding"))
    abc = [97, 98, 99]

    def dyn(ll_lens, d_lens, toks, **kw):
        w = Bits()
        dynamic(w, ll_lens, d_lens, toks, **kw)
        return w.bytes()

    L = lambda d: [d.get(s, 0) for s in range(max(max(d) + 1, 257))]
    out.append(_bad("ll_oversubscribed", m(dyn(L({97: 1, 98: 1, 256: 1}), [0], [97]), b"a"), "ll_oversubscribed"))
    out.append(_bad("ll_incomplete", m(dyn(L({97: 2, 256: 1}), [0], [97]), b"a"), "ll_incomplete"))
    out.append(_bad("d_oversubscribed", m(dyn(L({97: 1, 256: 2, 257: 2}), [1, 1, 1], [97]), b"a"), "d_oversubscribed"))
    out.append(_bad("d_incomplete", m(dyn(L({97: 1, 256: 2, 257: 2}), [2, 2], [97]), b"a"), "d_incomplete"))
    out.append(_bad("d_single_code_of_length_2", m(dyn(L({97: 1, 256: 2, 257: 2}), [0, 2], [97]), b"a"), "d_incomplete"))
    over = [4] * 16 + [1, 0, 0]
    out.append(_bad("cl_oversubscribed", m(dyn(L({97: 1, 256: 1}), [0], [97], cl_lens=over), b"a"), "cl_oversubscribed"))
    inc = [4] * 15 + [0] * 4
    out.append(_bad("cl_incomplete", m(dyn(L({97: 1, 256: 1}), [0], [97], cl_lens=inc), b"a"), "cl_incomplete"))
    out.append(_bad("no_end_of_block_code", m(dyn([0] * 97 + [1, 1] + [0] * 158, [0], [97], eob=False), b"a"), "no_end_of_block"))
    cl4 = [0] * 19
    cl4[0], cl4[18] = 1, 1
    out.append(_bad("hclen_4_spells_only_zeros", m(dyn([0] * 257, [0], [], cl_lens=cl4, hclen=4, spell=[(18, 127), (18, 258 - 138 - 11)], eob=False)), "no_end_of_block"))
    out.append(_bad("repeat_at_the_first_length", m(dyn(L({97: 1, 256: 1}), [0], [97], cl_lens=CL_REPEATS, spell=[(16, 0)] + [(0, 0)] * 255), b"a"), "repeat_first"))
    out.append(_bad("repeat_past_the_last_length", m(dyn(L({97: 1, 256: 1}), [0], [97], cl_lens=CL_REPEATS, spell=[(18, 86), (1, 0), (18, 127), (18, 127)]), b"a"), "repeat_past_last"))
    w = Bits(); fixed(w, [97, ("L", 286)])
    out.append(_bad("length_symbol_286", m(w.bytes(), b"a"), "length_symbol"))
    w = Bits(); fixed(w, [97, 98, 99, ("L", 257), ("D", 30, 0)])
    out.append(_bad("distance_symbol_30", m(w.bytes(), b"abc"), "distance_symbol"))
    out.append(_bad("distance_before_the_start", m(auto_dynamic([97, 98, (3, 3)]), b"ab"), "distance_before_start"))
    out.append(_bad("distance_into_the_member_before", m(_fixed_bytes([(3, 1)])), "distance_before_start"))
    raw = zraw(t[:500])
    out.append(_bad("output_longer_than_isize", m(raw, t[:500], isize=499), "output_long"))
    out.append(_bad("match_runs_over_isize", m(auto_dynamic(abc + [(258, 3)]), D.replay(abc + [(258, 3)]), isize=200), "output_long"))
    out.append(_bad("output_shorter_than_isize", m(raw, t[:500], isize=501), "output_short"))
    out.append(_bad("wrong_isize", m(raw, t[:500], isize=600), "output_short"))
    out.append(_bad("stream_runs_past_its_span", m(raw[:-3], t[:500]), "past_span"))
    out.append(_bad("stored_runs_past_its_span", m(b"\x01\x10\x00\xef\xffhello", b"hello"), "past_span"))
    out.append(_bad("trailing_bytes", m(raw + b"\0", t[:500]), "trailing_bytes"))
    out.append(_bad("wrong_crc", m(raw, t[:500], crc=zlib.crc32(t[:500]) ^ 1), "crc"))
    flip = bytearray(zraw(_noise(300), 0)); flip[100] ^= 0x40
    out.append(_bad("a_flipped_stored_byte", m(bytes(flip), _noise(300)), "crc"))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _block_kinds() + _matches() + _codes() + _refused()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def accepted():
    return [c for c in cases() if c["refused"] is None]


def refused():
    return [c for c in cases() if c["refused"] is not None]


def refused_offset(c):
    """the file offset of the member that is refused: the first one px2def or the checks of a member turn down"""
    gz = c["gz"]
    p = 0
    while p < len(gz):
        if gz[p:p + 4] != b"\x1f\x8b\x08\x04" or len(gz) - p < 18 or gz[p + 10:p + 16] != b"\x06\0BC\x02\0":
            return p
        bsize = struct.unpack_from("<H", gz, p + 16)[0] + 1
        if p + bsize > len(gz):
            return p
        crc, isize = struct.unpack_from("<II", gz, p + bsize - 8)
        try:
            _, data = D.inflate(gz[p + 18:p + bsize - 8])
            if len(data) != isize or zlib.crc32(data) != crc:
                return p
        except D.InflateError:
            return p
        p += bsize
    raise AssertionError("nothing is refused in " + c["name"])
