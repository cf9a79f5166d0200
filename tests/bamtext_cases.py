"""TEST INFRASTRUCTURE: directed BAM streams for the BAM-to-SAM decoder, built with struct (records samtools itself would not write) and
compressed with Python's zlib.  Families: lengths, numbers, tags, segments (edges of the record index at segment_bytes = 256), refused.
A case is a dict: name, raw (the inflated stream), and for a refused one `refused` = (reason key, record ordinal, stream offset) and
maybe `opts`.  tests/golden/make_bamtext_golden.py records what samtools printed for the accepted ones."""
import struct
import zlib

TEXT = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chr10\tLN:133797422\n@SQ\tSN:chrM\tLN:16569\n"
REFS = [(b"chr1", 248956422), (b"chr10", 133797422), (b"chrM", 16569)]
SEGMENT = 256
FLOATS = [0x00000000, 0x80000000, 0x3FC00000, 0x3727C5AC, 0x47F12059, 0x501502F9, 0x7F7FC99E, 0x00000001]      # 0, -0.0, 1.5, 1e-5, 123456.7, 1e10, 3.4e38, a denormal
BASES = "=ACMGRSVTWYHKDBN"


def header(text=TEXT, refs=REFS, n_ref=None):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs) if n_ref is None else n_ref)
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return out


HEADER = header()
START = len(HEADER)


def pack_seq(seq: str) -> bytes:
    codes = [BASES.index(c) for c in seq] + [0]
    return bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))


def rec(name=b"r", flag=0, tid=0, pos=99, mapq=60, cigar=((10, 0),), mtid=-1, mpos=-1, tlen=0, seq="ACGTACGTAC", qual=None, tags=b"", l_seq=None, l_name=None,
        block_size=None, seq_bytes=None):
    """one record with its block_size; every field can be set against the others"""
    qual = bytes([30] * len(seq)) if qual is None else qual
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(nm) if l_name is None else l_name, mapq, 4680, len(cigar), flag, len(seq) if l_seq is None else l_seq, mtid, mpos, tlen)
    body += nm + b"".join(struct.pack("<I", (n << 4) | op) for n, op in cigar) + (pack_seq(seq) if seq_bytes is None else seq_bytes) + qual + tags
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def tag(name, ty, v=None, sub=None):
    t = name.encode() + ty.encode()
    if ty == "A":
        return t + v
    if ty in "ZH":
        return t + v + b"\0"
    if ty == "f":
        return t + struct.pack("<I", v)
    if ty == "B":
        fmt = "I" if sub == "f" else {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[sub]
        return t + sub.encode() + struct.pack("<I", len(v)) + struct.pack("<%d%s" % (len(v), fmt), *v)
    return t + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[ty], v)


def bgzf(raw: bytes, block=0xFF00, level=6) -> bytes:
    out = []
    for k in range(0, max(len(raw), 1), block):
        piece = raw[k:k + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        d = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out) + bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _seq(n):
    return "".join(BASES[(7 * i + 3) % 16] for i in range(n))


def _qual(n):
    return bytes((11 * i + 2) % 42 for i in range(n))


def padded(total, **kw):
    """a record of exactly `total` bytes (block_size included): an XP:Z tag takes up the slack"""
    base = len(rec(tags=tag("XP", "Z", b""), **kw))
    assert total >= base, (total, base)
    return rec(tags=tag("XP", "Z", b"p" * (total - base)), **kw)


OPS70 = tuple((1 + k % 3, k % 9) for k in range(70))
OPS70_Q = sum(n for n, op in OPS70 if op in (0, 1, 4, 7, 8))          # the bases the operations take from the read


def _lengths():
    recs = [rec(name=b"len%d" % n, seq=_seq(n), qual=_qual(n), cigar=((n, 0),) if n else ()) for n in (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)]
    recs += [rec(name=b""), rec(name=b"n"), rec(name=b"N" * 254), rec(name=b"noqual", seq=_seq(33), qual=b"\xff" * 33, cigar=((33, 0),)), rec(name=b"nocigar", cigar=()), rec(name=b"oneop", cigar=((10, 0),)),
             rec(name=b"ops70", seq=_seq(OPS70_Q), qual=_qual(OPS70_Q), cigar=OPS70), rec(name=b"qhigh", seq=_seq(9), qual=bytes([0, 93, 94, 200, 222, 223, 254, 1, 255]), cigar=((9, 0),))]
    return recs


def _numbers():
    recs = [rec(name=b"pos_m1", pos=-1, tid=-1, cigar=()), rec(name=b"pos_max", pos=2 ** 31 - 2), rec(name=b"mpos_max", mtid=1, mpos=2 ** 31 - 2)]
    recs += [rec(name=b"tlen%d" % k, tlen=v) for k, v in enumerate((-(2 ** 31 - 1), -1, 0, 2 ** 31 - 1))]
    recs += [rec(name=b"flag0", flag=0), rec(name=b"flag65535", flag=65535), rec(name=b"mapq255", mapq=255), rec(name=b"mapq0", mapq=0)]
    for ty, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", -2 ** 31, 2 ** 31 - 1), ("I", 0, 2 ** 32 - 1)):
        vals = [lo, hi] + [10 ** k for k in range(10) if 10 ** k <= hi] + [-(10 ** k) for k in range(10) if -(10 ** k) >= lo] + [10 ** k - 1 for k in range(1, 10) if 10 ** k - 1 <= hi]
        recs.append(rec(name=b"int_" + ty.encode(), tags=b"".join(tag("X%s" % "abcdefghijklmnopqrstuvwxyzABCDEFGHIJ"[k], ty, v) for k, v in enumerate(vals))))
    for tid in (-1, 0, 2):
        for mtid in (-1, 0, 2):
            recs.append(rec(name=b"ref%d_%d" % (tid + 1, mtid + 1), tid=tid, mtid=mtid, pos=5 if tid >= 0 else -1, mpos=7 if mtid >= 0 else -1))
    return recs


def _tags(floats):
    recs = [rec(name=b"types", tags=tag("XA", "A", b"q") + tag("Xc", "c", -5) + tag("XC", "C", 5) + tag("Xs", "s", -500) + tag("XS", "S", 500) + tag("Xi", "i", -70000) + tag("XI", "I", 70000) +
                tag("XZ", "Z", b"some text") + tag("XH", "H", b"1AE301") + tag("XE", "Z", b""))]
    for sub in "cCsSiI":
        lo = {"c": -128, "s": -32768, "i": -2 ** 31}.get(sub, 0)
        for n in (0, 1, 300):
            recs.append(rec(name=b"B%s%d" % (sub.encode(), n), tags=tag("XB", "B", [lo + (k * 37) % 200 for k in range(n)], sub) + tag("NM", "C", 1)))
    if floats:
        recs.append(rec(name=b"floats", tags=b"".join(tag("F%d" % k, "f", v) for k, v in enumerate(FLOATS)) + tag("NM", "C", 2)))
        for n in (0, 1, 300):
            recs.append(rec(name=b"Bf%d" % n, tags=tag("XB", "B", [FLOATS[k % len(FLOATS)] for k in range(n)], "f") + tag("XZ", "Z", b"behind")))
        recs.append(rec(name=b"nofloat", tags=tag("NM", "C", 3)))
    return recs


def decoy(n=4):
    """a chain of n records whose fixed fields are plausible: what a guess takes for record starts"""
    return b"".join(struct.pack("<IiiBBHHHIiii", 34, 0, 7, 2, 0, 4680, 0, 0, 0, -1, -1, 0) + b"d\0" for _ in range(n))


def _segments(kind):
    S = SEGMENT
    small = dict(seq="ACGT", qual=b"\x1e" * 4, cigar=((4, 0),))
    tail = [rec(name=b"t%d" % k, **small) for k in range(9)]
    if kind.startswith("edge"):
        d = int(kind[4:])                                # a record that starts d bytes before the first segment edge
        return [padded(S - d, name=b"first", **small), rec(name=b"at_edge", seq=_seq(40), qual=_qual(40), cigar=((40, 0),))] + tail
    if kind == "long_z":                                 # a record longer than three segments
        return [rec(name=b"a", **small), rec(name=b"long", tags=tag("XL", "Z", bytes(33 + k % 90 for k in range(900))), **small)] + tail
    if kind == "last_one_byte":                          # the last segment holds one byte
        recs = [rec(name=b"a", **small), rec(name=b"b", **small)]
        used = sum(len(r) for r in recs)
        return recs + [padded(2 * S + 1 - used, name=b"c", **small)]
    if kind in ("decoy_qual", "decoy_b"):
        # Plausible records inside a payload, right behind a segment edge, in the segment the record ends in: the guess of that segment
        # takes the decoy, the true start lies behind it.  (A Z payload cannot hold one: it has no NUL, so every 32-bit field in it is at
        # least 0x01010101, above the largest block_size accepted; the B:C array stands in for it.)
        if kind == "decoy_b":
            n, r0 = 700, lambda payload: rec(name=b"dd", tags=tag("XB", "B", list(payload), "C"), **small)
        else:
            n, r0 = 600, lambda payload: rec(name=b"dd", seq=_seq(len(payload)), qual=payload, cigar=((len(payload), 0),))
        probe = r0(bytes([40]) * n)
        at = probe.index(bytes([40]) * n)                # where the payload begins in the record
        edge = len(probe) // S * S                       # the record ends inside the segment that begins here
        payload = bytearray(bytes([40]) * n)
        dc = decoy()
        assert at <= edge and edge - at + len(dc) <= n, kind
        payload[edge - at:edge - at + len(dc)] = dc
        r = r0(bytes(payload))
        assert r[edge:edge + len(dc)] == dc and edge < len(r) < edge + S, (kind, len(r))
        return [r] + tail
    raise KeyError(kind)


SEGMENT_KINDS = ["edge0", "edge1", "edge3", "edge4", "edge35", "edge36", "long_z", "last_one_byte", "decoy_qual", "decoy_b"]


def _stream(recs, hdr=HEADER):
    return hdr + b"".join(recs)


def accepted(floats=True):
    out = [{"name": "lengths", "raw": _stream(_lengths())}, {"name": "numbers", "raw": _stream(_numbers())}, {"name": "tags", "raw": _stream(_tags(False))}]
    if floats:
        out.append({"name": "floats", "raw": _stream(_tags(True))})
    out += [{"name": "seg_" + k, "raw": _stream(_segments(k)), "repairs": k.startswith("decoy")} for k in SEGMENT_KINDS]
    out += [{"name": "no_records", "raw": HEADER}, {"name": "no_refs", "raw": _stream([rec(name=b"u", tid=-1, pos=-1, cigar=())], header(b"@HD\tVN:1.6\n", []))},
            {"name": "text_without_newline", "raw": _stream([rec()], header(TEXT[:-1]))}, {"name": "text_with_nul", "raw": _stream([rec()], header(TEXT + b"\0\0\0"))},
            {"name": "text_nul_no_newline", "raw": _stream([rec()], header(TEXT[:-1] + b"\0\0"))},
            {"name": "text_only_nul", "raw": _stream([rec(name=b"u", tid=-1, pos=-1, cigar=())], header(b"\0\0", []))},
            {"name": "empty_text_no_refs", "raw": _stream([rec(name=b"u", tid=-1, pos=-1, cigar=())], header(b"", []))}]
    return out


def refused():
    good = [rec(name=b"g%d" % k) for k in range(3)]
    at = START + sum(len(r) for r in good)               # the offset of record 3

    def one(name, bad, reason, **kw):
        return dict(name=name, raw=_stream(good + [bad] + good), refused=(reason, 3, at), **kw)
    out = [one("block_size_small", rec(block_size=31), "block_size_small"),
           one("past_end", rec(l_seq=11), "past_end"),
           one("tag_overrun", rec(tags=tag("NM", "C", 1) + tag("Xi", "i", 5)[:-1]), "tag_overrun"),
           one("tag_type", rec(tags=b"XXq\0"), "tag_type"),
           one("b_subtype", rec(tags=b"XBBd" + struct.pack("<I", 0)), "b_subtype"),
           one("z_unterminated", rec(tags=b"XZZabc"), "z_unterminated"),
           one("ref_id", rec(tid=len(REFS)), "ref_id"),
           one("next_ref_id", rec(mtid=len(REFS)), "ref_id"),
           one("read_name", rec(name=b"abc", l_name=3), "read_name"),
           one("cigar_op", rec(cigar=((10, 9),)), "cigar_op"),
           one("cg_tag", rec(cigar=((10, 4), (10, 3)), tags=tag("CG", "B", [160], "I")), "cg_tag"),
           one("cigar_seq_length", rec(cigar=((4, 4), (5, 0), (3, 2))), "cigar_seq_length"),
           one("max_record", rec(seq=_seq(200), qual=_qual(200), cigar=((200, 0),)), "block_size_large", opts={"max_record": 128}),
           {"name": "bad_magic", "raw": b"BAM\2" + HEADER[4:] + b"".join(good), "refused": ("bad_magic", 0, 0)},
           {"name": "negative_l_text", "raw": b"BAM\1" + struct.pack("<i", -1) + HEADER[8:], "refused": ("bad_header", 0, 0)},
           {"name": "ref_name_without_nul", "raw": HEADER.replace(b"chr10\0", b"chr10x") + b"".join(good), "refused": ("bad_header", 0, 0)},
           {"name": "header_nul", "raw": _stream(good, header(TEXT[:30] + b"\0" + TEXT[30:])), "refused": ("header_nul", 0, 0)},
           {"name": "no_sq_lines", "raw": _stream(good, header(b"@HD\tVN:1.6\n")), "refused": ("no_sq_lines", 0, 0)}]
    big = header(n_ref=1000)
    out.append({"name": "n_ref_past_data", "raw": big, "refused": ("header_truncated", 0, len(big))})
    cut = _stream(good)[:-5]
    out.append({"name": "truncated", "raw": cut, "refused": ("truncated", 2, START + len(good[0]) + len(good[1]))})
    return out


def big(n=70000, bad_at=None):
    """A stream of n small records whose QUAL compresses badly (more than 64 KiB of BGZF, more than 256 blocks of 256 records, thousands
    of segments at SEGMENT); bad_at: that record carries a tag of an unknown type.  -> (stream, offset of record bad_at or None)"""
    out, off, bad = [HEADER], START, None
    x = 12345
    for k in range(n):
        q = bytearray(20)
        for i in range(20):
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            q[i] = (x >> 16) % 42
        r = rec(name=b"b%d" % k, pos=k, seq=_seq(20), qual=bytes(q), cigar=((20, 0),), tags=b"XXq\0" if k == bad_at else tag("NM", "C", k & 255))
        if k == bad_at:
            bad = off
        out.append(r)
        off += len(r)
    return b"".join(out), bad


_big = {}


def big_case(bad_at=None):
    """big() once per process, with its BGZF file and (bad_at None) the text tests/bamtextdef.py gives for it"""
    if bad_at not in _big:
        import bamtextdef
        raw, bad = big(bad_at=bad_at)
        _big[bad_at] = {"raw": raw, "bam": bgzf(raw), "bad_offset": bad, "lines": bamtextdef.decode(raw)[2] if bad_at is None else None}
    return _big[bad_at]


_golden = None


def golden():
    """tests/golden/bamtext_golden.json"""
    global _golden
    if _golden is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bamtext_golden.json")) as f:
            _golden = json.load(f)
    return _golden


def unz(s):
    import base64
    return zlib.decompress(base64.b64decode(s))


def inflate(bam: bytes) -> bytes:
    """the inflated stream of a BGZF file (zlib checks every member)"""
    out, p = [], 0
    while p < len(bam):
        bsize = struct.unpack_from("<H", bam, p + 16)[0] + 1
        out.append(zlib.decompress(bam[p:p + bsize], wbits=31))
        p += bsize
    return b"".join(out)


def golden_raw(key):
    """the inflated stream a golden entry stands for"""
    return inflate(unz(golden()[key]["bam"])) if key.startswith("sam/") else case(key[5:])["raw"]


def case(name):
    for c in accepted() + refused():
        if c["name"] == name:
            return c
    raise KeyError(name)
