"""TEST INFRASTRUCTURE: BAM records to SAM text, by definition.  A plain Python decoder of the inflated stream of a BAM (hts-specs SAMv1
4.2) to the bytes `samtools view`, `view -h` and `view -H` print (samtools 1.17; tests/golden/bamtext_golden.json records what it printed),
with the refusals include/mkt.h lists for mkt_bamtext: their reason, the ordinal of the record and its offset in the stream.  It shares no
code with the product; product code never imports this file."""
import struct
import zlib

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
MAX_RECORD = 16 << 20
INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


class Refused(ValueError):
    def __init__(self, reason, record, offset):
        ValueError.__init__(self, f"{reason}: record {record} at {offset}")
        self.reason, self.record, self.offset = reason, record, offset


def inflate(bam: bytes) -> bytes:
    """the inflated stream of a BGZF file (zlib checks every member)"""
    out, p = [], 0
    while p < len(bam):
        bsize = struct.unpack_from("<H", bam, p + 16)[0] + 1
        out.append(zlib.decompress(bam[p:p + bsize], wbits=31))
        p += bsize
    return b"".join(out)


def float_text(bits: int) -> bytes:
    """%g of the single (the golden decides whether samtools prints the same)"""
    return b"%g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def header(raw: bytes):
    """-> (stored text, [(name, length)], offset of the first record); Refused for a stream whose header is refused or not complete"""
    n = len(raw)
    if raw[:4] != b"BAM\1"[:min(n, 4)]:
        raise Refused("bad_magic", 0, 0)
    short = Refused("header_truncated", 0, n)
    if n < 8:
        raise short
    l_text = struct.unpack_from("<i", raw, 4)[0]
    if l_text < 0:
        raise Refused("bad_header", 0, 0)
    p = 8 + l_text
    if p + 4 > n:
        raise short
    n_ref = struct.unpack_from("<i", raw, p)[0]
    if n_ref < 0:
        raise Refused("bad_header", 0, 0)
    p += 4
    refs = []
    for _ in range(n_ref):
        if p + 4 > n:
            raise short
        l_name = struct.unpack_from("<i", raw, p)[0]
        if l_name < 1:
            raise Refused("bad_header", 0, 0)
        if p + 8 + l_name > n:
            raise short
        name = raw[p + 4:p + 4 + l_name]
        if name[-1] != 0:
            raise Refused("bad_header", 0, 0)
        refs.append((name.split(b"\0")[0], struct.unpack_from("<i", raw, p + 4 + l_name)[0]))
        p += 8 + l_name
    text = raw[8:8 + l_text]
    shown = text.rstrip(b"\0")
    if b"\0" in shown:
        raise Refused("header_nul", 0, 0)
    if n_ref and not (shown.startswith(b"@SQ\t") or b"\n@SQ\t" in shown):
        raise Refused("no_sq_lines", 0, 0)
    return text, refs, p


def header_text(stored: bytes) -> bytes:
    """what `view -H` prints"""
    body = stored.rstrip(b"\0")
    if not body or body.endswith(b"\n"):
        return stored
    return body + b"\n" + stored[len(body) + 1:]          # the newline takes the place of the first NUL where there is one


def _tags(b, p, end, fail):
    out = []
    while p < end:
        if p + 3 > end:
            fail("tag_overrun")
        tag, ty = b[p:p + 2], chr(b[p + 2])
        p += 3
        if ty == "A":
            if p + 1 > end:
                fail("tag_overrun")
            out.append(tag + b":A:" + b[p:p + 1])
            p += 1
        elif ty in INT_FMT:
            size = struct.calcsize(INT_FMT[ty])
            if p + size > end:
                fail("tag_overrun")
            out.append(tag + b":i:%d" % struct.unpack_from(INT_FMT[ty], b, p)[0])
            p += size
        elif ty == "f":
            if p + 4 > end:
                fail("tag_overrun")
            out.append(tag + b":f:" + float_text(struct.unpack_from("<I", b, p)[0]))
            p += 4
        elif ty in "ZH":
            e = b.find(b"\0", p, end)
            if e < 0:
                fail("z_unterminated")
            out.append(tag + b":" + ty.encode() + b":" + b[p:e])
            p = e + 1
        elif ty == "B":
            if p + 5 > end:
                fail("tag_overrun")
            sub = chr(b[p])
            if sub not in "cCsSiIf":
                fail("b_subtype")
            cnt = struct.unpack_from("<I", b, p + 1)[0]
            size = 4 if sub == "f" else struct.calcsize(INT_FMT[sub])
            if p + 5 + cnt * size > end:
                fail("tag_overrun")
            if tag == b"CG" and sub == "I":
                fail("cg_tag")
            if sub == "f":
                vals = [float_text(v) for v in struct.unpack_from("<%dI" % cnt, b, p + 5)]
            else:
                vals = [b"%d" % v for v in struct.unpack_from("<%d%s" % (cnt, INT_FMT[sub][1]), b, p + 5)]
            out.append(tag + b":B:" + sub.encode() + b"".join(b"," + v for v in vals))
            p += 5 + cnt * size
        else:
            fail("tag_type")
    return out


def line(raw: bytes, off: int, refs, ordinal=0) -> bytes:
    """the SAM line (with its newline) of the complete record at off"""
    def fail(reason):
        raise Refused(reason, ordinal, off)
    bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<IiiBBHHHIiii", raw, off)
    end = off + 4 + bs
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        fail("past_end")
    if not (-1 <= tid < len(refs) and -1 <= mtid < len(refs)):
        fail("ref_id")
    p = off + 36
    if l_name < 1 or raw[p + l_name - 1] != 0:
        fail("read_name")
    qname = raw[p:p + l_name].split(b"\0")[0]
    p += l_name
    cig, qlen = b"", 0
    for v in struct.unpack_from("<%dI" % n_cig, raw, p):
        if v & 15 > 8:
            fail("cigar_op")
        cig += b"%d%c" % (v >> 4, CIGAR_OPS[v & 15])
        qlen += (v >> 4) if v & 15 in (0, 1, 4, 7, 8) else 0
    if n_cig and l_seq and not flag & 4 and qlen != l_seq:
        fail("cigar_seq_length")                          # samtools ends with "CIGAR and query sequence lengths differ"
    p += 4 * n_cig
    packed = raw[p:p + (l_seq + 1) // 2]
    seq = bytes(SEQ_CODES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    p += (l_seq + 1) // 2
    q = raw[p:p + l_seq]
    qual = b"*" if not l_seq or q[0] == 0xFF else bytes((x + 33) & 255 for x in q)
    p += l_seq
    rname = b"*" if tid < 0 else refs[tid][0]
    rnext = b"*" if mtid < 0 else b"=" if mtid == tid else refs[mtid][0]
    f = [qname, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cig or b"*", rnext, b"%d" % (mpos + 1), b"%d" % tlen, seq or b"*", qual]
    return b"\t".join(f + _tags(raw, p, end, fail)) + b"\n"


def decode(raw: bytes, max_record=MAX_RECORD, first_record=0, stream_offset=0):
    """-> (header text as view -H prints it, refs, [lines]) of a whole stream; Refused as the decoder refuses it"""
    text, refs, p = header(raw)
    lines, k = [], first_record
    while p < len(raw):
        if p + 4 > len(raw):
            raise Refused("truncated", k, stream_offset + p)
        bs = struct.unpack_from("<I", raw, p)[0]
        if bs < 32:
            raise Refused("block_size_small", k, stream_offset + p)
        if bs > max_record:
            raise Refused("block_size_large", k, stream_offset + p)
        if p + 4 + bs > len(raw):
            raise Refused("truncated", k, stream_offset + p)
        try:
            lines.append(line(raw, p, refs, k))
        except Refused as e:
            raise Refused(e.reason, k, stream_offset + p)
        p += 4 + bs
        k += 1
    return header_text(text), refs, lines


def view(raw: bytes, mode=""):
    """the bytes of `samtools view` (mode ""), `view -h` ("h") and `view -H` ("H")"""
    h, _, lines = decode(raw)
    return {"": b"".join(lines), "h": h + b"".join(lines), "H": h}[mode]
