"""TEST INFRASTRUCTURE: the BAM record stream, by definition.  A plain Python encoder SAM text -> BAM bytes (before BGZF), written
from the published specification (hts-specs SAMv1: 1.4 the alignment line, 4.2 the BAM layout, 5.3 reg2bin) plus the conventions
DESIGN.md states for the GPU writer ("N3" and "The records, exactly"): the htslib ones the specification leaves open.  It shares no
code with the product and never imports it; tests/bamio.py is the independent READER of the same section, this is the WRITER, and
tests/test_bamdef_host.py holds the two against each other.  All text is handled as bytes (a SAM line need not be UTF-8).

    header_bytes(header_text, sorted)        magic, l_text, text, n_ref, (l_name, name NUL, l_ref)*
    record_bytes(line, ref_ids)              one alignment line -> block_size + record; raises Reject where the writer must refuse
    stream_bytes(header_text, lines, sorted) header + records, in input order or in the stable coordinate order
    float32_exact(text)                      decimal text -> the bits of the nearest IEEE-754 single, ties to even, by exact rationals
    explain(got, header_text, lines, sorted) "" or the first differing record and field, in words
"""
import re
import struct
from fractions import Fraction

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = b"MIDNSHP=X"
REF_CONSUMING = frozenset(b"MDN=X")


class Reject(ValueError):
    """the line is not an alignment the writer accepts"""


# ---- numbers ---------------------------------------------------------------------------------------------------------------------
_UINT = re.compile(rb"[0-9]{1,19}\Z")
_SINT = re.compile(rb"[+-]?[0-9]{1,19}\Z")
_FLOAT = re.compile(rb"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]{1,19}))?\Z")


def _uint(b, hi, what):
    if not _UINT.match(b) or int(b) > hi:
        raise Reject(f"{what}: {b[:40]!r}")
    return int(b)


def _sint(b, lo, hi, what):
    if not _SINT.match(b) or not lo <= int(b) <= hi:
        raise Reject(f"{what}: {b[:40]!r}")
    return int(b)


def decimal_parts(text):
    """(negative, integer mantissa M, power of ten E) with value = M * 10^E, or None when the text is no decimal number.
    Grammar: [+-] digits [. digits] [e|E [+-] digits], at least one digit in the mantissa, the exponent within +-400."""
    if isinstance(text, str):
        text = text.encode()
    m = _FLOAT.match(text)
    if not m:
        return None
    sign, ip, fp, ex = m.groups()
    fp = fp or b""
    if not ip and not fp:
        return None
    e = int(ex) if ex is not None else 0
    if abs(e) > 400:
        return None
    return sign == b"-", int(ip + fp), e - len(fp)


def _f32_round(neg, M, E):
    """bits of the single nearest to (-1)^neg * M * 10^E, ties to even: integer / Fraction arithmetic only"""
    s = 0x80000000 if neg else 0
    if M == 0:
        return s
    v = Fraction(M * 10 ** E) if E >= 0 else Fraction(M, 10 ** -E)
    # 2^e <= v < 2^(e + 1)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if v < Fraction(2) ** e:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    e = max(e, -126)                                     # below the smallest normal number the spacing stays 2^-149
    n = v / Fraction(2) ** (e - 23)                      # v in units of the spacing there
    r = n.numerator // n.denominator
    rem = n - r
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and r & 1):
        r += 1
    if r == 1 << 24:
        r, e = 1 << 23, e + 1
    if e > 127:
        return s | 0x7F800000                            # beyond the largest finite single by half a spacing or more: infinity
    if r < 1 << 23:
        return s | r                                     # subnormal (or zero)
    return s | (e + 127) << 23 | (r - (1 << 23))


def float32_exact(text):
    """Decimal text -> the bit pattern (int) of the IEEE-754 single nearest its exact rational value, ties to even.  No Python
    float takes part: float() then struct.pack('f') rounds twice, which is the very error the tests look for."""
    parts = decimal_parts(text)
    if parts is None:
        raise Reject(f"not a decimal number: {text[:40]!r}")
    return _f32_round(*parts)


def f32_ordinal(bits):
    """singles on one line: consecutive values differ by 1; -0 and +0 coincide; +-infinity follow the largest finite values"""
    mag = bits & 0x7FFFFFFF
    return -mag if bits >> 31 else mag


def ulps_between(bits_a, bits_b):
    return abs(f32_ordinal(bits_a) - f32_ordinal(bits_b))


def float32_ulps(text, bits):
    """how many singles lie between `bits` and the correctly rounded value of the decimal text (0: it is the correct rounding)"""
    return ulps_between(float32_exact(text), bits)


def f32_class(bits):
    mag = bits & 0x7FFFFFFF
    return (bits >> 31, "zero" if mag == 0 else "inf" if mag == 0x7F800000 else "nan" if mag > 0x7F800000 else "finite")


def f32_value(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# ---- header ----------------------------------------------------------------------------------------------------------------------
def split_sam(sam: bytes):
    """SAM text -> (header text, alignment lines).  The leading '@' lines are the header; a line ends at \\n, one \\r before it does
    not belong to the line; a last line need not end with a newline."""
    p = 0
    while p < len(sam) and sam[p:p + 1] == b"@":
        e = sam.find(b"\n", p)
        p = len(sam) if e < 0 else e + 1
    header = sam[:p]
    if header and not header.endswith(b"\n"):
        header += b"\n"
    body = sam[p:]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return header, [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def references(header_text: bytes):
    """[(name, length)] from the @SQ lines, in order"""
    out = []
    for ln in header_text.split(b"\n"):
        if ln[:3] == b"@SQ":
            f = dict((x[:2], x[3:]) for x in ln.split(b"\t")[1:] if x[2:3] == b":")
            out.append((f[b"SN"], int(f[b"LN"])))
    return out


def header_text_out(header_text: bytes, sorted_: bool) -> bytes:
    """the text a file carries: unchanged in input order; sorted, @HD says SO:coordinate and no longer claims a grouping"""
    if not sorted_:
        return header_text
    if header_text[:3] != b"@HD":
        return b"@HD\tVN:1.6\tSO:coordinate\n" + header_text
    first, nl, rest = header_text.partition(b"\n")
    fields = [f for f in first.split(b"\t") if f[:3] != b"GO:"]
    if any(f[:3] == b"SO:" for f in fields):
        fields = [b"SO:coordinate" if f[:3] == b"SO:" else f for f in fields]
    else:
        fields.append(b"SO:coordinate")
    return b"\t".join(fields) + nl + rest


def header_bytes(header_text: bytes, sorted_: bool) -> bytes:
    text = header_text_out(header_text, sorted_)
    refs = references(header_text)
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
    return out


# ---- one record ------------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """SAMv1 5.3"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


_CIGAR_ITEM = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_INT_FMT = {"c": ("<b", -128, 127), "C": ("<B", 0, 255), "s": ("<h", -32768, 32767), "S": ("<H", 0, 65535),
            "i": ("<i", -(1 << 31), (1 << 31) - 1), "I": ("<I", 0, (1 << 32) - 1)}


def _cigar(field):
    if field == b"*":
        return None
    items = _CIGAR_ITEM.findall(field)
    if not items or b"".join(n + o for n, o in items) != field:
        raise Reject(f"CIGAR {field[:40]!r}")
    if len(items) > 65535 or any(int(n) >= 1 << 28 for n, _ in items):
        raise Reject("CIGAR: too many operations or a length of 2^28 or more")
    return [(int(n), o[0]) for n, o in items]


def _tag(field, floats):
    if len(field) < 5 or field[2:3] != b":" or field[4:5] != b":":
        raise Reject(f"tag {field[:40]!r}")
    name, ty, val = field[:2], chr(field[3]), field[5:]
    if ty in "AacC":                                     # htslib reads the lower-case and the integer letters as a character
        if len(val) != 1:
            raise Reject(f"tag {field[:40]!r}: one character")
        return name + b"A" + val
    if ty in "iI":
        v = _sint(val, -(1 << 31), (1 << 32) - 1, "integer tag")
        if val[:1] == b"-":                              # smallest type: signed when the text carries a minus sign, else unsigned
            c = "c" if v >= -128 else "s" if v >= -32768 else "i"
        else:
            c = "C" if v <= 255 else "S" if v <= 65535 else "I"
        return name + c.encode() + struct.pack(_INT_FMT[c][0], v)
    if ty == "f":
        floats.append((len(name) + 1, val))
        return name + b"f" + struct.pack("<I", float32_exact(val))
    if ty in "ZH":
        return name + ty.encode() + val + b"\0"
    if ty == "B":
        sub = chr(val[0]) if val else ""
        if sub not in tuple("cCsSiIf") or (len(val) > 1 and val[1:2] != b","):
            raise Reject(f"tag {field[:40]!r}: array subtype")
        elems = val[2:].split(b",") if len(val) > 1 else []
        out = name + b"B" + sub.encode() + struct.pack("<i", len(elems))
        for x in elems:
            if sub == "f":
                floats.append((len(out), x))
                out += struct.pack("<I", float32_exact(x))
            else:
                fmt, lo, hi = _INT_FMT[sub]
                out += struct.pack(fmt, _sint(x, lo, hi, "array element"))
        return out
    raise Reject(f"tag type {ty!r}")


def record_layout(line: bytes, ref_ids: dict):
    """-> (record bytes with block_size, [(offset of a float word in them, its decimal text)])"""
    f = line.split(b"\t")
    if len(f) < 11:
        raise Reject("fewer than eleven fields")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if not 1 <= len(qname) <= 254:
        raise Reject("QNAME length")
    flag = _uint(flag, 65535, "FLAG")
    pos = _sint(pos, 0, (1 << 31) - 1, "POS")
    mapq = _uint(mapq, 255, "MAPQ")
    pnext = _sint(pnext, 0, (1 << 31) - 1, "PNEXT")
    tlen = _sint(tlen, -(1 << 31), (1 << 31) - 1, "TLEN")

    def ref(name):
        if name not in ref_ids:
            raise Reject(f"reference {name[:40]!r} not in the header")
        return ref_ids[name]
    tid = -1 if rname == b"*" else ref(rname)
    mtid = -1 if rnext == b"*" else tid if rnext == b"=" else ref(rnext)
    ops = _cigar(cigar)
    if pos == 0 or tid < 0 or ops is None:               # no place or no alignment: the read counts as unmapped
        flag |= 4
    ops = ops or []
    l_seq = 0 if seq == b"*" else len(seq)
    if qual != b"*" and len(qual) != l_seq:
        raise Reject("SEQ and QUAL lengths differ")
    span = sum(n for n, o in ops if o in REF_CONSUMING)
    if flag & 4 or span == 0:
        span = 1
    codes = [SEQ_CODES.find(bytes([c]).upper()) for c in seq[:l_seq]]
    codes = [15 if c < 0 else c for c in codes] + [0]    # an odd tail: low nibble zero
    body = struct.pack("<iiBBHHHiiii", tid, pos - 1, len(qname) + 1, mapq, reg2bin(pos - 1, pos - 1 + span) & 0xFFFF, len(ops), flag, l_seq, mtid, pnext - 1, tlen)
    body += qname + b"\0"
    body += b"".join(struct.pack("<I", n << 4 | CIGAR_OPS.index(bytes([o]))) for n, o in ops)
    body += bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
    body += b"\xff" * l_seq if qual == b"*" else bytes(q - 33 & 0xFF for q in qual)
    floats = []
    for t in f[11:]:
        mine = []
        enc = _tag(t, mine)
        floats += [(4 + len(body) + o, txt) for o, txt in mine]
        body += enc
    return struct.pack("<i", len(body)) + body, floats


def record_bytes(line: bytes, ref_ids: dict) -> bytes:
    return record_layout(line, ref_ids)[0]


def ref_ids_of(header_text: bytes):
    return {n: i for i, (n, _) in enumerate(references(header_text))}


def file_order(lines, ref_ids, sorted_):
    """indices of the lines in file order: input order, or stable by (reference with none last, POS, reverse strand)"""
    if not sorted_:
        return list(range(len(lines)))

    def key(i):
        f = lines[i].split(b"\t")
        return (ref_ids[f[2]] if f[2] != b"*" else len(ref_ids), int(f[3]), 1 if int(f[1]) & 16 else 0)
    return sorted(range(len(lines)), key=key)


def stream_bytes(header_text: bytes, lines, sorted_: bool) -> bytes:
    ids = ref_ids_of(header_text)
    recs = [record_bytes(ln, ids) for ln in lines]
    return header_bytes(header_text, sorted_) + b"".join(recs[i] for i in file_order(lines, ids, sorted_))


# ---- saying where two streams differ ---------------------------------------------------------------------------------------------
_FIXED = (("block_size", 0, 4), ("refID", 4, 4), ("pos", 8, 4), ("l_read_name", 12, 1), ("mapq", 13, 1), ("bin", 14, 2), ("n_cigar_op", 16, 2),
          ("flag", 18, 2), ("l_seq", 20, 4), ("next_refID", 24, 4), ("next_pos", 28, 4), ("tlen", 32, 4))


def record_fields(line: bytes, ref_ids: dict):
    """[(field name, start, end)] over the bytes record_bytes gives for the line: the fixed fields, then read_name, cigar, seq, qual
    and every tag by name"""
    rec = record_bytes(line, ref_ids)
    f = line.split(b"\t")
    out = [(n, a, a + l) for n, a, l in _FIXED]
    p = 36
    n_cig, l_seq = struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<i", rec, 20)[0]
    for name, size in (("read_name", rec[12]), ("cigar", 4 * n_cig), ("seq", (l_seq + 1) // 2), ("qual", l_seq)):
        out.append((name, p, p + size))
        p += size
    for t in f[11:]:
        size = len(_tag(t, []))
        out.append(("tag " + t[:2].decode("latin-1") + " (" + chr(t[3]) + ")", p, p + size))
        p += size
    assert p == len(rec)
    return out


def explain(got: bytes, header_text: bytes, lines, sorted_: bool, ignore=()) -> str:
    """"" when `got` is stream_bytes(...), else the first difference in words: which header part, or which record (its place in the
    file, its input line, its QNAME) and which field.  ignore: byte ranges [(start, end)] of the stream left out of the comparison."""
    want = stream_bytes(header_text, lines, sorted_)
    skip = bytearray(len(want))
    for a, b in ignore:
        skip[a:b] = b"\1" * (b - a)
    n = min(len(got), len(want))
    d = next((i for i in range(n) if got[i] != want[i] and not skip[i]), None)
    if d is None:
        if len(got) == len(want):
            return ""
        d = n
    hb = header_bytes(header_text, sorted_)
    if d < len(hb):
        l_text = struct.unpack_from("<i", hb, 4)[0]
        part = "magic" if d < 4 else "l_text" if d < 8 else "text" if d < 8 + l_text else "n_ref" if d < 12 + l_text else "reference dictionary"
        return f"header: {part} differs at byte {d}: got {got[d:d + 16]!r}, want {want[d:d + 16]!r}"
    ids = ref_ids_of(header_text)
    p = len(hb)
    for k, i in enumerate(file_order(lines, ids, sorted_)):
        rec = record_bytes(lines[i], ids)
        if d < p + len(rec):
            qname = lines[i].partition(b"\t")[0][:40]
            who = f"record {k} of {len(lines)} (input line {i}, QNAME {qname!r}, stream offset {p})"
            for name, a, b in record_fields(lines[i], ids):
                if a <= d - p < b:
                    g, w = got[p + a:p + b], want[p + a:p + b]
                    if b - a <= 4 and len(g) == b - a:
                        g, w = int.from_bytes(g, "little"), int.from_bytes(w, "little")
                        return f"{who}: field {name}: got {g} (0x{g:x}), want {w} (0x{w:x})"
                    return f"{who}: field {name}: byte {d - p - a} of {b - a}: got {got[d:d + 8].hex()}, want {want[d:d + 8].hex()}"
            raise AssertionError("a record's bytes are covered by its fields")
        p += len(rec)
    return f"length: got {len(got)} bytes, want {len(want)}: the streams agree up to the shorter one's end"
