"""TEST INFRASTRUCTURE: the inputs of tests/test_gpu_bam_records.py (GPU) and tests/test_bamdef_host.py (CPU): small, deterministic
SAM texts that put every byte the BAM record writer emits (bam_record / Sink in mkt_bam.hip) at its edges, to be compared byte for
byte with tests/bamdef.py.  Each list says in its docstring which condition on the input it relies on; the host test asserts those
conditions, so that an edit here cannot quietly stop a case from testing what it is named for.

The three functions below the cases restate what the product's reference-name table does (FNV-1a, capacity, home slot): they exist
only to CONSTRUCT names that collide there and to check that they do; nothing compares their output with the product."""
import collections
import random

import bamdef

Case = collections.namedtuple("Case", "name header lines raw masked")
WG = 256                                    # records per workgroup of the record kernels


def case(name, header, lines, raw=None, masked=False):
    return Case(name, header, list(lines), raw, masked)


def sam_text(c) -> bytes:
    return c.raw if c.raw is not None else c.header + b"".join(ln + b"\n" for ln in c.lines)


def line(qname=b"q", flag=0, rname=b"chr1", pos=1, mapq=0, cigar=b"1M", rnext=b"*", pnext=0, tlen=0, seq=b"A", qual=b"I", tags=()):
    f = [qname, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, seq, qual]
    return b"\t".join(f + list(tags))


HDR = b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:chr1\tLN:250000000\n@SQ\tSN:chr2\tLN:250000000\n@PG\tID:x\tPN:x\n"
HDR_WIDE = b"@SQ\tSN:chr1\tLN:2147483647\n@SQ\tSN:chr2\tLN:2147483647\n"          # positions up to 2^31 - 1 (no index is made then)


# ---- sink: every (start offset mod 8, record size mod 8) with a neighbour on both sides ---------------------------------------------
def sink_lines():
    """QNAME length 1..16 against a Z tag of 0..7 characters (CIGAR *, SEQ *: 42 + l_qname + l_tag bytes), in a fixed shuffled order,
    with minimal records (QNAME of one byte, no tag: 38 bytes) mixed in; three workgroups and a partial one.  POS is a permutation,
    so that the sorted file has other neighbours than the input.  CONDITION (asserted on the CPU): all 64 classes occur, in input
    order and in sorted order, on records that have both neighbours."""
    rng = random.Random(64)
    combos = [(l, k) for l in range(1, 17) for k in range(8)]
    shapes = []
    for _ in range(7):
        rng.shuffle(combos)
        shapes += combos
    shapes = shapes[:3 * WG + 37 - 30]
    for i in range(30):
        shapes.insert(rng.randrange(len(shapes)), (1, None))
    pos = list(range(1, len(shapes) + 1))
    rng.shuffle(pos)
    out = []
    for i, (l, k) in enumerate(shapes):
        q = (b"%x" % (i % 16)) + b"ABCDEFGHIJKLMNOP"[:l - 1]
        tags = () if k is None else (b"XZ:Z:" + b"tuvwxyz{"[:k],)
        out.append(line(q, 16 * (i % 2), b"chr1" if i % 5 else b"chr2", pos[i], 7, b"*", b"*", 0, 0, b"*", b"*", tags))
    return out


def alignment_classes(header, lines, sorted_):
    """{(start offset mod 8, size mod 8)} of the records that have a record before and after them, from bamdef's sizes"""
    ids = bamdef.ref_ids_of(header)
    order = bamdef.file_order(lines, ids, sorted_)
    p = len(bamdef.header_bytes(header, sorted_))
    seen = set()
    for k, i in enumerate(order):
        n = len(bamdef.record_bytes(lines[i], ids))
        if 0 < k < len(order) - 1:
            seen.add((p % 8, n % 8))
        p += n
    return seen


# ---- fields -----------------------------------------------------------------------------------------------------------------------
def field_lines():
    """the fixed fields at their limits (the accepted side; REJECTS holds the other)"""
    L = []
    for n in (1, 253, 254):
        L.append(line(b"N" * n))
    for fl in (0, 4, 16, 65535):
        L.append(line(b"flag%d" % fl, fl))
    L.append(line(b"mapq255", mapq=255))
    for p in (0, 1, 1 << 29, (1 << 31) - 1):
        L.append(line(b"pos%d" % p, pos=p))
    L.append(line(b"pnext_max", rnext=b"=", pnext=(1 << 31) - 1))
    L.append(line(b"pnext0", rnext=b"chr2", pnext=0))
    for t in ((1 << 31) - 1, -((1 << 31) - 1), -(1 << 31), 1, -1):
        L.append(line(b"tlen%d" % t, tlen=t))
    L.append(line(b"signs", 0, b"chr1", 5, 0, b"1M", b"*", 0, 0).replace(b"\t5\t", b"\t+5\t").replace(b"\t0\t0\tA", b"\t-0\t+0\tA"))
    L.append(line(b"eq_nowhere", 4, b"*", 0, 0, b"*", b"=", 0, 0))                  # RNEXT = with RNAME *: no mate reference either
    L.append(line(b"eq_chr1", 1, b"chr1", 9, 0, b"1M", b"=", 99, 0))
    L.append(line(b"other", 1, b"chr1", 9, 0, b"1M", b"chr2", 99, 0))
    L.append(line(b"other_unplaced", 1, b"*", 0, 0, b"*", b"chr2", 99, 0))
    L.append(line(b"none", 1, b"chr2", 9, 0, b"1M", b"*", 0, 0))
    L.append(line(b"star_pos", 0, b"*", 77, 0, b"1M"))                             # RNAME * with a position: unmapped, sorts last by POS
    L.append(line(b"nocigar", 0, b"chr1", 77, 0, b"*"))                            # mapped without CIGAR: FLAG gains 4
    L.append(line(b"ops", cigar=b"1M2I3D4N5S6H7P8=9X", seq=b"*", qual=b"*"))
    for c in (b"0M", b"1M", b"268435455M", b"268435455S", b"5S3I", b"0M0D", b"3H"):
        L.append(line(b"cig" + c, cigar=c, seq=b"*", qual=b"*"))
    L.append(line(b"ops65535", cigar=b"1M" * 65535, seq=b"*", qual=b"*"))
    # bin: the six levels of reg2bin, and both sides of a 2^14 boundary
    for k, sh in enumerate((14, 17, 20, 23, 26, 29)):
        L.append(line(b"lvl%d" % k, pos=(1 << sh) - 4, cigar=b"10M", seq=b"*", qual=b"*"))
    L.append(line(b"lvl_leaf", pos=3, cigar=b"10M", seq=b"*", qual=b"*"))
    for p, c in ((16384, b"1M"), (16385, b"1M"), (16375, b"10M"), (16375, b"11M"), (16375, b"5M5N1M"), (16375, b"5M5I5S"), (1, b"16384M"), (1, b"16385M")):
        L.append(line(b"edge%d_%s" % (p, c), pos=p, cigar=c, seq=b"*", qual=b"*"))
    return L


def expected_bins():
    """{QNAME: bin} for the lvl* lines of field_lines, from the level table of SAMv1 5.3 written out (not through a reg2bin)"""
    out = {b"lvl_leaf": 4681}
    first = (4681, 585, 73, 9, 1)
    for k, sh in enumerate((14, 17, 20, 23, 26)):                # the span straddles 2^sh: the smallest bin holding it is one level up
        out[b"lvl%d" % k] = 0 if k == 4 else first[k + 1] + (((1 << sh) - 5) >> (sh + 3))
    out[b"lvl5"] = 0
    return out


REJECTS = []          # (what, header, line): the writer must refuse the line; filled below


def _rej(what, ln, header=HDR_WIDE):
    REJECTS.append((what, header, ln))


_rej("QNAME of 255 bytes", line(b"N" * 255))
_rej("QNAME empty", line(b""))
_rej("FLAG 65536", line(flag=65536))
_rej("FLAG signed", line().replace(b"\t0\tchr1", b"\t+0\tchr1"))
_rej("MAPQ 256", line(mapq=256))
_rej("POS 2^31", line(pos=1 << 31))
_rej("POS -1", line(pos=-1))
_rej("PNEXT 2^31", line(pnext=1 << 31))
_rej("TLEN 2^31", line(tlen=1 << 31))
_rej("TLEN -2^31 - 1", line(tlen=-(1 << 31) - 1))
_rej("CIGAR count 2^28", line(cigar=b"268435456M", seq=b"*", qual=b"*"))
_rej("CIGAR of 65536 operations", line(cigar=b"1M" * 65536, seq=b"*", qual=b"*"))
_rej("CIGAR without count", line(cigar=b"M"))
_rej("CIGAR ending in digits", line(cigar=b"1M2"))
_rej("CIGAR empty", line(cigar=b""))
_rej("CIGAR letter", line(cigar=b"1Q"))
_rej("ten fields", b"\t".join(line().split(b"\t")[:10]))
_rej("SEQ / QUAL lengths", line(seq=b"AC", qual=b"I"))
_rej("QUAL for SEQ *", line(seq=b"*", qual=b"II"))
_rej("POS not a number", line().replace(b"\t1\t0\t1M", b"\tx\t0\t1M"))
_rej("reference not in the header", line(rname=b"chr9"))
_rej("mate reference not in the header", line(rnext=b"chr9"))
for _what, _tag in (("integer tag 2^32", b"XI:i:4294967296"), ("integer tag -2^31 - 1", b"XI:i:-2147483649"), ("integer tag text", b"NM:i:x"),
                    ("integer tag empty", b"NM:i:"), ("integer tag two signs", b"NM:i:+-1"), ("A of two characters", b"XA:A:ab"), ("A empty", b"XA:A:"),
                    ("unknown type", b"XQ:q:1"), ("tag without type", b"XQ1"), ("tag with a long name", b"XQQ:i:1"), ("B unknown subtype", b"XB:B:x,1"),
                    ("B no subtype", b"XB:B:"), ("B subtype without comma", b"XB:B:c1"), ("B empty element", b"XB:B:c,"), ("B empty middle", b"XB:B:c,1,,2"),
                    ("B:c 128", b"XB:B:c,128"), ("B:c -129", b"XB:B:c,-129"), ("B:C 256", b"XB:B:C,256"), ("B:C -1", b"XB:B:C,-1"),
                    ("B:s 32768", b"XB:B:s,32768"), ("B:S 65536", b"XB:B:S,65536"), ("B:i 2^31", b"XB:B:i,2147483648"), ("B:I 2^32", b"XB:B:I,4294967296"),
                    ("B:f text", b"XB:B:f,1,x"), ("float without digits", b"Xf:f:."), ("float empty", b"Xf:f:"), ("float sign only", b"Xf:f:-"),
                    ("float empty exponent", b"Xf:f:1e"), ("float two points", b"Xf:f:1.2.3"), ("float exponent 401", b"Xf:f:1e401"),
                    ("float hexadecimal", b"Xf:f:0x10"), ("float trailing text", b"Xf:f:1.5f")):
    _rej(_what, line(tags=(_tag,)))


# ---- SEQ / QUAL ----------------------------------------------------------------------------------------------------------------
SEQ_BYTES = bytes(c for c in range(1, 256) if c not in (9, 10))            # every byte a line can carry inside a field


def seqqual_lines():
    rng = random.Random(15)
    L = [line(b"len0", seq=b"*", qual=b"*", cigar=b"*"), line(b"len1_noqual", seq=b"G", qual=b"*"), line(b"len1_star_is_absent", seq=b"*", qual=b"*")]
    for n in (1, 2, 3, 255, 256):
        s = bytes(rng.choice(b"=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn.Uu0-") for _ in range(n))
        L.append(line(b"len%d" % n, cigar=b"%dM" % n, seq=s, qual=bytes(33 + (7 * i) % 94 for i in range(n))))
        L.append(line(b"len%d_noqual" % n, cigar=b"%dM" % n, seq=s.swapcase(), qual=b"*"))
    L.append(line(b"allbytes_hi", seq=SEQ_BYTES, qual=b"*"))                 # every byte in the high nibble of its pair ...
    L.append(line(b"allbytes_lo", seq=b"T" + SEQ_BYTES, qual=b"*"))          # ... and in the low one
    L.append(line(b"allbytes_q", seq=SEQ_BYTES[::-1], qual=bytes(33 + i % 94 for i in range(len(SEQ_BYTES)))))
    L.append(line(b"qual_lo", seq=b"ACGTA", qual=b"!!!!!"))
    L.append(line(b"qual_hi", seq=b"ACGTA", qual=b"~~~~~"))
    L.append(line(b"qual_star_then", seq=b"ACGTA", qual=b"*IIII"))           # a QUAL that merely starts with *
    L.append(line(b"qual_high_bytes", seq=b"ACG", qual=b"\x20\x7f\xff"))     # below ! and above ~: the byte minus 33, modulo 256
    return L


# ---- tags ----------------------------------------------------------------------------------------------------------------------
INT_EDGES = [b"0", b"+0", b"-0", b"1", b"+1", b"-1", b"+5", b"127", b"128", b"255", b"256", b"+255", b"+256", b"32767", b"32768", b"65535", b"65536",
             b"+65536", b"2147483647", b"2147483648", b"4294967294", b"4294967295", b"+4294967295", b"-127", b"-128", b"-129", b"-32767", b"-32768",
             b"-32769", b"-2147483647", b"-2147483648", b"007", b"-000128", b"0000000000000065536"]
_B_RANGE = {b"c": (-128, 127), b"C": (0, 255), b"s": (-32768, 32767), b"S": (0, 65535), b"i": (-(1 << 31), (1 << 31) - 1), b"I": (0, (1 << 32) - 1)}


def tag_name(i):
    a = b"XYZxyz"[i // 36 % 6:][:1]
    return a + b"0123456789abcdefghijklmnopqrstuvwxyz"[i % 36:][:1]


def tag_lines():
    rng = random.Random(4)
    L = [line(b"chars", tags=(b"XA:A:q", b"Xa:a:r", b"Xc:c:5", b"XC:C:~", b"XB:A:!", b"Xd:c:-"))]
    L.append(line(b"hex", tags=(b"H0:H:", b"H1:H:1AE301", b"H2:H:1AE30", b"H3:H:g")))
    L.append(line(b"text", tags=(b"Z0:Z:", b"Z1:Z:" + bytes(range(0x20, 0x7F)), b"Z2:Z:a:b:c", b"Z3:Z:\xc3\xa9")))
    for i, v in enumerate(INT_EDGES):
        L.append(line(b"int" + v, tags=(tag_name(i) + (b":I:" if i % 3 == 2 else b":i:") + v,)))
    L.append(line(b"ints", tags=tuple(tag_name(i) + b":i:" + v for i, v in enumerate(INT_EDGES))))
    for sub in (b"c", b"C", b"s", b"S", b"i", b"I", b"f"):
        for n in (0, 1, 300):
            if sub == b"f":
                vals = [b"%d.%d" % (rng.randrange(-999, 999), 25 * rng.randrange(4)) for _ in range(n)]
            else:
                lo, hi = _B_RANGE[sub]
                vals = [b"%d" % (lo if k == 0 else hi if k == 1 else rng.randrange(lo, hi + 1)) for k in range(n)]
                rng.shuffle(vals)
                if n == 1:
                    vals = [b"%d" % (hi if sub in b"csi" else lo)]
            L.append(line(b"B%s%d" % (sub, n), tags=(b"B" + sub + b":B:" + sub + b"".join(b"," + v for v in vals), b"ZZ:Z:after")))
    L.append(line(b"Bsigns", tags=(b"XB:B:c,+5,-0,+0", b"XC:B:I,+4294967295", b"XD:B:i,-2147483648,2147483647")))
    kinds = [b":i:-7", b":A:k", b":Z:str", b":f:0.5", b":H:FF", b":B:S,1,2", b":i:70000", b":Z:"]
    L.append(line(b"forty", tags=tuple(tag_name(i) + kinds[i % len(kinds)] for i in range(40))))
    L.append(line(b"big", tags=(b"XL:Z:" + bytes(33 + (i * 31) % 94 for i in range(70000)), b"XE:i:-129")))     # > 64 KiB: spans BGZF blocks
    return L


# ---- floats --------------------------------------------------------------------------------------------------------------------
def f32_corpus_bits():
    """fixed-seed float32 bit patterns: the extremes, powers of two and their neighbours, random normal and subnormal values"""
    rng = random.Random(32)
    bits = [1, 2, 3, 0x7FFFFF, 0x7FFFFE, 0x800000, 0x800001, 0x7F7FFFFF, 0x7F7FFFFE, 0x3F800000, 0x3F7FFFFF, 0x3F800001]
    for e in (-126, -100, -60, -30, -10, -1, 1, 10, 23, 24, 30, 60, 100, 127):
        p = (e + 127) << 23
        bits += [p - 1, p, p + 1]
    for _ in range(60):
        bits.append(rng.randrange(1, 255) << 23 | rng.getrandbits(23))
    for _ in range(100):                                   # the range where most tag values live
        bits.append(rng.randrange(90, 200) << 23 | rng.getrandbits(23))
    for _ in range(20):
        bits.append(rng.getrandbits(23) or 1)
    return [b | (rng.getrandbits(1) << 31) for b in bits]


def is_domain_a(text):
    """at most 9 significant digits (leading zeros do not count, trailing ones do) scaled by 10^e with |e| <= 22; zero in any spelling"""
    neg, m, e = bamdef.decimal_parts(text)
    return m == 0 or (m < 10 ** 9 and abs(e) <= 22)


def is_domain_c(text):
    """the %.9g print of a finite float32"""
    b = bamdef.float32_exact(text)
    if bamdef.f32_class(b)[1] not in ("finite", "zero"):
        return False
    return ("%.9g" % bamdef.f32_value(b)).encode() == text


# decimals of at most 9 digits, |e| <= 22, whose exact value lies within half a unit of a DOUBLE of a float32 midpoint without being on
# it (found by exhaustive search over 9-digit mantissas): the double nearest to m * 10^e IS the midpoint, so rounding that double to
# float ties to even, whichever side the decimal really lies on.  The first five go the wrong way under that double rounding.
NEAR_MIDPOINT = [b"967498269e-19", b"585052973e13", b"949766107e15", b"804624287e18", b"896981543e20",
                 b"9.67498269e-11", b"0.0000000000967498269", b"5.85052973E+21", b"-9.49766107e23", b"+8.04624287e26", b"89698154.3e21",
                 b"248237791e-20", b"702990899e-20", b"544286477e-18", b"939430711e-17", b"682972221e-16", b"477805429e-14", b"265092267e-13",
                 b"163364931e13", b"721866475e13", b"144373295e14", b"509086429e14", b"28874659e15", b"374751039e16", b"316694311e18"]
DOMAIN_A_FORMS = [b".5", b"5.", b"1E3", b"+1e-3", b"-0", b"0.000", b"0", b"+0", b"-0.0e5", b"0e-400", b"000001", b"1e22", b"1e-22", b"999999999e22",
                  b"999999999e-22", b"123456789e-22", b"0.1", b"0.3", b"1.1", b"3.25", b"-2", b"1e+3", b"1.5e-007",
                  b"16777216", b"16777217", b"16777218", b"16777219", b"33554434", b"33554438", b"-16777217",          # exactly on a midpoint: to even
                  b"1.00000005", b"1.00000006", b"1.00000017", b"1.00000018", b"0.999999970", b"0.999999971",        # either side of one
                  b"8388608.5", b"8388609.5", b"4194304.25", b"4194304.75"]
DOMAIN_B = [b"0.1000000000000000055511151231257827", b"3.14159265358979323846", b"1.2345678901234567", b"123456789012345678e-30", b"1234567890123456789",
            b"12345678901234567890123456789", b"1234567890", b"16777217.0000000001", b"16777216.9999999999", b"0.33333333333333333333333",
            b"1e-45", b"7e-46", b"8e-46", b"1e-46", b"1e-39", b"-1e-39", b"5.87747e-39", b"1e23", b"1e-23", b"1e38", b"-1e38", b"3.4028236e38", b"1e39", b"-1e39",
            b"3.5e38", b"1e45", b"1e400", b"-1e400", b"1e-400", b"-1e-400", b"9.87654321e-30", b"1.17549421e-38", b"100000000000000000000000000000e-7",
            b"0.00000000000000000000000000000000001234567891"]


def float_corpus():
    """[(decimal text, domain)]: A (<= 9 digits, |e| <= 22: must be exact), C (%.9g print of a finite float32 outside A: exact by
    derivation), B (everything else: within one ulp, same class).  CONDITIONS (asserted on the CPU): every label agrees with
    is_domain_a / is_domain_c, and B holds fewer than 20 % of the corpus."""
    out, seen = [], set()

    def add(t, want=None):
        if t in seen:
            return
        seen.add(t)
        d = "A" if is_domain_a(t) else "C" if is_domain_c(t) else "B"
        assert want is None or want == d, (t, want, d)
        out.append((t, d))
    for t in DOMAIN_A_FORMS + NEAR_MIDPOINT:
        add(t, "A")
    nb = 0
    for b in f32_corpus_bits():
        v = bamdef.f32_value(b)
        add(("%.9g" % v).encode())
        g = ("%g" % v).encode()
        if is_domain_a(g):
            add(g, "A")
        elif nb < 12:                                      # (a 6-digit print beyond 10^+-22 is neither A nor C: a few of them)
            nb += 1
            add(g)
    for t in DOMAIN_B:                                     # (labelled like the rest: 1e-23 happens to be a float's %.9g print, so C)
        add(t)
    return out


def float_lines(domains):
    """the corpus values of the given domains, eight to a line: the first as an f tag, the rest as the elements of a B:f array"""
    vals = [t for t, d in float_corpus() if d in domains]
    L = []
    for k in range(0, len(vals), 8):
        v = vals[k:k + 8]
        tags = [b"Xf:f:" + v[0]]
        if len(v) > 1:
            tags.append(b"XF:B:f" + b"".join(b"," + x for x in v[1:]))
        L.append(line(b"fl%s%03d" % (domains.encode(), k // 8), tags=tuple(tags)))
    return L


# ---- reference names -------------------------------------------------------------------------------------------------------------
def fnv1a(name: bytes):
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h or 1


def table_capacity(nref):
    cap = 64
    while cap < 4 * nref + 4:
        cap <<= 1
    return cap


def home_slot(name, cap):
    return (fnv1a(name) >> 20) & (cap - 1)


def table_slots(names):
    """{name: (home slot, slot it ends up in)} when the names are entered in order with linear probing"""
    cap = table_capacity(len(names))
    used, out = set(), {}
    for n in names:
        k = home = home_slot(n, cap)
        while k in used:
            k = (k + 1) & (cap - 1)
        used.add(k)
        out[n] = (home, k)
    return out


def _names_at(slot, cap, prefix, count, avoid=()):
    out, i = [], 0
    while len(out) < count:
        n = b"%s%d" % (prefix, i)
        if home_slot(n, cap) == slot and n not in avoid:
            out.append(n)
        i += 1
    return out


def ref_case(nref):
    """-> (header, lines, present names, {kind: absent name}).  Names: four that share the LAST home slot of the table (their chain
    wraps to slots 0, 1, 2), three that share a slot in the middle, a family of prefixes and extensions, plain ones for the rest.
    Absent names: (a) two whose home slot lies in an occupied chain (the wrapping one: at its head and past the table's end),
    (b) a proper prefix of a present name, (c) an extension of one.  Every present name occurs as RNAME and as RNEXT.
    CONDITIONS (asserted on the CPU): the capacity steps as 4 * nref + 4 says, the chains collide and wrap, the absent names'
    home slots are occupied."""
    cap = table_capacity(nref)
    wrap = _names_at(cap - 1, cap, b"w", 4)
    mid = _names_at(cap // 2, cap, b"m", 3)
    family = [b"scaf_12", b"scaf_123", b"scaf_", b"scaf_12|x", b"SCAF_12"]
    names = wrap + mid + family
    i = 0
    while len(names) < nref:
        n = b"contig%04d" % i
        i += 1
        if home_slot(n, cap) not in (cap - 1, 0, 1, 2, 3):       # (the wrapped chain stays as constructed)
            names.append(n)
    names = names[:nref]
    absent = {
        "a: home slot at the head of the wrapping chain": _names_at(cap - 1, cap, b"absent", 1)[0],
        "a: home slot inside the wrapped part": _names_at(1, cap, b"absent", 1)[0],
        "a: home slot in the middle chain": _names_at(cap // 2, cap, b"absent", 1)[0],
        "b: prefix of a present name": b"scaf_1",
        "b: prefix of a present name (one byte short)": names[-1][:-1],
        "c: extension of a present name": b"scaf_1234",
        "c: extension of a present name (one byte more)": names[-1] + b"0",
    }
    header = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, 100000 + k) for k, n in enumerate(names))
    lines = [line(b"r%d" % k, 16 * (k % 2), n, 1 + (k * 7919) % 90000, 3, b"2M", names[(7 * k + 3) % nref], 1 + k, k - 5, b"AC", b"IJ") for k, n in enumerate(names)]
    return header, lines, names, absent


REF_SIZES = (15, 16, 17, 2000)


# ---- line ends --------------------------------------------------------------------------------------------------------------------
def line_end_case():
    """\\r\\n line ends and no newline after the last line: the \\r belongs to no field, whatever the last field is (QUAL, a Z tag, a
    float, an array)"""
    L = [line(b"crlf_qual", seq=b"ACG", qual=b"IJK"), line(b"crlf_z", tags=(b"XZ:Z:text",)), line(b"crlf_f", tags=(b"Xf:f:2.5",)),
         line(b"crlf_B", tags=(b"XB:B:s,1,-2",)), line(b"crlf_i", tags=(b"Xi:i:-129",)), line(b"crlf_star", seq=b"*", qual=b"*"), line(b"last", tags=(b"XZ:Z:",))]
    return case("line ends", HDR, L, raw=HDR + b"\r\n".join(L))


# ---- the lists ----------------------------------------------------------------------------------------------------------------------
def all_cases():
    out = [case("sink", HDR, sink_lines()), case("fields", HDR_WIDE, field_lines()), case("seq and qual", HDR, seqqual_lines()),
           case("tags", HDR, tag_lines()), case("floats A and C", HDR, float_lines("AC")), case("floats B", HDR, float_lines("B"), masked=True)]
    for n in REF_SIZES:
        h, lines, _, _ = ref_case(n)
        out.append(case("refs %d" % n, h, lines))
    out.append(line_end_case())
    out.append(case("no header line", b"@SQ\tSN:chr1\tLN:1000\n", [line()]))
    out.append(case("header without SO", b"@HD\tVN:1.5\n@SQ\tSN:chr1\tLN:1000\n", [line()]))
    return out


def float_word_ranges(c, sorted_):
    """[(start, end, decimal text)] in stream_bytes(...) of the float words of a case's records"""
    ids = bamdef.ref_ids_of(c.header)
    p = len(bamdef.header_bytes(c.header, sorted_))
    out = []
    for i in bamdef.file_order(c.lines, ids, sorted_):
        rec, floats = bamdef.record_layout(c.lines[i], ids)
        out += [(p + o, p + o + 4, txt) for o, txt in floats]
        p += len(rec)
    return out
