"""The definition of `final.pairs.gz` + `final.pairs.gz.px2` (pairix 0.3.7, preset `pairs`) in plain Python.

Everything here was read off what the reference's `bgzip` and `pairix` binaries write (tests/golden/px2_golden.json records it,
tests/make_px2_golden.py made it); include/mkt.h states the same definition in words.  Three parts:

  * BGZF: the block table of a .gz (`bgzf_blocks`), its inflation with every CRC-32 and ISIZE checked, a writer on top of zlib, and
    the two maps between a virtual offset (coffset << 16 | offset in block) and an offset in the uncompressed text.
  * The index: `parse_px2` accounts for every byte of a .px2, `build_index` makes the index of (text, block table), `serialize`
    writes it with the bins of a name in ascending order.
  * `query` answers a region `chrA:b-e|chrB:b-e` from the two files the way `pairix file.gz REGION` prints it.

Comparisons between indexes of differently compressed files go through `to_text_offsets`, which replaces every virtual offset by
the offset in the text it points to and the bins of a name by a sorted list (their order in pairix's file is a hash walk).
"""
import bisect
import functools
import struct
import zlib

MAGIC = b"PX2.004\x01"
LIDX_SHIFT = 15                       # the finest bin and the linear window are 2^15 = 32768 positions wide
BIN_FIRST = 4681                      # first bin of the finest level: ((1 << 15) - 1) / 7
LEVEL_FIRST = (0, 1, 9, 73, 585, 4681)
POS_MAX = 0x7FFFFFFF                  # pairix keeps positions in an int32; this project refuses larger ones
QUERY_END_MAX = 1 << 30               # pairix's reader clips the first range of a region here: records behind it are indexed but never answered
BGZF_RAW = 0xFF00
BGZF_EOF = bytes([0x1F, 0x8B, 0x08, 0x04, 0, 0, 0, 0, 0, 0xFF, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1B, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])
# preset `pairs`: (preset word, sc, bc, ec, sc2, bc2, ec2) in 1-based columns, then delimiter, region separator, meta char, skip
CONF_PAIRS = (3, 2, 3, 3, 4, 5, 5)
DELIM, REGION_SEP, META, SKIP = 9, ord("|"), ord("#"), 0


class Px2Error(ValueError):
    """An input this project refuses; `line` is 1-based and counts every line of the text."""

    def __init__(self, line, what):
        ValueError.__init__(self, "line %d: %s" % (line, what))
        self.line = line
        self.what = what


# ---- BGZF ------------------------------------------------------------------------------------------------------------------------
def bgzf_blocks(gz, check=True):
    """[(coffset, BSIZE + 1, offset of its first byte in the text, ISIZE)] of every block; with `check`, every block is inflated and
    its CRC-32 and ISIZE compared."""
    out = []
    p = u = 0
    while p < len(gz):
        if gz[p:p + 4] != b"\x1f\x8b\x08\x04" or len(gz) - p < 18:
            raise ValueError("no BGZF block at %d" % p)
        xlen, = struct.unpack_from("<H", gz, p + 10)
        if xlen != 6 or gz[p + 12:p + 16] != b"BC\x02\x00":
            raise ValueError("block at %d: not the one BC subfield" % p)
        bsize = struct.unpack_from("<H", gz, p + 16)[0] + 1
        if p + bsize > len(gz):
            raise ValueError("block at %d runs past the file" % p)
        crc, isize = struct.unpack_from("<II", gz, p + bsize - 8)
        if check:
            data = zlib.decompress(gz[p + 18:p + bsize - 8], -15)
            if len(data) != isize or zlib.crc32(data) != crc:
                raise ValueError("block at %d: ISIZE or CRC-32 is wrong" % p)
        out.append((p, bsize, u, isize))
        u += isize
        p += bsize
    return tuple(out)


@functools.lru_cache(maxsize=8)
def _columns(blocks):
    return [b[2] for b in blocks], [b[0] for b in blocks]


def bgzf_inflate(gz):
    return b"".join(zlib.decompress(gz[c + 18:c + b - 8], -15) for c, b, _, _ in bgzf_blocks(gz, check=False))


def bgzf_compress(data, level=6, cuts=None):
    """BGZF of `data`; `cuts`: ascending text offsets at which a new block begins (default: every BGZF_RAW bytes)."""
    if cuts is None:
        cuts = list(range(BGZF_RAW, len(data), BGZF_RAW))
    edges = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    out = []
    for a, b in zip(edges, edges[1:]):
        if a == b:
            continue
        assert b - a <= BGZF_RAW
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(data[a:b]) + co.flush()
        if len(body) + 26 > 0x10000:
            co = zlib.compressobj(0, zlib.DEFLATED, -15)
            body = co.compress(data[a:b]) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(data[a:b]), b - a))
    out.append(BGZF_EOF)
    return b"".join(out)


def voff_of(blocks, u, gz_len):
    """Where a reader stands that has consumed text[0, u): in the block that holds byte u; when a block ends at u, at offset 0 of
    the block behind it (the EOF block at the end of the text); behind the file if there is none."""
    starts = _columns(blocks)[0]
    k = bisect.bisect_left(starts, u)                     # the first block that starts at u, if one does
    if k < len(blocks) and starts[k] == u:
        return blocks[k][0] << 16
    k -= 1
    if k < 0 or u >= blocks[k][2] + blocks[k][3]:
        if k >= 0 and u == blocks[k][2] + blocks[k][3]:
            return gz_len << 16
        raise ValueError("text offset %d lies outside the file" % u)
    return blocks[k][0] << 16 | (u - blocks[k][2])


def text_offset_of(blocks, v, gz_len):
    c, o = v >> 16, v & 0xFFFF
    if c == gz_len and o == 0:
        return blocks[-1][2] + blocks[-1][3] if blocks else 0
    coffs = _columns(blocks)[1]
    k = bisect.bisect_left(coffs, c)
    if k == len(blocks) or coffs[k] != c or o > blocks[k][3]:
        raise ValueError("virtual offset %#x points at no block" % v)
    return blocks[k][2] + o


# ---- the index ---------------------------------------------------------------------------------------------------------------------
def pos_bin(pos1):
    """The bin and the linear window of a record: pairix indexes the one base [pos1 - 1, pos1), which always fits the finest level."""
    w = (pos1 - 1 if pos1 > 0 else 0) >> LIDX_SHIFT
    return BIN_FIRST + w, w


def bin_range(b):
    """[beg, end) in 0-based positions that bin b covers.  Bins past the six-level scheme (positions from 2^30 on) continue the finest level."""
    for lv in range(5, -1, -1):
        if b >= LEVEL_FIRST[lv]:
            sh = LIDX_SHIFT + 3 * (5 - lv)
            return (b - LEVEL_FIRST[lv]) << sh, (b - LEVEL_FIRST[lv] + 1) << sh
    raise ValueError(b)


def split_lines(text):
    """[(start, end without the newline)] of every line; a last line without a newline is a line."""
    out = []
    p = 0
    while p < len(text):
        q = text.find(b"\n", p)
        if q < 0:
            q = len(text)
        out.append((p, q))
        p = q + 1
    return out


def parse_record(text, a, b, line):
    """(chr1, pos1, chr2) of the record text[a, b); refuses fewer than five columns and a pos1 that is not a decimal number <= POS_MAX."""
    cols = text[a:b].split(b"\t", 5)
    if len(cols) < 5:
        raise Px2Error(line, "fewer than five columns")
    p = cols[2]
    if not p or not p.isdigit() or len(p) > 10 or int(p) > POS_MAX:
        raise Px2Error(line, "pos1 is not a decimal number below 2^31")
    return cols[1], int(p), cols[3]


def build_index(text, blocks, gz_len):
    """The index of `text` compressed into `blocks`: {"n_lines", "names": [bytes], "bins": [{bin: [(beg, end)]}], "linear": [[voff]]}.
    Lines that begin with '#' are counted and belong to the chunk in front of them.  A chunk runs from the start of its first
    record to the start of the first record of the next chunk (the end of the text for the last one)."""
    lines = split_lines(text)
    names, bins, linear = [], [], []
    seen = {}
    prev = None                                           # (name id, pos1, bin) of the record before
    open_chunk = None                                     # (name id, bin, beg voff)
    for j, (a, b) in enumerate(lines):
        if b > a and text[a] == META:
            continue
        c1, pos, c2 = parse_record(text, a, b, j + 1)
        name = c1 + b"|" + c2
        if prev is None or names[prev[0]] != name:
            if name in seen:
                raise Px2Error(j + 1, "the pair %s reappears: its lines are not contiguous" % name.decode("latin-1"))
            seen[name] = tid = len(names)
            names.append(name)
            bins.append({})
            linear.append([])
        else:
            tid = prev[0]
            if pos < prev[1]:
                raise Px2Error(j + 1, "pos1 goes backwards inside the pair %s" % name.decode("latin-1"))
        bn, w = pos_bin(pos)
        if prev is None or tid != prev[0] or bn != prev[2]:
            v = voff_of(blocks, a, gz_len)
            if open_chunk:
                bins[open_chunk[0]].setdefault(open_chunk[1], []).append((open_chunk[2], v))
            open_chunk = (tid, bn, v)
            lin = linear[tid]
            fill = lin[-1] if lin else 0                  # empty windows repeat the one before; those before the first record stay 0
            lin.extend([fill] * (w - len(lin)))
            lin.append(v)
        prev = (tid, pos, bn)
    if open_chunk:
        bins[open_chunk[0]].setdefault(open_chunk[1], []).append((open_chunk[2], voff_of(blocks, len(text), gz_len)))
    return {"n_lines": len(lines), "names": names, "bins": bins, "linear": linear}


def serialize(ix):
    """The uncompressed bytes of a .px2, bins ascending."""
    nm = b"".join(n + b"\0" for n in ix["names"])
    out = [MAGIC, struct.pack("<iQ7i", len(ix["names"]), ix["n_lines"], *CONF_PAIRS), bytes([DELIM, REGION_SEP, 0, 0]), struct.pack("<3i", META, SKIP, len(nm)), nm]
    for bins, lin in zip(ix["bins"], ix["linear"]):
        out.append(struct.pack("<i", len(bins)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])))
            for beg, end in bins[b]:
                out.append(struct.pack("<QQ", beg, end))
        out.append(struct.pack("<i%dQ" % len(lin), len(lin), *lin))
    return b"".join(out)


def parse_px2_raw(d):
    """The fields of the uncompressed bytes of a .px2; raises unless every byte is accounted for."""
    if d[:8] != MAGIC:
        raise ValueError("magic %r" % d[:8])
    p = 8
    n_ref, n_lines = struct.unpack_from("<iQ", d, p); p += 12
    conf = struct.unpack_from("<7i", d, p); p += 28
    delim, sep, z0, z1 = d[p:p + 4]; p += 4
    meta, skip, l_nm = struct.unpack_from("<3i", d, p); p += 12
    blob = d[p:p + l_nm]; p += l_nm
    if len(blob) != l_nm or (l_nm and blob[-1] != 0) or z0 or z1:
        raise ValueError("name table")
    names = blob.split(b"\0")[:-1]
    if len(names) != n_ref:
        raise ValueError("%d names for n_ref %d" % (len(names), n_ref))
    bins, linear, order = [], [], []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, p); p += 4
        bb, oo = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, p); p += 8
            if b in bb:
                raise ValueError("bin %d twice" % b)
            bb[b] = [struct.unpack_from("<QQ", d, p + 16 * k) for k in range(n_chunk)]; p += 16 * n_chunk
            oo.append(b)
        n_intv, = struct.unpack_from("<i", d, p); p += 4
        linear.append(list(struct.unpack_from("<%dQ" % n_intv, d, p))); p += 8 * n_intv
        bins.append(bb)
        order.append(oo)
    if p != len(d):
        raise ValueError("%d bytes behind the last linear index" % (len(d) - p))
    return {"n_lines": n_lines, "conf": list(conf), "delim": delim, "sep": sep, "meta": meta, "skip": skip, "names": names, "bins": bins, "linear": linear, "bin_order": order}


def parse_px2(px2):
    """... of a .px2 file, which is BGZF and ends with the EOF block."""
    bgzf_blocks(px2)
    if px2[-28:] != BGZF_EOF:
        raise ValueError("no EOF block")
    return parse_px2_raw(bgzf_inflate(px2))


def _runs(values):
    """[[value, repeats], ...]: a linear index is mostly repeats (65536 entries for a pos1 near 2^31)"""
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return out


def to_text_offsets(ix, blocks, gz_len):
    """The comparable form: JSON-ready, every virtual offset as an offset in the text (a 0 in a linear index that stands for "no record yet" stays
    None), bins as a sorted list, a linear index as runs [[offset, repeats], ...]."""
    t = lambda v: text_offset_of(blocks, v, gz_len)
    out = {"n_lines": ix["n_lines"], "names": [n.decode("latin-1") for n in ix["names"]], "bins": [], "linear": []}
    for k in ("conf", "delim", "sep", "meta", "skip"):
        out[k] = ix.get(k, {"conf": list(CONF_PAIRS), "delim": DELIM, "sep": REGION_SEP, "meta": META, "skip": SKIP}[k])
    for bins, lin in zip(ix["bins"], ix["linear"]):
        out["bins"].append([[b, [[t(x), t(y)] for x, y in bins[b]]] for b in sorted(bins)])
        first = min((x for b in bins for x, _ in bins[b]), default=0)
        lead = 0
        while lead < len(lin) and lin[lead] == 0 and first != 0:
            lead += 1
        out["linear"].append(_runs([None] * lead + [t(v) for v in lin[lead:]]))
    return out


# ---- queries -------------------------------------------------------------------------------------------------------------------------
def parse_region(region):
    """'chrA:b-e|chrB:b-e' (1-based, inclusive; either range may be missing) -> (name, (beg1, end1), (beg2, end2)) 0-based half-open."""
    sides = region.split("|")
    if len(sides) != 2:
        raise ValueError(region)
    out = []
    for s in sides:
        if ":" in s:
            c, r = s.rsplit(":", 1)
            b, e = r.split("-")
            out.append((c, int(b.replace(",", "")) - 1, int(e.replace(",", ""))))
        else:
            out.append((s, 0, 1 << 31))
    return (out[0][0] + "|" + out[1][0]).encode(), (out[0][1], out[0][2]), (out[1][1], out[1][2])


def query(gz, px2, region):
    """The lines `pairix gz region` prints: the records of the pair whose bases [pos - 1, pos) (a position 0 counts as 1) overlap the
    two ranges, found through the bins and the linear index alone."""
    ix = parse_px2(px2)
    name, (b1, e1), (b2, e2) = parse_region(region)
    if name not in ix["names"]:
        return []
    tid = ix["names"].index(name)
    e1 = min(e1, QUERY_END_MAX)
    if b1 >= e1:
        return []
    blocks = bgzf_blocks(gz, check=False)
    text = bgzf_inflate(gz)
    lin = ix["linear"][tid]
    w = b1 >> LIDX_SHIFT
    min_off = lin[min(w, len(lin) - 1)] if lin else 0
    spans = []
    for b, chunks in ix["bins"][tid].items():
        lo, hi = bin_range(b)
        if lo < e1 and b1 < hi:
            spans += [(x, y) for x, y in chunks if y > min_off]
    out = []
    for x, y in sorted(spans):
        a, z = text_offset_of(blocks, x, len(gz)), text_offset_of(blocks, y, len(gz))
        for s, e in split_lines(text[a:z]):
            ln = text[a + s:a + e]
            if not ln or ln[0] == META:
                continue
            cols = ln.split(b"\t")
            if cols[1] + b"|" + cols[3] != name:
                continue
            p1, p2 = int(cols[2]), int(cols[4])
            if max(p1 - 1, 0) < e1 and b1 < max(p1, 1) and max(p2 - 1, 0) < e2 and b2 < max(p2, 1):
                out.append(ln.decode("latin-1"))
    return out


def count_lines(px2):
    """`pairix -n`."""
    return parse_px2(px2)["n_lines"]
