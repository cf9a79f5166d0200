"""The .hic container of include/mkt.h (mkt_matrix_hic), restated in pure Python: struct and zlib only.

build()  the file bytes from the chromosome table, the bin sizes, the cells of every resolution and the weights, by the definition
parse()  a file back into its parts; every position, size and nBytes is checked, and so is that the header, the matrix records with
         their blocks, the footer and the vectors cover the file exactly once, in that order, with nothing in between or behind them

The definition is the project's own, modelled on hic format version 8; no other reader or writer of .hic files is involved.
"""
import math
import struct
import zlib

SOFTWARE = b"microcket-mi355x"
PIECE = 65280
QNAN = struct.pack("<Q", 0x7FF8000000000000)


def _s(b):
    return bytes(b) + b"\0"


def offsets(lengths, r):
    """first bin of every chromosome and the number of bins at bin size r"""
    off, nb = [], 0
    for L in lengths:
        off.append(nb)
        nb += (L + r - 1) // r
    return off, nb


def block_payload(recs, x_off, y_off):
    """recs: [(x, y, count)] of one block, any order -> its payload"""
    recs = sorted(recs, key=lambda t: (t[1], t[0]))
    short = all(c <= 32767 for _, _, c in recs)
    rows = {}
    for x, y, c in recs:
        rows.setdefault(y, []).append((x, c))
    out = [struct.pack("<iiiBBh", len(recs), x_off, y_off, 1 if short else 0, 1, len(rows))]
    for y in sorted(rows):
        out.append(struct.pack("<hh", y - y_off, len(rows[y])))
        for x, c in rows[y]:
            out.append(struct.pack("<hh", x - x_off, c) if short else struct.pack("<hf", x - x_off, c))
    return b"".join(out)


def build(chromsizes, resolutions, cells_per_res, weights=None, opts=None, compress=zlib.compress):
    """chromsizes: [(name bytes, length)]; resolutions: bin sizes in the object's order; cells_per_res: per resolution an iterable of
    (bin1, bin2, count) with genome-wide bin ids; weights: per resolution None or the nbins float weights; opts: block_bins, norm,
    genome_id, norm_label; compress: payload -> zlib stream.  Returns the file."""
    opts = dict(opts or {})
    bb = opts.get("block_bins", 1000)
    genome, label = opts.get("genome_id", b"") or b"", opts.get("norm_label", b"ICE") or b"ICE"
    norm = opts.get("norm", True)
    assert 1 <= bb <= 32767
    names = [n for n, _ in chromsizes]
    lens = [L for _, L in chromsizes]
    nres = len(resolutions)
    zoom = sorted(range(nres), key=lambda k: -resolutions[k])
    assert len(set(resolutions)) == nres
    weights = weights or [None] * nres

    head = [b"HIC\0", struct.pack("<iq", 8, 0), _s(genome), struct.pack("<i", 1), _s(b"software"), _s(SOFTWARE), struct.pack("<i", len(names))]
    for n, L in chromsizes:
        head.append(_s(n) + struct.pack("<i", L))
    head.append(struct.pack("<i", nres) + b"".join(struct.pack("<i", resolutions[k]) for k in zoom) + struct.pack("<i", 0))
    head = b"".join(head)

    # pair -> zoom index -> block number -> records
    pairs = {}
    for z, k in enumerate(zoom):
        r = resolutions[k]
        off, nb = offsets(lens, r)
        ends = off[1:] + [nb]

        def chrom(b):
            lo, hi = 0, len(off) - 1
            while lo < hi:                                   # the last chromosome with bins that starts at or before b
                mid = (lo + hi + 1) // 2
                if off[mid] <= b:
                    lo = mid
                else:
                    hi = mid - 1
            while ends[lo] <= b or ends[lo] == off[lo]:      # (a chromosome without bins shares its first bin with the next one)
                lo += 1
            return lo
        for b1, b2, c in cells_per_res[k]:
            b1, b2, c = int(b1), int(b2), int(c)
            c1, c2 = chrom(b1), chrom(b2)
            x, y = b1 - off[c1], b2 - off[c2]
            bcc = max(lens[c1], lens[c2]) // r // bb + 1
            bn = (y // bb) * bcc + x // bb
            pairs.setdefault((c1, c2), [dict() for _ in range(nres)])[z].setdefault(bn, []).append((x, y, c))

    body, entries, pos = [], [], len(head)
    for (c1, c2) in sorted(pairs):
        per = pairs[(c1, c2)]
        streams = []
        for z, k in enumerate(zoom):
            r = resolutions[k]
            bcc = max(lens[c1], lens[c2]) // r // bb + 1
            streams.append([(bn, compress(block_payload(per[z][bn], (bn % bcc) * bb, (bn // bcc) * bb))) for bn in sorted(per[z])])
        at = pos + 12 + 39 * nres + 16 * sum(len(s) for s in streams)
        rec = [struct.pack("<iii", c1, c2, nres)]
        for z, k in enumerate(zoom):
            r = resolutions[k]
            total = sum(c for v in per[z].values() for _, _, c in v)
            assert total < 1 << 53
            rec.append(_s(b"BP") + struct.pack("<iffffiiii", z, float(total), 0.0, 0.0, 0.0, r, bb, max(lens[c1], lens[c2]) // r // bb + 1, len(streams[z])))
            for bn, st in streams[z]:
                rec.append(struct.pack("<iqi", bn, at, len(st)))
                at += len(st)
        rec = b"".join(rec) + b"".join(st for s in streams for _, st in s)
        assert len(rec) == at - pos
        entries.append(_s(b"%d_%d" % (c1, c2)) + struct.pack("<qi", pos, len(rec)))
        body.append(rec)
        pos = at
    footer_pos = pos
    foot = struct.pack("<i", len(entries)) + b"".join(entries) + struct.pack("<ii", 0, 0)
    vecs = []
    if norm:
        for z, k in enumerate(zoom):
            if weights[k] is None:
                continue
            r = resolutions[k]
            off, nb = offsets(lens, r)
            assert len(weights[k]) == nb
            for c in range(len(names)):
                hi = off[c + 1] if c + 1 < len(names) else nb
                vals = b"".join(QNAN if math.isnan(w) else struct.pack("<d", (1.0 / w) if w != 0.0 else math.copysign(math.inf, w)) for w in map(float, weights[k][off[c]:hi]))
                vecs.append((c, r, struct.pack("<i", hi - off[c]) + vals))
    index_len = len(vecs) * (len(label) + 1 + 4 + 3 + 4 + 8 + 4)
    foot += struct.pack("<i", len(vecs))
    vpos = footer_pos + 4 + len(foot) + index_len
    for c, r, data in vecs:
        foot += _s(label) + struct.pack("<i", c) + _s(b"BP") + struct.pack("<iqi", r, vpos, len(data))
        vpos += len(data)
    out = head + b"".join(body) + struct.pack("<i", len(foot)) + foot + b"".join(d for _, _, d in vecs)
    return out[:8] + struct.pack("<q", footer_pos) + out[16:]


class _R:
    def __init__(self, b, pos=0):
        self.b, self.pos = b, pos

    def take(self, fmt):
        n = struct.calcsize(fmt)
        assert self.pos + n <= len(self.b), "the file ends inside a field"
        v = struct.unpack_from(fmt, self.b, self.pos)
        self.pos += n
        return v if len(v) > 1 else v[0]

    def string(self):
        e = self.b.index(b"\0", self.pos)
        v = self.b[self.pos:e]
        self.pos = e + 1
        return v


def decode_payload(p):
    """payload -> (header dict, [(x, y, count)] in file order); the payload must end with its last record"""
    r = _R(p)
    n, x_off, y_off, short, mtype, rows = r.take("<iiiBBh")
    assert mtype == 1 and short in (0, 1)
    recs = []
    last_y = -1
    for _ in range(rows):
        dy, k = r.take("<hh")
        assert dy > last_y and k >= 1, "rows ascend and are not empty"
        last_y, last_x = dy, -1
        for _ in range(k):
            dx, c = r.take("<hh" if short else "<hf")
            assert dx > last_x, "records of a row ascend"
            last_x = dx
            if not short:
                assert c == int(c)
            recs.append((x_off + dx, y_off + dy, int(c)))
    assert len(recs) == n and r.pos == len(p), "record count and payload length agree"
    if recs:
        assert short == (1 if max(c for _, _, c in recs) <= 32767 else 0)
    return dict(nRecords=n, xOff=x_off, yOff=y_off, useShort=short, matrixType=mtype, rowCount=rows), recs


def parse(b, inflate=zlib.decompress):
    """-> dict(header, matrices, footer, vectors).  matrices: per record c1, c2 and per resolution its fields and blocks (number,
    position, size, stream, payload, head, records as (x, y, count))."""
    r = _R(b)
    assert r.take("<4s") == b"HIC\0"
    version, footer_pos = r.take("<iq")
    assert version == 8
    genome = r.string()
    attrs = {}
    for _ in range(r.take("<i")):
        k = r.string()
        attrs[k] = r.string()
    chroms = []
    for _ in range(r.take("<i")):
        n = r.string()
        chroms.append((n, r.take("<i")))
    res = [r.take("<i") for _ in range(r.take("<i"))]
    assert res == sorted(res, reverse=True) and len(set(res)) == len(res)
    assert r.take("<i") == 0
    header = dict(genome=genome, attrs=attrs, chroms=chroms, resolutions=res, bytes=b[:r.pos])
    lens = [L for _, L in chroms]

    f = _R(b, footer_pos)
    nbytes = f.take("<i")
    foot_start = f.pos
    entries = []
    for _ in range(f.take("<i")):
        k = f.string()
        entries.append((k,) + f.take("<qi"))
    assert f.take("<i") == 0 and f.take("<i") == 0
    index = []
    for _ in range(f.take("<i")):
        t = f.string()
        c = f.take("<i")
        unit = f.string()
        index.append((t, c, unit) + f.take("<iqi"))
    assert f.pos - foot_start == nbytes, "nBytes is the footer behind it, up to the end of the vector index"
    vectors, vp = [], f.pos
    for t, c, unit, bs, pos, nb in index:
        assert unit == b"BP" and pos == vp, "vectors follow the index in its order"
        n = struct.unpack_from("<i", b, pos)[0]
        assert nb == 4 + 8 * n and n == (lens[c] + bs - 1) // bs
        vectors.append(dict(type=t, chr=c, bin_size=bs, raw=b[pos + 4:pos + nb], values=list(struct.unpack_from("<%dd" % n, b, pos + 4))))
        vp += nb
    assert vp == len(b), "the file ends with the last vector"

    matrices, pos = [], r.pos
    for key, mpos, msize in entries:
        assert mpos == pos, "matrix records follow each other from the end of the header"
        m = _R(b, mpos)
        c1, c2, nres = m.take("<iii")
        assert key == b"%d_%d" % (c1, c2) and c1 <= c2 and nres == len(res)
        zs = []
        for z in range(nres):
            assert m.string() == b"BP"
            zi, total, f1, f2, f3, bs, bb, bcc, nblk = m.take("<iffffiiii")
            assert zi == z and bs == res[z] and (f1, f2, f3) == (0.0, 0.0, 0.0)
            assert bcc == max(lens[c1], lens[c2]) // bs // bb + 1
            zs.append(dict(zoom=zi, sum=total, bin_size=bs, bb=bb, bcc=bcc, blocks=[(m.take("<iqi")) for _ in range(nblk)]))
        at = m.pos
        record = b[mpos:at]
        for z in zs:
            blocks, last = [], -1
            for bn, bpos, bsize in z["blocks"]:
                assert bn > last and bpos == at, "blocks ascend and follow each other from the end of the record"
                last = bn
                stream = b[bpos:bpos + bsize]
                payload = inflate(stream)
                head, recs = decode_payload(payload)
                assert recs and head["xOff"] == (bn % z["bcc"]) * z["bb"] and head["yOff"] == (bn // z["bcc"]) * z["bb"]
                for x, y, c in recs:
                    assert x // z["bb"] == bn % z["bcc"] and y // z["bb"] == bn // z["bcc"] and c >= 1
                    assert c1 != c2 or x <= y
                blocks.append(dict(number=bn, position=bpos, size=bsize, stream=stream, payload=payload, head=head, records=recs))
                at += bsize
            z["blocks"] = blocks
        assert at - mpos == msize, "the size of a master index entry is the record plus its blocks"
        assert any(z["blocks"] for z in zs), "a pair without cells has no record"
        matrices.append(dict(c1=c1, c2=c2, position=mpos, size=msize, record=record, res=zs))
        pos = at
    assert pos == footer_pos, "the footer follows the last block"
    assert [(m["c1"], m["c2"]) for m in matrices] == sorted((m["c1"], m["c2"]) for m in matrices)
    return dict(header=header, matrices=matrices, footer=dict(position=footer_pos, nbytes=nbytes, keys=[e[0] for e in entries], index=index), vectors=vectors)


def cells_of(parsed, chroms, bin_size):
    """the decoded cells of one bin size as sorted (bin1, bin2, count) with genome-wide bin ids"""
    off, _ = offsets([L for _, L in chroms], bin_size)
    out = []
    for m in parsed["matrices"]:
        for z in m["res"]:
            if z["bin_size"] == bin_size:
                for blk in z["blocks"]:
                    out += [(off[m["c1"]] + x, off[m["c2"]] + y, c) for x, y, c in blk["records"]]
    return sorted(out)
