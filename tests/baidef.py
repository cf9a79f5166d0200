"""TEST INFRASTRUCTURE: the BAI index of a coordinate-sorted BAM as DESIGN.md defines it ("The index, exactly"), built from the
decoded file alone: plain loops over bamio's records, nothing from the package under test.  tests/test_gpu_bam.py compares the
index sam2bam wrote with bai_bytes(bai_definition(bam)) byte for byte and reports a difference through explain().  The builder is
itself checked against indexes written out by hand in tests/test_baidef_host.py (no GPU).  Parity with `samtools index` stays
UNPINNED (samtools is never run); what is pinned is the definition."""
import struct

import bamio

BLOCK = 0xff00                      # uncompressed bytes of every BGZF data block but the last
PSEUDO_BIN = 37450
MAX_REF = 1 << 29                   # bases a BAI index can address


class BaiDef(list):
    """[(bins {bin: [(beg, end)]}, lin [..], meta ((beg, end), (mapped, unmapped)) | None)] per reference, plus n_no_coor"""
    n_no_coor = 0


def block_table(bam: bamio.Bam):
    """[(compressed offset, uncompressed size)] of the data blocks and the compressed offset of the EOF marker block.  Asserts the
    layout the virtual offsets below rest on: every data block but the last holds 0xff00 bytes, the last block is the empty marker."""
    starts = bam._starts
    assert starts and starts[-1][2] == 0, "the last BGZF block is not the empty end-of-file marker"
    data = [(coff, n) for _, coff, n in starts[:-1]]
    for k, (_, n) in enumerate(data):
        if k + 1 < len(data):
            assert n == BLOCK, f"data block {k} holds {n} bytes, not 0xff00"
        else:
            assert 0 < n <= BLOCK, f"last data block holds {n} bytes"
    return data, starts[-1][1]


def voff_fn(bam: bamio.Bam):
    """voff(u) = coffset(block u // 0xff00) << 16 | u % 0xff00.  The data end maps to the EOF block only when it is a multiple of
    0xff00; otherwise it points behind the last byte of the last data block (bamio.Bam.voff maps it to the EOF block always)."""
    data, eof = block_table(bam)
    total = sum(n for _, n in data)
    assert total == bam.raw_len

    def voff(u):
        assert 0 <= u <= total
        k, w = divmod(u, BLOCK)
        if k == len(data):
            assert u == total and w == 0
            return eof << 16
        return data[k][0] << 16 | w
    return voff, total


def _uoffs(bam: bamio.Bam):
    """[u_0 .. u_n]: where each record starts in the uncompressed stream (block_size included), then the data end.  Recovered from
    bamio's virtual offsets: the block of a start offset is never ambiguous (a record holds at least 36 bytes)."""
    by_coff = {coff: u for u, coff, _ in bam._starts}
    us = [by_coff[v0 >> 16] + (v0 & 0xFFFF) for v0, _, _ in bam.records]
    us.append(bam.raw_len)
    assert all(a < b for a, b in zip(us, us[1:]))
    return us


def bai_definition(bam: bamio.Bam):
    """The index of DESIGN.md, or None where none is written (a reference longer than 2^29, a record ending past 2^29 or reaching a
    window >= (LN >> 14) + 2)."""
    voff, total = voff_fn(bam)
    us = _uoffs(bam)
    nref = len(bam.refs)
    if any(ln > MAX_REF for _, ln in bam.refs):
        return None
    out = BaiDef()
    per = [dict(bins={}, lin={}, beg=None, end=None, mapped=0, unmapped=0) for _ in range(nref)]
    runs = []                                               # (tid, bin, chunk_beg) in file order
    first_no_coor = None
    prev = None
    for i, (_, _, r) in enumerate(bam.records):
        tid = r["tid"]
        if tid < 0:
            out.n_no_coor += 1
            if first_no_coor is None:
                first_no_coor = voff(us[i])
            prev = None                                     # (no placed record follows one without coordinates in a sorted file;
            continue                                        # if one did, it would start a run)
        beg, end = bamio.ref_span(r)
        b = bamio.reg2bin(beg, end)
        v0, v1 = voff(us[i]), voff(us[i + 1])
        R = per[tid]
        w0, w1 = max(beg, 0) >> 14, max(end - 1, 0) >> 14
        if end > MAX_REF or w1 >= (bam.refs[tid][1] >> 14) + 2:
            return None
        if prev != (tid, b):
            runs.append((tid, b, v0))
            prev = (tid, b)
        R["beg"] = v0 if R["beg"] is None else min(R["beg"], v0)
        R["end"] = v1 if R["end"] is None else max(R["end"], v1)
        R["unmapped" if r["flag"] & 4 else "mapped"] += 1
        for w in range(w0, w1 + 1):
            R["lin"][w] = min(R["lin"].get(w, v0), v0)
    off_end = first_no_coor if first_no_coor is not None else voff(total)
    for k, (tid, b, v0) in enumerate(runs):
        per[tid]["bins"].setdefault(b, []).append((v0, runs[k + 1][2] if k + 1 < len(runs) else off_end))
    for R in per:
        lin = []
        if R["lin"]:
            lin = [None] * (max(R["lin"]) + 1)
            nxt = 0
            for w in range(len(lin) - 1, -1, -1):
                nxt = R["lin"].get(w, nxt)
                lin[w] = nxt
        meta = None if R["beg"] is None else ((R["beg"], R["end"]), (R["mapped"], R["unmapped"]))
        out.append((dict(sorted(R["bins"].items())), lin, meta))
    return out


def bai_bytes(index, n_no_coor=None) -> bytes:
    """SAMv1 5.2.  index: a BaiDef (or any list of (bins, lin, meta) with n_no_coor given); None: no index, no bytes."""
    if index is None:
        return b""
    if n_no_coor is None:
        n_no_coor = index.n_no_coor
    o = [b"BAI\1", struct.pack("<i", len(index))]
    for bins, lin, meta in index:
        o.append(struct.pack("<i", len(bins) + (meta is not None)))
        for b in sorted(bins):
            o.append(struct.pack("<Ii", b, len(bins[b])))
            o.extend(struct.pack("<QQ", c0, c1) for c0, c1 in bins[b])
        if meta is not None:
            o.append(struct.pack("<Ii", PSEUDO_BIN, 2))
            o.extend(struct.pack("<QQ", a, b) for a, b in meta)
        o.append(struct.pack("<i", len(lin)))
        o.append(struct.pack("<%dQ" % len(lin), *lin))
    o.append(struct.pack("<Q", n_no_coor))
    return b"".join(o)


def _v(x):
    return f"{x >> 16}:{x & 0xFFFF}"


def _parse(data: bytes):
    """like bamio.Bai, but keeps the order of the bins as written"""
    assert data[:4] == b"BAI\1", "no BAI magic"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    p = 8
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, p)[0]
        p += 4
        bins = []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, p)
            p += 8
            bins.append((b, [struct.unpack_from("<QQ", data, p + 16 * k) for k in range(n_chunk)]))
            p += 16 * n_chunk
        n_intv = struct.unpack_from("<i", data, p)[0]
        p += 4
        lin = list(struct.unpack_from("<%dQ" % n_intv, data, p))
        p += 8 * n_intv
        refs.append((bins, lin))
    tail = data[p:]
    return refs, (struct.unpack("<Q", tail)[0] if len(tail) == 8 else tail)


def explain(got_bytes: bytes, want) -> str:
    """Names the first difference between an index file and the defined one (reference, bin or window, both values as
    compressed:uncompressed offsets); "" when the bytes are equal."""
    want_bytes = bai_bytes(want)
    if got_bytes == want_bytes:
        return ""
    if want is None:
        return f"an index of {len(got_bytes)} bytes where the definition has none"
    if not got_bytes:
        return "no index where the definition has one"
    try:
        got, got_nc = _parse(got_bytes)
    except (AssertionError, struct.error) as e:
        return f"index does not parse: {e!r}"
    if len(got) != len(want):
        return f"n_ref: got {len(got)}, want {len(want)}"
    for t, ((gbins, glin), (wbins, wlin, wmeta)) in enumerate(zip(got, want)):
        wlist = [(b, list(wbins[b])) for b in sorted(wbins)]
        if wmeta is not None:
            wlist.append((PSEUDO_BIN, [tuple(wmeta[0]), tuple(wmeta[1])]))
        if [b for b, _ in gbins] != [b for b, _ in wlist]:
            gs, ws = [b for b, _ in gbins], [b for b, _ in wlist]
            extra, missing = [b for b in gs if b not in ws], [b for b in ws if b not in gs]
            return f"reference {t}: bins differ: got {len(gs)}, want {len(ws)}; not wanted {extra[:8]}, missing {missing[:8]}" + \
                   ("" if extra or missing else "; same bins in another order")
        for (b, gc), (_, wc) in zip(gbins, wlist):
            if gc == wc:
                continue
            if b == PSEUDO_BIN:
                if len(gc) == 2 and gc[0] != wc[0]:
                    return f"reference {t}: pseudo-bin file range: got ({_v(gc[0][0])}, {_v(gc[0][1])}), want ({_v(wc[0][0])}, {_v(wc[0][1])})"
                return f"reference {t}: pseudo-bin (mapped, unmapped): got {gc[1:]}, want {wc[1:]}"
            if len(gc) != len(wc):
                k = next((k for k, (a, c) in enumerate(zip(gc, wc)) if a != c), min(len(gc), len(wc)))
                return f"reference {t} bin {b}: got {len(gc)} chunks, want {len(wc)}; first difference at chunk {k}: got " + \
                       (f"({_v(gc[k][0])}, {_v(gc[k][1])})" if k < len(gc) else "none") + ", want " + (f"({_v(wc[k][0])}, {_v(wc[k][1])})" if k < len(wc) else "none")
            k = next(k for k, (a, c) in enumerate(zip(gc, wc)) if a != c)
            return f"reference {t} bin {b} chunk {k} of {len(wc)}: got ({_v(gc[k][0])}, {_v(gc[k][1])}), want ({_v(wc[k][0])}, {_v(wc[k][1])})"
        if len(glin) != len(wlin):
            return f"reference {t}: n_intv: got {len(glin)}, want {len(wlin)}"
        for w, (a, c) in enumerate(zip(glin, wlin)):
            if a != c:
                return f"reference {t} window {w}: got {_v(a)}, want {_v(c)}"
    if got_nc != want.n_no_coor:
        return f"n_no_coor: got {got_nc!r}, want {want.n_no_coor}"
    return "bytes differ, but no field does (serialisation)"
