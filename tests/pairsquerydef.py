"""The definition of a batch of region queries on final.pairs.gz through its .px2 (mkt_bgzf_query of include/mkt.h, bin/pairsquery), in
plain Python on top of tests/px2def.py, which has the single region (`query`, `parse_region`) and is left as it is.

What is added here, as probed from pairix 0.3.7 (tests/golden/pairsquery_golden.json records its answers, tests/make_pairsquery_golden.py
made them):

  * the strict region grammar and its refusals (`parse_region`), `*` as one side and autoflip (`expand`);
  * the selection of chunks of one sub-query with overlapping chunks merged (`select_spans`);
  * the block plan: which BGZF members a batch has to inflate (`plan`);
  * the answer of a batch, a list of lines per region (`answer`), by a walk over the spans that never looks outside them.
"""
import bisect

import px2def

WHOLE = (0, 1 << 30)                   # a side without a range: pairix takes [0, 2^30) on either side (px2def.parse_region says 2^31, which
                                       # differs on the second side only: an explicit second range is not clipped, the first always is)
MAX_DIGITS = 18                        # a bound of more digits is no number
MAX_LINE = (1 << 24) - 2               # a candidate line of more bytes never matches and is counted as unparsed


class RegionError(ValueError):
    """A region that is refused; .index is its position in the batch."""

    def __init__(self, index, what):
        ValueError.__init__(self, "region %d: %s" % (index, what))
        self.index = index
        self.what = what


def _bound(s, index):
    s = s.replace(",", "")
    if not s or not s.isdigit() or not s.isascii() or len(s) > MAX_DIGITS:
        raise RegionError(index, "a bound of a range is no number")
    return int(s)


def parse_side(side, index):
    """(chromosome or None for '*', (beg, end) 0-based half-open)"""
    if side == "*":
        return None, WHOLE
    if ":" not in side:
        if not side:
            raise RegionError(index, "an empty chromosome name")
        return side, WHOLE
    c, r = side.rsplit(":", 1)
    if not c:
        raise RegionError(index, "an empty chromosome name")
    if c == "*":
        raise RegionError(index, "the * side takes no range")
    parts = r.split("-")
    if len(parts) != 2:
        raise RegionError(index, "a bound of a range is no number")
    b, e = _bound(parts[0], index), _bound(parts[1], index)
    if b > e:
        raise RegionError(index, "the start coordinate must not exceed the end coordinate")
    return c, (max(b - 1, 0), e)       # pairix answers b = 0 as b = 1 (recorded in the golden)


def parse_region(region, index=0):
    """((chrA or None, range), (chrB or None, range)); RegionError for what is refused."""
    sides = region.split("|")
    if len(sides) == 1:
        raise RegionError(index, "no '|': a one-sided query on a 2D file is not offered")
    if len(sides) != 2:
        raise RegionError(index, "more than one '|'")
    a, b = parse_side(sides[0], index), parse_side(sides[1], index)
    if a[0] is None and b[0] is None:
        raise RegionError(index, "*|* is not offered")
    return a, b


def expand(names, region, autoflip=False, index=0):
    """The sub-queries [(name id, b1, e1, b2, e2)] of one region: a star is every name whose other side is the chromosome given, in
    the order of the name table; with autoflip a pair that is absent while its flip is present is answered flipped."""
    (ca, ra), (cb, rb) = parse_region(region, index)
    out = []
    if ca is None or cb is None:
        for tid, nm in enumerate(names):
            x, _, y = nm.partition(b"|")
            if (cb is None and x == ca.encode("latin-1")) or (ca is None and y == cb.encode("latin-1")):
                out.append((tid, ra[0], ra[1], rb[0], rb[1]))
        return out
    first = {}
    for tid, nm in enumerate(names):
        first.setdefault(nm, tid)
    nm, fl = (ca + "|" + cb).encode("latin-1"), (cb + "|" + ca).encode("latin-1")
    if nm in first:
        out.append((first[nm], ra[0], ra[1], rb[0], rb[1]))
    elif autoflip and fl in first:
        out.append((first[fl], rb[0], rb[1], ra[0], ra[1]))
    return out


class File:
    """A .gz and its .px2, parsed once."""

    def __init__(self, gz, px2):
        self.gz, self.ix = gz, px2def.parse_px2(px2)
        self.blocks = px2def.bgzf_blocks(gz, check=False)
        self.coffs = [b[0] for b in self.blocks]
        self._text = None

    @property
    def text(self):
        if self._text is None:
            self._text = px2def.bgzf_inflate(self.gz)
        return self._text

    def member_of(self, v):
        """(member index, text offset) of a virtual offset; ValueError when the index does not belong to this file"""
        c, o = v >> 16, v & 0xFFFF
        if c == len(self.gz) and o == 0:
            return len(self.blocks), (self.blocks[-1][2] + self.blocks[-1][3] if self.blocks else 0)
        k = bisect.bisect_left(self.coffs, c)
        if k == len(self.blocks) or self.coffs[k] != c or o > self.blocks[k][3]:
            raise ValueError("the index does not belong to this file")
        return k, self.blocks[k][2] + o

    def select_spans(self, sub):
        """[(a, z, first member, last member)] of one sub-query in text offsets, ascending, overlapping ones merged; the member behind
        an end that has in-block offset 0 is not among them."""
        tid, b1, e1 = sub[0], sub[1], min(sub[2], px2def.QUERY_END_MAX)
        if b1 >= e1:
            return []
        lin = self.ix["linear"][tid]
        min_off = lin[min(b1 >> px2def.LIDX_SHIFT, len(lin) - 1)] if lin else 0
        chunks = []
        for b, cc in self.ix["bins"][tid].items():
            lo, hi = px2def.bin_range(b)
            if lo < e1 and b1 < hi:
                chunks += [(x, y) for x, y in cc if y > min_off]
        out = []
        for x, y in sorted(chunks):
            (kx, a), (ky, z) = self.member_of(x), self.member_of(y)
            if z <= a:
                continue
            kend = ky if y & 0xFFFF else ky - 1
            if out and a < out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], z), out[-1][2], max(out[-1][3], kend))
            else:
                out.append((a, z, kx, kend))
        return out

    def plan(self, regions, autoflip=False):
        """{"subqueries": [(region index, name id, b1, e1, b2, e2)], "spans": [(sub-query index, a, z)], "members": [ascending member
        indexes to inflate], "runs": number of runs of adjacent members}"""
        subs, spans, members = [], [], set()
        for r, region in enumerate(regions):
            for sub in expand(self.ix["names"], region, autoflip, r):
                for a, z, kx, kend in self.select_spans(sub):
                    spans.append((len(subs), a, z))
                    members.update(range(kx, kend + 1))
                subs.append((r,) + sub)
        members = sorted(members)
        return {"subqueries": subs, "spans": spans, "members": members, "runs": sum(1 for i, k in enumerate(members) if i == 0 or members[i - 1] + 1 != k)}

    def answer(self, regions, autoflip=False, info=None):
        """One list of lines (bytes, without the newline) per region."""
        p = self.plan(regions, autoflip)
        text = self.text
        out = [[] for _ in regions]
        unparsed = cand = 0
        for s, a, z in p["spans"]:
            r, tid, b1, e1, b2, e2 = p["subqueries"][s]
            e1 = min(e1, px2def.QUERY_END_MAX)
            ca, _, cb = self.ix["names"][tid].partition(b"|")
            for x, y in px2def.split_lines(text[a:z]):
                ln = text[a + x:a + y]
                cand += 1
                m = match_line(ln, ca, cb, b1, e1, b2, e2)
                unparsed += m == 2
                if m == 1:
                    out[r].append(ln)
        if info is not None:
            info.update(unparsed=unparsed, candidate_lines=cand, subqueries=len(p["subqueries"]), chunks=len(p["spans"]), blocks_inflated=len(p["members"]),
                        bytes_inflated=sum(self.blocks[k][3] for k in p["members"]), lines=sum(len(x) for x in out))
        return out


def _number(f):
    return int(f) if f and f.isdigit() and len(f) <= 10 and int(f) <= px2def.POS_MAX else None


def match_line(ln, ca, cb, b1, e1, b2, e2):
    """0 no match, 1 match, 2 unparsed (fewer than five columns, or a pos1 / pos2 that is no decimal number <= 2^31 - 1, or a line of
    more than MAX_LINE bytes): the filter of one candidate line."""
    if ln[:1] == b"#":
        return 0
    cols = ln.split(b"\t", 5)
    if len(ln) > MAX_LINE or len(cols) < 5:
        return 2
    p1, p2 = _number(cols[2]), _number(cols[4])
    if p1 is None or p2 is None:
        return 2
    if cols[1] != ca or cols[3] != cb:
        return 0
    return 1 if max(p1 - 1, 0) < e1 and b1 < max(p1, 1) and max(p2 - 1, 0) < e2 and b2 < max(p2, 1) else 0


def answer(gz, px2, regions, autoflip=False):
    return File(gz, px2).answer(regions, autoflip)


def golden_lines(entry):
    """what a golden entry records: ("lines", [str]) for a short answer, ("sha256", (n, hex)) of pairix's stdout for a long one"""
    return ("lines", entry["lines"]) if "lines" in entry else ("sha256", (entry["n"], entry["sha256"]))


def same_as_golden(entry, lines):
    """lines: [bytes] without newlines"""
    import hashlib
    if "lines" in entry:
        return [ln.decode("latin-1") for ln in lines] == entry["lines"]
    return (len(lines), hashlib.sha256(printed(lines)).hexdigest()) == (entry["n"], entry["sha256"])


def printed(lines):
    """pairix's stdout for a list of answered lines"""
    return b"".join(ln + b"\n" for ln in lines)


# ---- what the golden asks of every accepted case of px2_inputs ------------------------------------------------------------------------
REFUSED = ["chr1", "chr1|chr2|chr3", "chr1:10-5|chr2", "chr1:a-5|chr2", "chr1:5|chr2", "chr1:-5|chr2", "chr1:1-|chr2", "|chr2", "chr1|", ":1-5|chr2", "*|*", "*:1-5|chr2"]


def names_of(text):
    out = []
    for a, b in px2def.split_lines(text):
        if text[a:a + 1] != b"#":
            c = text[a:b].split(b"\t")
            nm = (c[1] + b"|" + c[3]).decode("latin-1")
            if nm not in out:
                out.append(nm)
    return out


def requests(c):
    """{"single": [regions], "autoflip": [regions asked with -a], "batch": [regions of one call]} of a case of px2_inputs"""
    names = names_of(c["text"]) or ["chr1|chr1"]
    a, b = names[0].split("|")
    pos = 1
    for x, y in px2def.split_lines(c["text"]):
        if c["text"][x:x + 1] != b"#":
            pos = max(int(c["text"][x:y].split(b"\t")[2]), 1)
            break
    trans = [n.split("|") for n in names if n.split("|")[0] != n.split("|")[1] and "|".join(n.split("|")[::-1]) not in names]
    single = ["%s:1-100000|*" % a, "*|%s:1-100000" % b, "%s|*" % a, "*|%s" % b, "%s:%d-%d|%s" % (a, pos, pos, b), "%s:0-100000|%s" % (a, b), "%s:0-0|%s" % (a, b),
              "%s|%s:0-100000" % (a, b), "%s:1-100,000|%s:1-2,000,000,000" % (a, b), "%s:1-1073741823|%s" % (a, b), "%s:1-1073741824|%s" % (a, b),
              "%s:1-1073741825|%s" % (a, b), "%s:1073741824-1073741824|%s" % (a, b), "%s:1073741825-1073741830|%s" % (a, b), "%s|%s" % (a, b), "zz|%s" % a]
    flip = ["zz|%s" % a, "%s|%s" % (a, b)] + c["regions"][:1]
    for x, y in trans[:2]:
        flip += ["%s|%s" % (y, x), "%s:1-200000|%s:1-70000" % (y, x), "%s:1-70000|%s:1-200000" % (y, x)]
        single += ["%s|%s" % (y, x)]
    # (pairix ends a call at a pair that is absent while its flip is present; such a region stays out of the batch)
    base = [q for q in c["regions"] if "|".join(x.rsplit(":", 1)[0] if ":" in x else x for x in q.split("|")) in names or
            "|".join(x.rsplit(":", 1)[0] if ":" in x else x for x in q.split("|")[::-1]) not in names]
    batch = base + base[:1] + ["%s|%s" % (a, b), "zz|%s" % a, "%s:1-100000|*" % a] + base[::-1]
    return {"single": single, "autoflip": flip, "batch": batch}
