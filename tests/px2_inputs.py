"""The inputs of the pairs.gz / .px2 tests, built deterministically (no random source): the smallest shapes at which the index can go
wrong.  tests/golden/px2_golden.json holds what the reference's bgzip | pairix made of each of them.

A case: {"name", "text" (bytes), "regions" ([str], queried in the golden), "refused" (None, or the 1-based line this project's
error names)}.  The reference accepts some of the refused inputs; the golden records what it did."""

HEADER = b"## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
W = 1 << 15                            # the finest bin and the linear window (tests/px2def.py LIDX_SHIFT)
BLOCK = 0xFF00                         # the text bytes of one BGZF block of this project


def rec(i, c1, p1, c2, p2, pad=0):
    return b"r%d%s\t%s\t%d\t%s\t%d\t%s\t%s\n" % (i, b"x" * pad, c1.encode(), p1, c2.encode(), p2, b"+-"[i % 2:i % 2 + 1], b"-+"[i % 3 % 2:i % 3 % 2 + 1])


def _minimal():
    one = HEADER + rec(1, "chr1", 100, "chr1", 5000)
    return [
        {"name": "header_only", "text": HEADER, "regions": ["chr1|chr1"], "refused": None},
        {"name": "one_record", "text": one, "regions": ["chr1:1-200|chr1:1-6000", "chr1:101-200|chr1:1-6000", "chr1:1-200|chr1:1-4999", "chr1|chr2"], "refused": None},
        {"name": "no_final_newline", "text": HEADER + rec(1, "chr1", 100, "chr1", 5000) + rec(2, "chr1", 70000, "chr2", 5)[:-1],
         "regions": ["chr1:1-200|chr1:1-6000", "chr1:60000-80000|chr2:1-10"], "refused": None},
        {"name": "no_header", "text": rec(1, "chr1", 3 * W + 7, "chr1", 9) + rec(2, "chr1", 3 * W + 8, "chr1", 9), "regions": ["chr1:1-200000|chr1:1-10", "chr1:1-%d|chr1:1-10" % (3 * W)],
         "refused": None},
        {"name": "meta_in_middle", "text": HEADER + rec(1, "a", 5, "b", 5) + b"#mid\n" + rec(2, "a", 40000, "b", 7) + b"#mid2\n" + rec(3, "b", 7, "b", 8) + b"#end\n",
         "regions": ["a:1-100000|b:1-10", "b:1-10|b:1-10"], "refused": None},
    ]


CHROMS = ["chr1", "chr2", "chr10", "chrX", "chrUn_KI270742v1", "c", "chrM", "chr2_random_alt"]


def _many_pairs():
    out = [HEADER]
    i = 0
    for a in range(len(CHROMS)):
        for b in range(a, len(CHROMS)):               # 36 pairs, upper triangle, cis and trans
            if (a * 7 + b) % 6 == 5:
                continue                              # ... of which 30 occur
            n = 1 + (a * 3 + b) % 5
            for k in range(n):
                i += 1
                out.append(rec(i, CHROMS[a], 1 + k * (W // 2) * (1 + a % 3) + b, CHROMS[b], 1000 * (k + 1) + a))
    regions = ["chr1:1-100000|chr2:1-100000", "chr10:1-40000|chrUn_KI270742v1:1-5000", "c:1-%d|c:1-100000" % (4 * W), "chrM|chr2_random_alt", "chr2|chr1"]
    return [{"name": "many_pairs", "text": b"".join(out), "regions": regions, "refused": None}]


def _bin_edges():
    # pos1 on both sides of every edge of every level (2^15, 2^18, ... 2^30) and of the linear window: pairix indexes pos1 - 1
    edges = [W, 2 * W, 1 << 18, 1 << 21, 1 << 24, 1 << 27, 1 << 30]
    out = [HEADER]
    i = 0
    for e in edges:
        for p in (e - 1, e, e + 1, e + 2):
            i += 1
            out.append(rec(i, "chr1", p, "chr1", p + 10))
    # a gap of several empty windows inside a pair (above: 2W+2 .. 2^18) and before a pair's first record
    for p in (5 * W + 1, 5 * W + 1, 9 * W, 9 * W + 1):
        i += 1
        out.append(rec(i, "chr1", p, "chr2", 77))
    regions = ["chr1:%d-%d|chr1:1-2000000000" % (W, W), "chr1:%d-%d|chr1:1-2000000000" % (W + 1, 2 * W), "chr1:%d-%d|chr1:1-2000000000" % ((1 << 18) - 5, (1 << 24) + 1),
               "chr1:1-%d|chr2:1-100" % (5 * W), "chr1:%d-%d|chr2:70-80" % (5 * W + 1, 9 * W), "chr1:%d-%d|chr1:1-2000000000" % ((1 << 30) - 1, (1 << 30) + 5)]
    return [{"name": "bin_edges", "text": b"".join(out), "regions": regions, "refused": None}]


def _large():
    out = [HEADER]
    for i, p in enumerate([0, 1, (1 << 30) + 1, (1 << 31) - W, (1 << 31) - 2, (1 << 31) - 1, (1 << 31) - 1]):
        out.append(rec(i, "chr1", p, "chr1", 5))
    over = HEADER + rec(1, "chr1", 5, "chr1", 5) + rec(2, "chr1", 1 << 31, "chr1", 5)
    return [{"name": "large_positions", "text": b"".join(out), "regions": ["chr1:1-1|chr1:1-10", "chr1:2147450000-2147483647|chr1:1-10"], "refused": None},
            {"name": "position_past_int32", "text": over, "regions": [], "refused": 4}]


def _blocks(name, step, pad0=0):
    """About three BGZF blocks.  Block edge 1: a chunk ends and a line starts exactly on it.  Edge 2: a line straddles it.  Edge 3: the
    boundary between two pairs falls on it.  step: pos1 advance per line (small: few long runs; W: a new bin on almost every line); pad0: longer read names, so fewer lines."""
    out = [HEADER]
    at = len(HEADER)
    i = 0
    pos = 1
    pair = ("chr1", "chr1")
    edge = 1
    total = 3 * BLOCK + 1500
    while at < total:
        i += 1
        pos += step if i % 7 else 0                   # every seventh line repeats a position
        ln = rec(i, pair[0], pos, pair[1], pos + 3, pad=pad0)
        target = edge * BLOCK
        near = 2 * len(ln) + 20                       # close enough that this line can be stretched to end on the edge
        if edge <= 3 and edge != 2 and target - at < near:
            ln = rec(i, pair[0], pos, pair[1], pos + 3, pad=pad0 + target - at - len(ln))      # this line ends exactly on the edge
            assert at + len(ln) == target
            edge += 1
            if edge == 2:
                pos = (pos // W + 1) * W + 1          # edge 1: the next line opens a new bin
            else:
                pair, pos = ("chr1", "chr2"), 1       # edge 3: the next line opens a new pair
        elif edge == 2 and target - at < near:
            if at + len(ln) > target:
                edge += 1                             # edge 2: this line straddles
        out.append(ln)
        at += len(ln)
    text = b"".join(out)
    lines = text.split(b"\n")
    starts = set()
    a = 0
    for ln in lines:
        starts.add(a)
        a += len(ln) + 1
    assert BLOCK in starts and 3 * BLOCK in starts and 2 * BLOCK not in starts and 2 * BLOCK - 1 not in starts
    assert 150000 <= len(text) <= 200000
    last = pos
    regions = ["chr1:1-%d|chr1:1-2000000000" % (50 * step), "chr1:%d-%d|chr1:1-2000000000" % (last // 2, last // 2 + 3 * max(step, 40)), "chr1:1-%d|chr2:1-%d" % (W, W), "chr1:%d-%d|chr2:1-2000000000" % (pos - step, pos)]
    return {"name": name, "text": text, "regions": regions, "refused": None}


def _refused():
    good = HEADER + rec(1, "chr1", 100, "chr1", 5) + rec(2, "chr1", 200, "chr1", 5) + rec(3, "chr1", 300, "chr2", 5)
    return [
        {"name": "unsorted", "text": good + rec(4, "chr1", 299, "chr2", 5) + rec(5, "chr2", 1, "chr2", 5), "regions": [], "refused": 6},
        {"name": "pair_reappears", "text": good + rec(4, "chr1", 400, "chr1", 5), "regions": [], "refused": 6},
        {"name": "four_columns", "text": good + b"r4\tchr1\t400\tchr2\n" + rec(5, "chr1", 500, "chr2", 5), "regions": [], "refused": 6},
        {"name": "empty_line", "text": good + b"\n", "regions": [], "refused": 6},
        {"name": "pos1_not_a_number", "text": good + b"r4\tchr1\t4x0\tchr2\t5\t+\t-\n", "regions": [], "refused": 6},
        {"name": "pos1_empty", "text": HEADER + b"r1\tchr1\t\tchr2\t5\t+\t-\n", "regions": [], "refused": 3},
    ]


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _minimal() + _many_pairs() + _bin_edges() + _large() + [_blocks("blocks_long_runs", 37), _blocks("blocks_many_bins", W, pad0=120)] + _refused()
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


def accepted():
    return [c for c in cases() if c["refused"] is None]


def refused():
    return [c for c in cases() if c["refused"] is not None]
