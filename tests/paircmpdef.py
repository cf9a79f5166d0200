"""The pair-level concordance of two .pairs texts (include/mkt.h, mkt_paircmp_*) in plain Python, with dicts: the definition the GPU
path and the host half of the library are held to.  tests/test_paircmp_host.py pins it to what the reference's script printed."""

COMMENT, SUPERSEDED, ONLY, CONSISTENT, DISCORDANT = 0, 1, 2, 3, 4
DIST_KEYS = ("cis_lt_1k", "cis_1_10k", "cis_gt_10k", "trans")


class BadLine(ValueError):
    def __init__(self, side, number):
        super().__init__(f"file {side} line {number}")
        self.side, self.number = side, number


def split_lines(text):
    """the lines of a text without their newlines; a last line without one counts"""
    rows = text.split(b"\n")
    if rows and rows[-1] == b"":
        rows.pop()
    return rows


def parse(text, side):
    """[(id, c1, p1 text, c2, p2 text) or None for a comment] per line"""
    out = []
    for k, row in enumerate(split_lines(text)):
        if row.startswith(b"#"):
            out.append(None)
            continue
        f = row.split(b"\t")
        if len(f) < 5 or not all(x.isdigit() and x.isascii() and int(x) < (1 << 31) for x in (f[2], f[4])):
            raise BadLine(side, k + 1)
        out.append(tuple(f[:5]))
    return out


def _dist_class(r):
    if r[1] != r[3]:
        return 3
    d = abs(int(r[4]) - int(r[2]))
    return 2 if d > 10000 else 0 if d < 1000 else 1


def consistent(a, b, D):
    straight = a[1] == b[1] and abs(int(a[2]) - int(b[2])) < D and a[3] == b[3] and abs(int(a[4]) - int(b[4])) < D
    swapped = a[1] == b[3] and abs(int(a[2]) - int(b[4])) < D and a[3] == b[1] and abs(int(a[4]) - int(b[2])) < D
    return straight or swapped


def millions(n):
    return "%.15g" % (n / 1e6)


class Result:
    pass


def compare(text_a, text_b, max_dist=200):
    """Result with: classes_a, classes_b (bytes, one per line), the counters (as microcket_amd.PairCompare.run returns them, without
    host_runs) and the inconsistent text split in its I/B part and its A part"""
    D = max_dist or 200
    ra, rb = parse(text_a, "A"), parse(text_b, "B")
    ca = bytearray(len(ra))
    cb = bytearray(len(rb))
    dist = [[0] * 4, [0] * 4]
    value = {}                                                        # id -> line of A that holds its unclaimed value
    for k, r in enumerate(ra):
        if r is None:
            continue
        dist[0][_dist_class(r)] += 1
        if r[0] in value:
            ca[value[r[0]]] = SUPERSEDED
        value[r[0]] = k
        ca[k] = ONLY
    distinct = len(value)
    ib = []
    for k, r in enumerate(rb):
        if r is None:
            continue
        dist[1][_dist_class(r)] += 1
        if r[0] in value:
            j = value.pop(r[0])
            ok = consistent(ra[j], r, D)
            ca[j] = cb[k] = CONSISTENT if ok else DISCORDANT
            if not ok:
                ib.append(b"\t".join((b"I", r[0]) + ra[j][1:] + (b"vs",) + r[1:]) + b"\n")
        else:
            cb[k] = ONLY
            ib.append(b"\t".join((b"B",) + r) + b"\n")
    res = Result()
    res.classes_a, res.classes_b = bytes(ca), bytes(cb)
    res.lines_ib = b"".join(ib)
    res.lines_a = b"".join(b"\t".join((b"A",) + ra[j]) + b"\n" for j in sorted(value.values()))
    res.lines = res.lines_ib + res.lines_a
    res.info = dict(lines=[len(ra), len(rb)], data_lines=[sum(r is not None for r in ra), sum(r is not None for r in rb)], distinct_a=distinct,
                    consistent=cb.count(CONSISTENT), discordant=cb.count(DISCORDANT), a_only=ca.count(ONLY), b_only=cb.count(ONLY),
                    dist=[dict(zip(DIST_KEYS, d)) for d in dist], lines_bytes=len(res.lines))
    res.max_dist = D
    return res


def report(res, name_a, name_b):
    i = res.info
    out = f"Using Distance: {res.max_dist}\nLoading file A: {name_a} ...\nLoading file B: {name_b} ...\n\n"
    out += f"Overalp report:\nA_only\t{millions(i['a_only'] + i['discordant'])}\nB_only\t{millions(i['b_only'] + i['discordant'])}\n"
    out += f"Consistent\t{millions(i['consistent'])}\n#Disconcordant\t{millions(i['discordant'])}\n\n"
    for s, d in zip("AB", i["dist"]):
        out += f"Pairs distribution report (file {s}):\nCis (<1 K)\t{millions(d['cis_lt_1k'])}\nCis (1-10 K)\t{millions(d['cis_1_10k'])}\n"
        out += f"Cis (>10 K)\t{millions(d['cis_gt_10k'])}\nTrans\t{millions(d['trans'])}\n\n"
    return out.encode()
