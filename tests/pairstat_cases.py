"""Directed inputs of the pair statistics (mkt_pairstat_* of include/mkt.h), shared by tests/test_pairstat_host.py and
tests/test_gpu_pairstat.py.  Every family is a dict: name, table, text, tol_permille, min_count, and `want`, what can be said about its
result by hand (checked against the definition, tests/pairstatdef.py, without a GPU).  MALFORMED holds (text, refused line)."""
import pairstatdef as pd

BIG = 3_000_000_000
ROWS = [(b"chr1", BIG), (b"chr2", 50_000), (b"chr3", 40_000), (b"chr4", 30_000), (b"chr5", 20_000), (b"chr6", 10_000), (b"chr7", 5_000), (b"chrM", 16_569)]
TABLE = b"".join(n + b"\t%d\n" % L for n, L in ROWS)
ORI = ((b"+", b"+"), (b"+", b"-"), (b"-", b"+"), (b"-", b"-"))
LINES_PER_WG = 2048                                              # kPsLinesPerWg of mkt_pairstat.hip


def line(rid, c1, p1, c2, p2, s1=None, s2=None, more=()):
    f = [rid, c1, b"%d" % p1, c2, b"%d" % p2] + ([s1] if s1 is not None else []) + ([s2] if s2 is not None else []) + list(more)
    return b"\t".join(f) + b"\n"


def edge_distances():
    d = {0, 999, 1000, 9999, 10000, 10 ** 9, 10 ** 9 + 1, 2 * 10 ** 9}
    for e in pd.EDGES:
        d.update(x for x in (e - 1, e, e + 1) if x >= 0)
    for t in pd.THRESHOLDS:
        d.update((t - 1, t))
    return sorted(d)


def edges_family():
    out = [b"## pairs format v1.0\n", b"#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"]
    ds = edge_distances()
    for i, d in enumerate(ds):
        for o, (s1, s2) in enumerate(ORI):
            lo, hi = 7 + i, 7 + i + d
            p1, p2 = (hi, lo) if (i + o) & 1 else (lo, hi)         # pos1 > pos2 on every other line
            out.append(line(b"e%d_%d" % (i, o), b"chr1", p1, b"chr1", p2, s1, s2))
    n = len(ds)
    want = {"total": 4 * n, "skipped": 0, "counted": 4 * n, "cis": 4 * n, "trans": 0, "no_strand": 0, "header_lines": 2,
            "cis0": 4 * sum(1 for d in ds if d < 1000), "cis1K": 4 * sum(1 for d in ds if 1000 <= d < 10000), "cis10K": 4 * sum(1 for d in ds if d >= 10000)}
    for key, t in zip(pd.GE_KEYS, pd.THRESHOLDS):
        want[key] = 4 * sum(1 for d in ds if d >= t)
    # by hand: where single distances land
    want["bins"] = {0: 0, 1: 2, 2: 4, 3: 5, 999: 24, 1000: 25, 1333: 25, 1334: 26, 9999: 32, 10000: 33, 10 ** 9 - 1: 72, 10 ** 9: 73, 2 * 10 ** 9: 73}
    want["empty_bins"] = (1, 3)
    return dict(name="edges", table=TABLE, text=b"".join(out), tol_permille=50, min_count=1000, want=want)


def strands_family():
    L = [
        line(b"s0", b"chr2", 100, b"chr2", 1200),                                    # five columns
        line(b"s1", b"chr2", 100, b"chr2", 1200, b"+"),                              # six
        line(b"s2", b"chr2", 100, b"chr2", 1200, b"++", b"-"),                       # a two-byte strand
        line(b"s3", b"chr2", 100, b"chr2", 1200, b"+", b"--"),
        line(b"s4", b"chr2", 100, b"chr2", 1200, b"", b"-"),                         # an empty one
        line(b"s5", b"chr2", 100, b"chr2", 1200, b"+", b""),
        line(b"s6", b"chr2", 100, b"chr2", 1200, b".", b"+"),                        # other bytes
        line(b"s7", b"chr2", 100, b"chr2", 1200, b"-", b"*"),
        line(b"s8", b"chr2", 100, b"chr2", 1200, b"-", b"+\r"),
        line(b"s9", b"chr2", 100, b"chr3", 1200, b"x", b"y"),                        # trans without strands
        line(b"s10", b"chr2", 100, b"chr2", 1200, b"-", b"+"),                       # good ones: seven columns, and more behind them
        line(b"s11", b"chr2", 1200, b"chr2", 100, b"+", b"-", (b"UU", b"60", b"")),
        line(b"s12", b"chr3", 100, b"chr2", 1200, b"-", b"-"),                       # trans with strands
        line(b"s13", b"chr2", 100, b"chr2", 1200, b"+", b"+")[:-1],                  # the last line has no newline
    ]
    want = {"total": 14, "skipped": 0, "counted": 14, "cis": 12, "trans": 2, "no_strand": 10, "header_lines": 0, "cis_1kb+": 12, "cis_2kb+": 0, "cis0": 0, "cis1K": 12, "cis10K": 0,
            "dist_rows": {25: [1, 1, 1, 0]}, "chrom": {(1, 1): 12, (1, 2): 1, (2, 1): 1}}
    return dict(name="strands", table=TABLE, text=b"".join(L), tol_permille=50, min_count=1000, want=want)


def skips_family():
    L = [
        line(b"k0", b"chrU", 5, b"chr2", 6, b"+", b"+"), line(b"k1", b"chr2", 5, b"chrU", 6, b"+", b"+"),             # unknown name
        line(b"k2", b"chr2", 0, b"chr2", 6, b"+", b"+"), line(b"k3", b"chr2", 5, b"chr2", 0, b"+", b"+"),             # position 0
        line(b"k4", b"chr2", 50_000, b"chr2", 6, b"+", b"+"), line(b"k5", b"chr2", 5, b"chr2", 50_000, b"-", b"-"),   # position L: counted
        line(b"k6", b"chr2", 50_001, b"chr2", 6, b"+", b"+"), line(b"k7", b"chr2", 5, b"chr2", 50_001, b"+", b"+"),   # L + 1
        line(b"k8", b"", 5, b"chr2", 6, b"+", b"+"), line(b"k9", b"chr2", 5, b"c" * 64, 6, b"+", b"+"),               # no name, a name of 64 bytes
        b"k10\tchr2\t99999999999999999999\tchr2\t6\t+\t+\n", b"k11\tchr2\t007\tchr3\t40000\t+\t-\n",                  # 20 digits; leading zeros
        line(b"k12", b"chr1", BIG, b"chr1", 1, b"-", b"+"), line(b"k13", b"chr1", BIG + 1, b"chr1", 1, b"-", b"+"),
        line(b"k14", b"chr22", 5, b"chr2", 6, b"+", b"+"), line(b"k15", b"chr", 5, b"chr2", 6, b"+", b"+"),            # a name longer and shorter than one in the table
    ]
    want = {"total": 16, "skipped": 12, "counted": 4, "cis": 3, "trans": 1, "no_strand": 0, "cis_10kb+": 3, "cis_40kb+": 3, "cis0": 2, "cis1K": 0, "cis10K": 7, "ref_trans": 7,
            "dist_rows": {38: [1, 0, 0, 1], 73: [0, 0, 1, 0]}, "chrom": {(1, 1): 2, (1, 2): 1, (0, 0): 1}}
    return dict(name="skips", table=TABLE, text=b"".join(L), tol_permille=50, min_count=1000, want=want)


def lines_family(n):
    """n data lines: cis pairs on chr1 whose distance grows with the line, a trans pair every 11th line, orientations in turn"""
    out = []
    trans = 0
    for i in range(n):
        s1, s2 = ORI[i & 3]
        if i % 11 == 10:
            out.append(line(b"l%d" % i, b"chr2", 1 + i, b"chr3", 2 + i, s1, s2))
            trans += 1
        else:
            out.append(line(b"l%d" % i, b"chr1", 1000 + i, b"chr1", 1000 + i + 37 * i, s1, s2))
    want = {"total": n, "skipped": 0, "counted": n, "cis": n - trans, "trans": trans, "no_strand": 0, "chrom": {(0, 0): n - trans, (1, 2): trans}}
    return dict(name="lines_%d" % n, table=TABLE, text=b"".join(out), tol_permille=50, min_count=1000, want=want)


LINE_COUNTS = (63, 64, 65, 255, 256, 257, LINES_PER_WG - 1, LINES_PER_WG, LINES_PER_WG + 1, 2 * LINES_PER_WG + 1)


def waves_families():
    small = ROWS[1:]                                              # chr2 .. chrM: seven names; with chr1 eight, 64 ordered pairs
    one = b"".join(line(b"w%d" % i, b"chr3", 10 + i, b"chr5", 20 + i, b"+", b"-") for i in range(64))
    names = [n for n, _ in ROWS]
    distinct = b"".join(line(b"d%d" % i, names[i >> 3], 1 + i, names[i & 7], 2 + i, b"-", b"-") for i in range(64))
    alt = b"".join(line(b"a%d" % i, b"chr2" if i & 1 else b"chr4", 10 + i, b"chr2" if i & 1 else b"chr6", 500 + i, b"+", b"+") for i in range(64))
    assert len(small) == 7
    return [
        dict(name="wave_one_pair", table=TABLE, text=one, tol_permille=50, min_count=1000,
             want={"total": 64, "counted": 64, "trans": 64, "cis": 0, "chrom": {(2, 4): 64}}),
        dict(name="wave_64_pairs", table=TABLE, text=distinct, tol_permille=50, min_count=1000,
             want={"total": 64, "counted": 64, "trans": 56, "cis": 8, "chrom": {(a, b): 1 for a in range(8) for b in range(8)}}),
        dict(name="wave_two_pairs", table=TABLE, text=alt, tol_permille=50, min_count=1000,
             want={"total": 64, "counted": 64, "trans": 32, "cis": 32, "cis0": 32, "chrom": {(1, 1): 32, (3, 5): 32}, "dist_rows": {22: [32, 0, 0, 0]}}),
    ]


def _bin_lines(tag, d, counts):
    out = []
    for o, c in enumerate(counts):
        for i in range(c):
            out.append(line(b"%s_%d_%d" % (tag, o, i), b"chr1", 100 + i, b"chr1", 100 + i + d, *ORI[o]))
    return out


def convergence_families():
    """bin 9 [10, 13): (40, 0, 0, 0); bin 17 [100, 133): (11, 10, 10, 9); bin 25 [1000, 1334): (10, 10, 10, 10); bin 40 [74989, 100000):
    (39, 0, 0, 0).  With T = 40: (11, 10, 10, 9) deviates by |44 - 40| * 1000 = 4000 = 4 * 40 * 25, balanced from 25 permille on;
    (40, 0, 0, 0) by 120000 = 4 * 40 * 750."""
    text = b"".join(_bin_lines(b"a", 10, (40, 0, 0, 0)) + _bin_lines(b"b", 100, (11, 10, 10, 9)) + _bin_lines(b"c", 1000, (10, 10, 10, 10)) + _bin_lines(b"d", 75000, (39, 0, 0, 0)))
    rows = {9: [40, 0, 0, 0], 17: [11, 10, 10, 9], 25: [10, 10, 10, 10], 40: [39, 0, 0, 0]}
    out = []
    for tol, mc, conv in ((25, 40, 100), (24, 40, 1000), (25, 41, -1), (750, 40, 10), (749, 40, 100), (25, 39, -1), (1000, 39, 10), (0, 40, 1000), (50, 1000, -1), (0, 0, 100000)):
        out.append(dict(name="convergence_tol%d_min%d" % (tol, mc), table=TABLE, text=text, tol_permille=tol, min_count=mc,
                        want={"total": 159, "cis": 159, "convergence_dist": conv, "dist_rows": rows}))
    return out


def families():
    return [edges_family(), strands_family(), skips_family()] + [lines_family(n) for n in LINE_COUNTS] + waves_families() + convergence_families()


# (text, the refused line): fewer than five columns, an empty line, a position that is no plain decimal
GOOD = line(b"g", b"chr2", 5, b"chr2", 6, b"+", b"-")
MALFORMED = [
    (GOOD + b"four\tchr2\t5\tchr2\n", 2),
    (b"#h\n" + GOOD + b"\n" + GOOD, 3),
    (GOOD * 3 + b"x\tchr2\t12a\tchr2\t6\t+\t+\n", 4),
    (b"x\tchr2\t5\tchr2\t-6\t+\t+\n" + GOOD, 1),
    (b"x\tchr2\t\tchr2\t6\t+\t+\n", 1),
    (b"x\tchrU\t5\tchr2\t6.0\n", 1),                               # refused although its chromosome would have made it skipped
    (GOOD * 70 + b"one\n" + GOOD * 70 + b"two\n", 71),            # the smallest of two
    (GOOD * 5 + b"x\tchr2\t5\tchr2", 6),                           # the carried last line
]


def name_table(n):
    return b"".join(b"c%d\t%d\n" % (i, 1000 + i) for i in range(n))
