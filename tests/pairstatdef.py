"""The definition of the pair statistics (mkt_pairstat_* of include/mkt.h) in plain Python: integers are Python ints, the only floats
are one conversion of an exact area and one division per bin.  Nothing here is fast or clever; it is the yardstick of
microcket_amd.PairStats, bin/pairsstat and tests/host/pairstat_host.cpp."""
import numpy as np

BINS = 74
LAST_HI = 1 << 32
THRESHOLDS = (1000, 2000, 4000, 10000, 20000, 40000)
GE_KEYS = ("cis_1kb+", "cis_2kb+", "cis_4kb+", "cis_10kb+", "cis_20kb+", "cis_40kb+")
ORI = ("++", "+-", "-+", "--")
MAX_CHROM = 2048


def edges():
    """0, then round(10^(k/8)) for k = 0 .. 72, derived with numpy (no value is nearer than 0.001 to a rounding tie)"""
    return [0] + [int(np.round(np.float64(10.0) ** (np.float64(k) / 8.0))) for k in range(BINS - 1)]


EDGES = edges()


def bin_of(d):
    """(number of edges <= d) - 1"""
    return sum(1 for e in EDGES if e <= d) - 1


def bin_hi(k):
    return EDGES[k + 1] if k + 1 < BINS else LAST_HI


class BadTable(ValueError):
    pass


class TooManyNames(ValueError):
    pass


class BadLine(ValueError):
    def __init__(self, number):
        ValueError.__init__(self, f"line {number}")
        self.number = number


def parse_table(text: bytes):
    """[(name, length)]: the grammar of mkt_matrix_create"""
    rows = []
    for ln in text.split(b"\n"):
        ln = ln[:-1] if ln.endswith(b"\r") else ln
        if not ln or ln.startswith(b"#"):
            continue
        f = ln.split(b"\t")
        if not 1 <= len(f[0]) <= 63 or len(f) < 2 or not f[1].isdigit() or len(f[1]) > 11 or int(f[1]) >= 1 << 32:
            raise BadTable(ln)
        rows.append((f[0], int(f[1])))
    if not rows:
        raise BadTable("empty")
    if len(rows) > MAX_CHROM:
        raise TooManyNames(len(rows))
    if len({n for n, _ in rows}) != len(rows):
        raise BadTable("a name twice")
    return rows


def _plain_decimal(f: bytes):
    return len(f) > 0 and all(48 <= c <= 57 for c in f)


class Result:
    pass


def areas(lengths):
    out = []
    for k in range(BINS):
        lo, hi = EDGES[k], bin_hi(k)
        a = 0
        for L in lengths:
            m = min(hi, L)
            if m > lo:
                a += sum(L - d for d in range(lo, m)) if m - lo <= 64 else (m - lo) * L - (lo + m - 1) * (m - lo) // 2
        out.append(a)
    return out


def convergence(dist, tol_permille, min_count):
    T = [sum(r) for r in dist]
    thick = [t >= min_count for t in T]
    balanced = [thick[k] and all(abs(4 * c - T[k]) * 1000 <= 4 * T[k] * tol_permille for c in dist[k]) for k in range(BINS)]
    for K in range(BINS):
        if thick[K] and balanced[K] and all(balanced[k] for k in range(K + 1, BINS) if thick[k]):
            return EDGES[K]
    return -1


def fmt(x: float) -> str:
    return "%.17g" % x


def stats(table: bytes, text: bytes, tol_permille=50, min_count=1000, skip=None) -> Result:
    """skip: None, or a byte string with one byte per data line (non-zero: the line is left out, as a flagged key is)"""
    rows = parse_table(table)
    index = {n: i for i, (n, _) in enumerate(rows)}
    n = len(rows)
    r = Result()
    c = {k: 0 for k in ("total", "skipped", "cis", "trans", "no_strand", "header_lines", "cis0", "cis1K", "cis10K", "ref_trans") + GE_KEYS}
    dist = [[0, 0, 0, 0] for _ in range(BINS)]
    chrom = [[0] * n for _ in range(n)]
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                            # the text ended with its newline
    nd = 0
    for number, ln in enumerate(lines, 1):
        if ln.startswith(b"#"):
            c["header_lines"] += 1
            continue
        f = ln.split(b"\t")
        if len(f) < 5 or not _plain_decimal(f[2]) or not _plain_decimal(f[4]):
            raise BadLine(number)
        nd += 1
        if skip is not None and skip[nd - 1]:
            continue
        c["total"] += 1
        ia, ib = index.get(f[1]), index.get(f[3])
        p1, p2 = min(int(f[2]), 1 << 40), min(int(f[4]), 1 << 40)             # what exceeds 2^40 counts as 2^40
        # the reference's classes: every data line, by name bytes and distance alone
        c["ref_trans" if f[1] != f[3] else "cis0" if abs(p2 - p1) < 1000 else "cis1K" if abs(p2 - p1) < 10000 else "cis10K"] += 1
        if ia is None or ib is None or p1 < 1 or p2 < 1 or p1 > rows[ia][1] or p2 > rows[ib][1]:
            c["skipped"] += 1
            continue
        chrom[ia][ib] += 1
        stranded = len(f) >= 7 and f[5] in (b"+", b"-") and f[6] in (b"+", b"-")
        if not stranded:
            c["no_strand"] += 1
        if ia != ib:
            c["trans"] += 1
            continue
        c["cis"] += 1
        d = abs(p2 - p1)
        for key, t in zip(GE_KEYS, THRESHOLDS):
            if d >= t:
                c[key] += 1
        if stranded:
            dist[bin_of(d)][(2 if f[5] == b"-" else 0) + (1 if f[6] == b"-" else 0)] += 1
    c["counted"] = c["total"] - c["skipped"]
    c["convergence_dist"] = convergence(dist, tol_permille, min_count)
    r.info, r.dist, r.chrom, r.names = c, dist, chrom, [nm for nm, _ in rows]
    r.area = areas([L for _, L in rows])
    r.area_f = [float(a) for a in r.area]                      # int -> float64 rounds to nearest even
    r.P = [float(sum(dist[k])) / r.area_f[k] if r.area[k] else 0.0 for k in range(BINS)]
    r.stat_text = stat_text(r)
    r.scaling_text = scaling_text(r)
    return r


def bin_name(k):
    return f"{EDGES[k]}+" if k + 1 == BINS else f"{EDGES[k]}-{EDGES[k + 1]}"


def stat_text(r) -> bytes:
    c = r.info
    o = [f"{k}\t{c[k]}\n" for k in ("total", "skipped", "counted", "cis", "trans", "no_strand", "header_lines") + GE_KEYS]
    o += [f"reference/{k}\t{c[v]}\n" for k, v in (("trans", "ref_trans"), ("cis10K", "cis10K"), ("cis1K", "cis1K"), ("cis0", "cis0"))]
    for k in ("cis",) + GE_KEYS + ("trans",):
        o.append(f"summary/frac_{k}\t{fmt(float(c[k]) / float(c['counted']) if c['counted'] else 0.0)}\n")
    o.append(f"summary/convergence_dist\t{c['convergence_dist']}\n")
    txt = "".join(o).encode()
    out = [txt]
    for a, na in enumerate(r.names):
        for b, nb in enumerate(r.names):
            if r.chrom[a][b]:
                out.append(b"chrom_freq/" + na + b"/" + nb + b"\t" + str(r.chrom[a][b]).encode() + b"\n")
    for k in range(BINS):
        for q in range(4):
            out.append(f"dist_freq/{bin_name(k)}/{ORI[q]}\t{r.dist[k][q]}\n".encode())
    return b"".join(out)


def scaling_text(r) -> bytes:
    o = ["lo\thi\tarea\t++\t+-\t-+\t--\ttotal\tP\n"]
    for k in range(BINS):
        d = r.dist[k]
        o.append(f"{EDGES[k]}\t{bin_hi(k)}\t{r.area[k]}\t{d[0]}\t{d[1]}\t{d[2]}\t{d[3]}\t{sum(d)}\t{fmt(r.P[k])}\n")
    return "".join(o).encode()


def reference_log(r):
    """the four distance classes under the reference's log keys"""
    return {"trans": r.info["ref_trans"], "cis10K": r.info["cis10K"], "cis1K": r.info["cis1K"], "cis0": r.info["cis0"]}
