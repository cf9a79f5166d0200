"""The contact-matrix definition of include/mkt.h (mkt_matrix_*) restated in plain Python / numpy: the CHECKER of the GPU code.
Imports nothing from the package under test.

  table: lines name<TAB>length, file order = bin order; for a resolution r chromosome i owns ceil(L_i / r) bins,
  bin(chr_i, pos) = off_i + (pos - 1) // r for 1-based positions; a pair is skipped when a chromosome is not in the table or a
  position is 0 or > L_i; every other pair adds 1 to cell (min(b1, b2), max(b1, b2)); the result is the list of non-empty cells
  ascending in (bin1, bin2)."""
import numpy as np


def parse_table(text: bytes):
    """[(name, length)] in file order; empty and '#' lines ignored"""
    out = []
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r")
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        out.append((f[0], int(f[1])))
    return out


def bin_layout(table, r):
    """(offsets per chromosome, bins per chromosome, nbins)"""
    n = [-(-L // r) for _, L in table]
    off = [0]
    for k in n:
        off.append(off[-1] + k)
    return off[:-1], n, off[-1]


POS_SAT = 1 << 40                                                   # see parse_pairs


def parse_pairs(pairs_text: bytes, flags=None):
    """(chrA names, posA, chrB names, posB) of the pair lines ('#' lines ignored); flags: one per pair line, truthy = left out.
    A line with fewer than five columns or a non-decimal position raises ValueError (a position that ends in '\\r' is one: only
    columns past the fifth may carry the '\\r' of a CRLF line).
    A position is a decimal number of any length, leading zeros allowed; it is capped at POS_SAT = 2^40.  Every tabulated length is
    below 2^32, so the cap changes no result: it only states that a number of 13 digits or more is "past every chromosome's end"
    and nothing else, however many digits follow (int() here cannot wrap; a 64-bit accumulator without the cap would)."""
    ca, pa, cb, pb = [], [], [], []
    k = 0
    lines = pairs_text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        if line.startswith(b"#"):
            continue
        f = line.split(b"\t")
        if len(f) < 5 or not f[2].isdigit() or not f[4].isdigit():
            raise ValueError(f"not a .pairs line: {line[:80]!r}")
        keep = flags is None or not flags[k]
        k += 1
        if keep:
            ca.append(f[1]); pa.append(min(int(f[2]), POS_SAT)); cb.append(f[3]); pb.append(min(int(f[4]), POS_SAT))
    return ca, pa, cb, pb


def definition_arrays(table, resolutions, ia, pa, ib, pb):
    """ia / ib: table index per pair (-1: not in the table), pa / pb: 1-based positions.  {r: (cells, skipped)} with cells a
    (k, 3) uint64 array of (bin1, bin2, count) ascending in (bin1, bin2)."""
    ia, pa, ib, pb = (np.asarray(x, dtype=np.int64) for x in (ia, pa, ib, pb))
    L = np.array([l for _, l in table], dtype=np.int64)
    ok = (ia >= 0) & (ib >= 0) & (pa >= 1) & (pb >= 1)
    ok &= pa <= L[np.maximum(ia, 0)]
    ok &= pb <= L[np.maximum(ib, 0)]
    skipped = int((~ok).sum())
    ia, pa, ib, pb = ia[ok], pa[ok], ib[ok], pb[ok]
    out = {}
    for r in resolutions:
        off, _, nbins = bin_layout(table, r)
        off = np.array(off, dtype=np.int64)
        b1 = off[ia] + (pa - 1) // r
        b2 = off[ib] + (pb - 1) // r
        lo, hi = np.minimum(b1, b2).astype(np.uint64), np.maximum(b1, b2).astype(np.uint64)
        key = lo * np.uint64(max(nbins, 1)) + hi                    # nbins < 2^32: no overflow
        uniq, cnt = np.unique(key, return_counts=True)
        cells = np.stack([uniq // np.uint64(max(nbins, 1)), uniq % np.uint64(max(nbins, 1)), cnt.astype(np.uint64)], axis=1) if uniq.size else np.zeros((0, 3), dtype=np.uint64)
        out[r] = (cells.astype(np.uint64), skipped)
    return out


def definition(chromsizes_text: bytes, resolutions, pairs_text: bytes, flags=None):
    """{r: (cells, skipped)} for .pairs text; see definition_arrays"""
    table = parse_table(chromsizes_text)
    index = {}
    for i, (nm, _) in enumerate(table):
        index.setdefault(nm, i)
    ca, pa, cb, pb = parse_pairs(pairs_text, flags)
    ia = [index.get(x, -1) for x in ca]
    ib = [index.get(x, -1) for x in cb]
    return definition_arrays(table, resolutions, ia, pa, ib, pb)


def n_pairs(pairs_text: bytes, flags=None):
    return len(parse_pairs(pairs_text, flags)[0])


def coo_text(cells) -> bytes:
    """bin1<TAB>bin2<TAB>count per cell"""
    return b"".join(b"%d\t%d\t%d\n" % (int(a), int(b), int(c)) for a, b, c in np.asarray(cells).tolist())


def cells_of_text(text: bytes):
    if not text:
        return np.zeros((0, 3), dtype=np.uint64)
    return np.array([[int(x) for x in line.split(b"\t")] for line in text.split(b"\n")[:-1]], dtype=np.uint64)


def bins_bed(chromsizes_text: bytes, r) -> bytes:
    """chrom<TAB>start<TAB>end per bin, 0-based half-open, end clipped to the chromosome length"""
    out = []
    for nm, L in parse_table(chromsizes_text):
        for s in range(0, L, r):
            out.append(b"%s\t%d\t%d\n" % (nm, s, min(s + r, L)))
    return b"".join(out)


def stat_text(pairs, skipped, nnz_by_res) -> bytes:
    """<prefix>.matrix.stat; nnz_by_res: [(r, nnz)] in the order of the resolution list"""
    return (f"Pairs\t{pairs}\nBinned\t{pairs - skipped}\nSkipped\t{skipped}\n" + "".join(f"nnz.{r}\t{n}\n" for r, n in nnz_by_res)).encode()


# the hand-computed example: table deliberately NOT in bytewise order; r = 100 -> chrB bins 0..9, chrA 10..12, chrC 13
HAND_TABLE = b"chrB\t1000\nchrA\t250\nchrC\t10\n"
HAND_RES = 100
HAND_PAIRS = (
    b"r1\tchrA\t1\tchrB\t1\t+\t-\n"          # bins 10 and 0: the text's order of the two sides is the reverse of the bin order -> (0, 10)
    b"r2\tchrB\t1000\tchrB\t1000\t+\t+\n"    # pos = L: the last bin -> (9, 9)
    b"r3\tchrB\t1001\tchrB\t5\t-\t+\n"       # pos = L + 1: skipped
    b"r4\tchrA\t0\tchrA\t10\t+\t+\n"         # pos = 0: skipped
    b"r5\tchrB\t5\tchrZ\t5\t+\t-\n"          # unknown name: skipped
    b"r6\tchrA\t250\tchrA\t201\t-\t-\n"      # pos = L inside the partial last bin -> (12, 12)
    b"r7\tchrB\t150\tchrB\t950\t+\t-\n"      # (1, 9)
    b"r8\tchrB\t199\tchrB\t901\t+\t-\n"      # (1, 9)
    b"r9\tchrB\t101\tchrB\t1000\t-\t-\n"     # (1, 9): three pairs in one cell
    b"r10\tchrA\t100\tchrC\t10\t+\t+\n"      # (10, 13)
    b"r11\tchrA\t101\tchrC\t1\t+\t+\n"       # (11, 13)
    b"r12\tchrB\t500\tchrC\t11\t+\t+\n"      # pos > L of chrC: skipped
    b"r13\tchrA\t251\tchrA\t1\t+\t+\n"       # pos > L of chrA: skipped
)
HAND_CELLS = [(0, 10, 1), (1, 9, 3), (9, 9, 1), (10, 13, 1), (11, 13, 1), (12, 12, 1)]
HAND_PAIRS_N, HAND_SKIPPED = 13, 5
HAND_COO = b"0\t10\t1\n1\t9\t3\n9\t9\t1\n10\t13\t1\n11\t13\t1\n12\t12\t1\n"
HAND_BED = (b"".join(b"chrB\t%d\t%d\n" % (s, s + 100) for s in range(0, 1000, 100)) +
            b"chrA\t0\t100\nchrA\t100\t200\nchrA\t200\t250\nchrC\t0\t10\n")
HAND_STAT = b"Pairs\t13\nBinned\t8\nSkipped\t5\nnnz.100\t6\n"
