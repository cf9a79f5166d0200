"""The expected-contact definition of include/mkt.h (mkt_matrix_expected) restated in plain numpy: the CHECKER of the GPU code.
Imports nothing from the package under test.  Modelled on cooltools `expected-cis` / `expected-trans` and on juicer's genome-wide
vector; parity with cooltools and juicer is unpinned (neither is run).

  cells (bin1 <= bin2, count) of one resolution, nbins, the chromosomes' first bins `offsets` (file order), weights or None
  1. weights None: every bin valid, w = 1; else valid(k) = w[k] is not NaN
  2. v = (count * w[bin1]) * w[bin2] in float64; a cell is used when both bins are valid
  3. cis table, nbins rows: row off_c + d = (chromosome c, diagonal d); n_valid = pairs (i, i + d) of valid bins inside c;
     count_sum (exact) and balanced_sum (sum of v) over the used cells of c with bin2 - bin1 == d
  4. trans table, a row per pair a < b at a * (2 * n_chr - a - 1) / 2 + (b - a - 1): n_valid = nvalid_a * nvalid_b, the sums over the
     used cells of the block, expected = balanced_sum / n_valid (NaN when n_valid == 0)
  5. genome-wide, a row per d < max n_c: the cis rows added over the chromosomes in file order; expected = S / N (NaN when N == 0)
  6. smoothed: diagonal 0 alone, then groups [e, e + max(1, e >> 3)) from e = 1, clipped; sum of S / sum of N, both in ascending d
  7. values in cell order: balanced = v; oe = v / expected[d] (cis) or v / expected(block) (trans); oe_smooth with the smoothed
     expected for cis cells; NaN for a cell with a masked bin"""
import collections

import numpy as np

Cis = collections.namedtuple("Cis", "n_valid count_sum balanced_sum")
Trans = collections.namedtuple("Trans", "n_valid count_sum balanced_sum expected")
Genome = collections.namedtuple("Genome", "n_valid count_sum balanced_sum expected expected_smooth")
Result = collections.namedtuple("Result", "cis trans genome balanced oe oe_smooth seg seg_cells used smooth_groups")


def smooth_edges(rows):
    """the first diagonal of every group of a table of `rows` diagonals, and rows itself at the end"""
    edges = [0]
    e = 1
    while e < rows:
        edges.append(e)
        e += max(1, e >> 3)
    if rows > 0:
        edges.append(rows)
    return edges


def _div(s, n):
    out = np.full(len(s), np.nan)
    ok = np.asarray(n) > 0
    out[ok] = np.asarray(s, dtype=np.float64)[ok] / np.asarray(n)[ok].astype(np.float64)
    return out


def expected(bin1, bin2, count, nbins, offsets, weights=None):
    """-> Result.  seg: the segment of every cell (cis: its row of the cis table, trans: nbins + its row of the trans table);
    seg_cells: USED cells per segment (what a sum's rounding bound is made of); used: per cell."""
    b1 = np.asarray(bin1, dtype=np.int64)
    b2 = np.asarray(bin2, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.uint64)
    off = np.asarray(list(offsets), dtype=np.int64)
    nchr = len(off)
    n_c = np.diff(np.append(off, nbins))
    w = np.ones(nbins, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    valid = ~np.isnan(w)
    chrom = np.searchsorted(off, np.arange(nbins), side="right") - 1          # the last chromosome that starts at or before the bin
    ca, cb = chrom[b1], chrom[b2]
    trans_rows = nchr * (nchr - 1) // 2
    seg = np.where(ca == cb, off[ca] + (b2 - b1), nbins + ca * (2 * nchr - ca - 1) // 2 + (cb - ca - 1))
    used = valid[b1] & valid[b2]
    v = (cnt.astype(np.float64) * w[b1]) * w[b2]
    nseg = nbins + trans_rows
    csum = np.zeros(nseg, dtype=np.uint64)
    np.add.at(csum, seg[used], cnt[used])
    bsum = np.bincount(seg[used], weights=v[used], minlength=nseg)
    seg_cells = np.bincount(seg[used], minlength=nseg)
    # n_valid of (c, d): pairs of valid bins d apart inside the chromosome
    nv = np.zeros(nbins, dtype=np.uint64)
    for c in range(nchr):
        m = valid[off[c]:off[c] + n_c[c]]
        for d in range(n_c[c]):
            nv[off[c] + d] = np.count_nonzero(m[:n_c[c] - d] & m[d:])
    cis = Cis(nv, csum[:nbins], bsum[:nbins])
    nvc = np.array([int(valid[off[c]:off[c] + n_c[c]].sum()) for c in range(nchr)], dtype=np.uint64)
    tn = np.array([nvc[a] * nvc[b] for a in range(nchr) for b in range(a + 1, nchr)], dtype=np.uint64)
    trans = Trans(tn, csum[nbins:], bsum[nbins:], _div(bsum[nbins:], tn))
    rows = int(n_c.max()) if nchr else 0
    N = np.zeros(rows, dtype=np.uint64)
    C = np.zeros(rows, dtype=np.uint64)
    S = np.zeros(rows, dtype=np.float64)
    for c in range(nchr):                                                      # file order, one chromosome after the other
        N[:n_c[c]] += cis.n_valid[off[c]:off[c] + n_c[c]]
        C[:n_c[c]] += cis.count_sum[off[c]:off[c] + n_c[c]]
        S[:n_c[c]] += cis.balanced_sum[off[c]:off[c] + n_c[c]]
    smooth = np.full(rows, np.nan)
    edges = smooth_edges(rows)
    for a, b in zip(edges[:-1], edges[1:]):
        ss = np.cumsum(S[a:b])[-1]                                             # cumsum adds in ascending order
        nn = int(N[a:b].sum())
        if nn:
            smooth[a:b] = ss / float(nn)
    genome = Genome(N, C, S, _div(S, N), smooth)
    cis_cell = ca == cb
    d = np.where(cis_cell, b2 - b1, 0)
    tr = np.where(cis_cell, 0, seg - nbins)
    nan = np.full(b1.size, np.nan)
    te = trans.expected[tr] if trans_rows else nan
    ge = genome.expected[d] if rows else nan
    gs = genome.expected_smooth[d] if rows else nan
    balanced = np.where(used, v, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        oe = np.where(used, v / np.where(cis_cell, ge, te), np.nan)
        oes = np.where(used, v / np.where(cis_cell, gs, te), np.nan)
    return Result(cis, trans, genome, balanced, oe, oes, seg, seg_cells, used, max(len(edges) - 1, 0))
