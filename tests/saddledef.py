"""The saddle definition of include/mkt.h (mkt_matrix_saddle) restated in numpy: the CHECKER of the GPU code.  Imports nothing from the
package under test.  Step 1 is `groups`, step 2 `used_cells` and `cell_values`, step 3 `chunked` (the sums in the order of the
definition: per chunk of 4096 stored cells in ascending index, then the chunks in ascending order), step 4 `positions`, step 5 `tables`,
step 6 `scores` in plain Python loops; `saddle` runs them all."""
import collections
import math

import numpy as np

CHUNK = 4096
NONE = 255
KINDS = ("oe", "oe_smooth")
CONTACTS = ("cis", "trans")
DEFAULTS = dict(n_groups=50, trim_lo=250, trim_hi=250, contact="cis", kind="oe", min_diag=2, max_diag=0, corner=0)
TABLES = ("n", "nnz", "csum", "vsum", "mean")
FIELDS = TABLES + ("groups", "group_bins", "group_lo", "group_hi", "strength", "aa_ab", "bb_ab")
SCORES = ("strength", "aa_ab", "bb_ab")
Result = collections.namedtuple("Result", FIELDS + ("info",))


def groups(track, valid, Q, trim_lo, trim_hi):
    """step 1 -> (g uint8 [nbins], bins uint64 [Q], lo, hi float64 [Q], T candidates, K kept)"""
    t = np.asarray(track, dtype=np.float64)
    cand = np.flatnonzero(np.asarray(valid, dtype=bool) & ~np.isnan(t))
    order = cand[np.argsort(t[cand], kind="stable")]                          # ties (-0.0 == 0.0) keep the ascending bins
    T = int(order.size)
    lo, hi = T * trim_lo // 10000, T * trim_hi // 10000
    K = T - hi - lo
    kept = order[lo:T - hi]
    gg = (np.arange(K, dtype=np.int64) * Q) // K if K else np.zeros(0, dtype=np.int64)
    g = np.full(t.size, NONE, dtype=np.uint8)
    g[kept] = gg
    bins = np.bincount(gg, minlength=Q).astype(np.uint64)
    glo, ghi = np.full(Q, np.nan), np.full(Q, np.nan)
    for q in range(Q):
        r = np.flatnonzero(gg == q)
        if r.size:
            glo[q], ghi[q] = t[kept[r[0]]], t[kept[r[-1]]]                    # the lowest and the highest rank of the group
    return g, bins, glo, ghi, T, K


def chrom_of(off, nbins):
    return np.searchsorted(np.asarray(list(off), dtype=np.int64), np.arange(nbins), side="right") - 1


def trans_row(a, b, nchr):
    """the row of block (a < b) in the trans table of the expected section"""
    return a * (2 * nchr - a - 1) // 2 + (b - a - 1)


def used_cells(b1, b2, g, chrom, contact, min_diag, max_diag):
    """step 2 -> (used bool [nnz], a, b int64 [nnz]: the unordered entry of every cell)"""
    b1, b2 = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)
    gi, gj = g[b1].astype(np.int64), g[b2].astype(np.int64)
    d = b2 - b1
    same = chrom[b1] == chrom[b2]
    if contact == "cis":
        ok = same & (d >= min_diag)
        if max_diag:
            ok &= d <= max_diag
    else:
        ok = ~same
    return ok & (gi != NONE) & (gj != NONE), np.minimum(gi, gj), np.maximum(gi, gj)


def cell_values(cnt, b1, b2, weights):
    """v = ((double)count * w[bin1]) * w[bin2] of every cell: two multiplications in this order"""
    c = np.asarray(cnt, dtype=np.float64)
    if weights is None:
        return c
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (c * w[np.asarray(b1, dtype=np.int64)]) * w[np.asarray(b2, dtype=np.int64)]


def chunked(used, a, b, x, Q):
    """step 3 -> vsum [Q, Q] with the unordered entries (a <= b) filled.  x: the value of every cell (read where used)."""
    n = used.size
    chunks = (n + CHUNK - 1) // CHUNK
    ent = np.full(chunks * CHUNK, -1, dtype=np.int64)
    ent[:n] = np.where(used, a * Q + b, -1)
    val = np.zeros(chunks * CHUNK, dtype=np.float64)
    val[:n] = np.where(used, x, 0.0)
    ent, val = ent.reshape(chunks, CHUNK), val.reshape(chunks, CHUNK)
    T = np.zeros((chunks, Q * Q), dtype=np.float64)
    for s in range(CHUNK if chunks else 0):                                   # slot s of every chunk at once, the slots in ascending order
        rows = np.flatnonzero(ent[:, s] >= 0)
        if rows.size:
            T[rows, ent[rows, s]] += val[rows, s]                             # one cell per chunk: no entry twice
    vsum = np.zeros(Q * Q, dtype=np.float64)
    for k in range(chunks):
        vsum += T[k]
    return vsum.reshape(Q, Q)


def positions(g, off, nbins, Q, contact, min_diag, max_diag):
    """step 4 -> n uint64 [Q, Q] with the unordered entries (a <= b) filled"""
    offs = list(off) + [nbins]
    n = np.zeros((Q, Q), dtype=np.int64)
    ar = np.arange(Q)
    if contact == "trans":
        before = np.zeros(Q, dtype=np.int64)                                   # the group counts of the chromosomes before this one
        M = np.zeros((Q, Q), dtype=np.int64)
        for c in range(len(offs) - 1):
            gl = g[offs[c]:offs[c + 1]]
            h = np.bincount(gl[gl != NONE], minlength=Q).astype(np.int64)
            M += np.outer(before, h)
            before += h
        for a in range(Q):
            for b in range(a, Q):
                n[a][b] = M[a][b] + (M[b][a] if a != b else 0)
        return n.astype(np.uint64)
    for c in range(len(offs) - 1):
        gl = g[offs[c]:offs[c + 1]].astype(np.int64)
        nc = gl.size
        P = np.zeros((nc + 1, Q), dtype=np.int64)
        P[1:] = np.cumsum(gl[:, None] == ar[None, :], axis=0)
        i = np.flatnonzero(gl != NONE)
        lo = np.minimum(i + min_diag, nc)
        hi = np.maximum(np.minimum(i + max_diag + 1, nc) if max_diag else np.full(i.size, nc), lo)
        cnt = P[hi] - P[lo]                                                   # [grouped bins, Q]: the partners ahead of bin i, per group
        for a in range(Q):
            row = cnt[gl[i] == a].sum(axis=0)
            for b in range(Q):
                n[min(a, b)][max(a, b)] += row[b]
    return n.astype(np.uint64)


def _q(x, y):
    """x / y; a zero denominator and every NaN are the one quiet NaN"""
    if y == 0.0:
        return math.nan
    with np.errstate(all="ignore"):
        r = float(np.float64(x) / np.float64(y))
    return math.nan if r != r else r


def scores(vsum, n, Q):
    """step 6: the symmetric (or upper) tables -> (strength, aa_ab, bb_ab) float64 [Q // 2], index k - 1"""
    out = [np.zeros(Q // 2), np.zeros(Q // 2), np.zeros(Q // 2)]
    for k in range(1, Q // 2 + 1):
        bbs = aas = abs_ = 0.0
        bbn = aan = abn = 0
        for a in range(Q):
            for b in range(a, Q):
                v, c = float(vsum[a][b]), int(n[a][b])
                if b < k:
                    bbs += v; bbn += c
                if a >= Q - k:
                    aas += v; aan += c
                if a < k and b >= Q - k:
                    abs_ += v; abn += c
        ab = _q(abs_, float(abn))
        out[0][k - 1] = _q(_q(bbs + aas, float(bbn + aan)), ab)
        out[1][k - 1] = _q(_q(aas, float(aan)), ab)
        out[2][k - 1] = _q(_q(bbs, float(bbn)), ab)
    return out


def _sym(u):
    return np.ascontiguousarray(np.triu(u) + np.triu(u, 1).T)


def tables(used, a, b, cnt, vsum_u, n_u, Q):
    """step 5 -> the five symmetric tables"""
    nnz, csum = np.zeros(Q * Q, dtype=np.uint64), np.zeros(Q * Q, dtype=np.uint64)
    e = (a * Q + b)[used]
    np.add.at(nnz, e, np.uint64(1))
    np.add.at(csum, e, np.asarray(cnt, dtype=np.uint64)[used])
    n, nnz, csum, vsum = _sym(n_u), _sym(nnz.reshape(Q, Q)), _sym(csum.reshape(Q, Q)), _sym(vsum_u)
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, vsum / n.astype(np.float64), np.nan)
    return n, nnz, csum, vsum, mean


def corner_of(Q, corner):
    return corner if corner else max(1, Q // 5)


def saddle(b1, b2, cnt, nbins, off, track, weights=None, expected=None, expected_smooth=None, trans_expected=None, **opts):
    """the whole definition.  weights None: every bin valid, w = 1; expected / expected_smooth: the genome-wide tables by distance;
    trans_expected: the expected of the trans blocks, by row."""
    o = dict(DEFAULTS)
    o.update(opts)
    Q = o["n_groups"]
    assert set(o) == set(DEFAULTS) and o["kind"] in KINDS and o["contact"] in CONTACTS and 2 <= Q <= 64 and 0 <= o["corner"] <= Q // 2
    b1, b2 = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)
    valid = np.ones(nbins, dtype=bool) if weights is None else ~np.isnan(np.asarray(weights, dtype=np.float64))
    g, bins, glo, ghi, T, K = groups(track, valid, Q, o["trim_lo"], o["trim_hi"])
    chrom = chrom_of(off, nbins)
    used, a, b = used_cells(b1, b2, g, chrom, o["contact"], o["min_diag"], o["max_diag"])
    v = cell_values(cnt, b1, b2, weights)
    if o["contact"] == "cis":
        div = np.asarray(expected if o["kind"] == "oe" else expected_smooth, dtype=np.float64)[np.where(used, b2 - b1, 0)] if used.size else np.zeros(0)
    else:
        rows = trans_row(chrom[b1], chrom[b2], len(list(off)))
        div = np.asarray(trans_expected, dtype=np.float64)[np.where(used, rows, 0)] if used.size else np.zeros(0)
    with np.errstate(all="ignore"):
        x = v / div                                                           # one IEEE division per cell
    vsum_u = chunked(used, a, b, x, Q)
    n_u = positions(g, off, nbins, Q, o["contact"], o["min_diag"], o["max_diag"])
    n, nnz, csum, vsum, mean = tables(used, a, b, cnt, vsum_u, n_u, Q)
    st, aa, bb = scores(vsum, n, Q)
    k = corner_of(Q, o["corner"])
    info = dict(n_groups=Q, candidates=T, kept=K, cells_used=int(used.sum()), chunks=(used.size + CHUNK - 1) // CHUNK, corner=k,
                strength=float(st[k - 1]), aa_ab=float(aa[k - 1]), bb_ab=float(bb[k - 1]))
    return Result(n, nnz, csum, vsum, mean, g, bins, glo, ghi, st, aa, bb, info)
