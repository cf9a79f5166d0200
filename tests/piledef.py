"""The pileup definition of include/mkt.h (mkt_matrix_pileup) restated in numpy: the CHECKER of the GPU code.  Imports nothing from the
package under test.  Step 1 is `statuses`, steps 2 .. 3 `lookup` (once per feature list and flank: where every position's cell is) and
`values`, steps 4 .. 5 `chunked` (the sums in the order of the definition: per chunk of 256 features in ascending index, then the
chunks in ascending order), step 6 `scores` in plain Python loops; `pileup` runs them all."""
import collections
import math

import numpy as np

USED, TRANS, EDGE, DIST = 1, 2, 3, 4
CHUNK = 256
KINDS = ("balanced", "oe", "oe_smooth")
DEFAULTS = dict(flank=10, corner=6, kind="oe_smooth", ignore_diags=2, edges=0, min_dist=0, max_dist=0)
SCORES = ("peak", "p2ll", "p2ul", "p2ur", "p2lr", "p2m", "z_ll")
Lookup = collections.namedtuple("Lookup", "inside d idx")                  # [n, S * S]: both bins in the chromosome and valid; |j - i|; the cell's index or -1
Result = collections.namedtuple("Result", "n csum vsum mean status scores")


def statuses(a, b, off, nbins, flank, edges=0, min_dist=0, max_dist=0):
    """step 1 -> (status uint8 [n], lo, hi of the first anchor's chromosome [n]); a bad feature is a ValueError that names it"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    bad = np.flatnonzero((a > b) | (b >= nbins))
    if bad.size:
        raise ValueError(f"feature {int(bad[0])} ({int(a[bad[0]])}, {int(b[bad[0]])})")
    offa = np.asarray(list(off), dtype=np.int64)
    ends = np.append(offa[1:], nbins)
    ca, cb = np.searchsorted(offa, a, side="right") - 1, np.searchsorted(offa, b, side="right") - 1
    lo, hi = offa[ca], ends[ca]
    d = b - a
    st = np.full(a.size, USED, dtype=np.uint8)
    out = (a - flank < lo) | (a + flank >= hi) | (b - flank < lo) | (b + flank >= hi)
    if not edges:
        st[out] = EDGE
    st[(d < min_dist) | ((d > max_dist) if max_dist else False)] = DIST       # DIST before EDGE, TRANS before both
    st[ca != cb] = TRANS
    return st, lo, hi


def lookup(b1, b2, nbins, a, b, status, lo, hi, valid, flank, block=2048):
    """steps 2 and 3, without ignore_diags: for every feature and position in ascending (p, q) whether both bins are inside the chromosome
    and valid, the distance, and the index of the stored cell (min(i, j), max(i, j)) or -1.  Rows of features that are not used are empty."""
    S = 2 * flank + 1
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = a.size
    keys = np.asarray(b1, dtype=np.int64) * nbins + np.asarray(b2, dtype=np.int64)      # ascending: the cells are sorted by (bin1, bin2)
    assert (np.diff(keys) > 0).all()
    inside = np.zeros((n, S * S), dtype=bool)
    dist = np.zeros((n, S * S), dtype=np.int32)
    idx = np.full((n, S * S), -1, dtype=np.int32)
    P, Q = np.repeat(np.arange(-flank, flank + 1), S), np.tile(np.arange(-flank, flank + 1), S)
    used = np.flatnonzero(np.asarray(status) == USED)
    for at in range(0, used.size, block):
        u = used[at:at + block]
        i, j = a[u, None] + P[None, :], b[u, None] + Q[None, :]
        l, h = lo[u, None], hi[u, None]
        ok = (i >= l) & (i < h) & (j >= l) & (j < h)
        x, y = np.minimum(i, j), np.maximum(i, j)
        ok[ok] = valid[x[ok]] & valid[y[ok]]
        k = x[ok] * nbins + y[ok]
        at_ = np.searchsorted(keys, k)
        found = (at_ < keys.size) & (keys[np.minimum(at_, keys.size - 1)] == k) if keys.size else np.zeros(k.size, dtype=bool)
        sub = np.full(ok.shape, -1, dtype=np.int32)
        sub[ok] = np.where(found, at_, -1)
        inside[u], dist[u], idx[u] = ok, (y - x), sub
    return Lookup(inside, dist, idx)


def cell_values(cnt, b1, b2, weights):
    """v = ((double)count * w[bin1]) * w[bin2] of every cell: two multiplications in this order"""
    c = np.asarray(cnt, dtype=np.float64)
    if weights is None:
        return c
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (c * w[np.asarray(b1, dtype=np.int64)]) * w[np.asarray(b2, dtype=np.int64)]


def values(look, cnt, v, divisor, ignore_diags):
    """-> (kept bool, count int64, value float64) [n, S * S]; divisor: expected[d] / expected_smooth[d], or None for balanced.  An absent
    cell has count 0 and value 0.0."""
    kept = look.inside & (look.d >= ignore_diags)
    have = kept & (look.idx >= 0)
    at = look.idx[have]
    c = np.zeros(kept.shape, dtype=np.int64)
    c[have] = np.asarray(cnt, dtype=np.int64)[at]
    val = np.zeros(kept.shape, dtype=np.float64)
    x = np.asarray(v, dtype=np.float64)[at]
    if divisor is not None:
        x = x / np.asarray(divisor, dtype=np.float64)[look.d[have]]             # one IEEE division per cell
    val[have] = x
    return kept, c, val


def chunked(kept, c, val):
    """steps 4 and 5.  A value of 0.0 for an absent cell or a feature that is not used changes no bit: every T_c and vsum is >= +0.0."""
    n, S2 = kept.shape
    chunks = (n + CHUNK - 1) // CHUNK
    T = np.zeros((chunks, S2), dtype=np.float64)
    for s in range(CHUNK):                                                    # slot s of every chunk at once, the slots in ascending order
        rows = val[s::CHUNK]
        T[:rows.shape[0]] += rows
    vsum = np.zeros(S2, dtype=np.float64)
    for k in range(chunks):
        vsum += T[k]
    return kept.sum(axis=0).astype(np.uint64), c.sum(axis=0).astype(np.uint64), vsum


def _q(x):
    """a quotient as IEEE gives it (x / 0 is an infinity, 0 / 0 not a number); every NaN is the one quiet NaN"""
    return math.nan if x != x else float(x)


def _div(a, b):
    with np.errstate(all="ignore"):
        return _q(np.float64(a) / np.float64(b))


def _box(mean, rows, cols, skip=None, want_sd=False):
    total, k = 0.0, 0
    for p in rows:
        for q in cols:
            x = float(mean[p][q])
            if (p, q) != skip and math.isfinite(x):
                total += x
                k += 1
    mu = total / float(k) if k else math.nan
    if not want_sd:
        return mu
    ss = 0.0
    for p in rows:
        for q in cols:
            x = float(mean[p][q])
            if math.isfinite(x):
                dx = x - mu
                ss += dx * dx
    return mu, (math.sqrt(ss / float(k - 1)) if k >= 2 else math.nan)


def scores(mean, flank, corner):
    """step 6: mean [S, S] (index [p + flank][q + flank]) -> dict of the seven scores"""
    S = 2 * flank + 1
    low, high, every = range(0, corner), range(S - corner, S), range(S)
    peak = float(mean[flank][flank])
    ll, sd = _box(mean, high, low, want_sd=True)
    return dict(peak=_q(peak), p2ll=_div(peak, ll), p2ul=_div(peak, _box(mean, low, low)), p2ur=_div(peak, _box(mean, low, high)),
                p2lr=_div(peak, _box(mean, high, high)), p2m=_div(peak, _box(mean, every, every, skip=(flank, flank))), z_ll=_div(_q(peak - ll), sd))


def finish(n, csum, vsum, status, flank, corner):
    S = 2 * flank + 1
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, vsum / n.astype(np.float64), np.nan)
    shape = lambda x: x.reshape(S, S)
    return Result(shape(n), shape(csum), shape(vsum), shape(mean), status, scores(shape(mean), flank, corner))


def pileup(b1, b2, cnt, nbins, off, a, b, weights=None, expected=None, expected_smooth=None, **opts):
    """the whole definition.  weights None: every bin valid, w = 1; expected / expected_smooth: the genome-wide tables by distance."""
    o = dict(DEFAULTS)
    o.update(opts)
    assert set(o) == set(DEFAULTS) and o["kind"] in KINDS and 1 <= o["corner"] <= o["flank"] <= 32
    valid = np.ones(nbins, dtype=bool) if weights is None else ~np.isnan(np.asarray(weights, dtype=np.float64))
    st, lo, hi = statuses(a, b, off, nbins, o["flank"], o["edges"], o["min_dist"], o["max_dist"])
    look = lookup(b1, b2, nbins, a, b, st, lo, hi, valid, o["flank"])
    divisor = None if o["kind"] == "balanced" else expected if o["kind"] == "oe" else expected_smooth
    kept, c, val = values(look, cnt, cell_values(cnt, b1, b2, weights), divisor, o["ignore_diags"])
    return finish(*chunked(kept, c, val), st, o["flank"], o["corner"])
