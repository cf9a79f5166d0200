"""The loop-calling definition of include/mkt.h (mkt_matrix_loops) restated in plain numpy: the CHECKER of the GPU code.  Imports
nothing from the package under test.  Modelled on HiCCUPS (Rao et al. 2014); parity with juicer_tools is unpinned (it is not run).

  cells (bin1 <= bin2, count) of one resolution, nbins, the chromosomes' first bins `offsets`, weights or None (every bin valid,
  weight 1), E = the genome-wide expected_smooth of tests/expecteddef.py for the same weights; v = (count * w[bin1]) * w[bin2]
  1. candidate (i, j): one chromosome, both valid, min_dist <= j - i (<= max_dist when set); tested: every region defined, every r <= 512
  2. kept positions of an offset (a, b): (i + a, j + b) inside the chromosome, both valid, (j + b) - (i + a) >= 1; the regions
     DONUT / LL / H / V of a window w and a peak width p are what region_offsets() lists, in ascending (a, b)
  3. w = window; while Csum_LL(w) < min_ll_count and w < window_max: w += 1
  4. Bsum_R = sum of v over the stored cells at kept positions, Esum_R = sum of E[(j + b) - (i + a)] over all kept positions, both in
     ascending (a, b); undefined when Esum_R == 0 or nothing is kept; e_R = (Bsum_R / Esum_R) * E[j - i]; r_R = e_R / (w[i] * w[j])
  5. edge_k = ldexp(C[k % 3], k // 3), chunk_R = the smallest k with r_R <= edge_k; r_R > 512 (or NaN): status OVER
  6. H_R[k][x] = tested cells with chunk_R == k and min(count, 2047) == x
  7. T_R[k] from the Poisson tail of lambda = edge_k: thresholds()
  8. enriched: tested and count >= T_R[chunk_R] for all four R
  9. loops: components of the enriched cells of one chromosome linked within cluster_radius (Chebyshev); the peak is the largest count,
     ties to the smallest cell index; loops ascend by peak cell index

cells_pass() keeps one dense padded matrix per chromosome: it is a checker for test-sized inputs."""
import collections
import math

import numpy as np

C3 = (1.0, 1.2599210498948732, 1.5874010519681994)
NCHUNK, NCOL = 28, 2048
EDGES = np.array([math.ldexp(C3[k % 3], k // 3) for k in range(NCHUNK)], dtype=np.float64)
NONE, TESTED, UNDEFINED, OVER = 0, 1, 2, 3
NOCHUNK = 255
REGIONS = ("donut", "ll", "h", "v")
DEFAULTS = dict(peak=2, window=5, window_max=20, min_ll_count=16, min_dist=8, max_dist=0, fdr=0.1, cluster_radius=2)

Cells = collections.namedtuple("Cells", "status window chunk r e bsum esum kept csum_ll")
Loop = collections.namedtuple("Loop", "cell bin1 bin2 count window r n_cells box")


def options(**opts):
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise TypeError(f"loops: unknown option {k}")
        o[k] = v
    return o


def in_region(R, a, b, w, p):
    """is the offset (a, b) in region R (0 DONUT, 1 LL, 2 H, 3 V) of window w"""
    if max(abs(a), abs(b)) > w:
        return False
    if R == 0:
        return not (abs(a) <= p and abs(b) <= p) and a != 0 and b != 0
    if R == 1:
        return 1 <= a and b <= -1 and not (a <= p and b >= -p)
    if R == 2:
        return abs(a) <= 1 and p < abs(b)
    return p < abs(a) and abs(b) <= 1


def region_offsets(w, p):
    """the offsets of the four regions, each in ascending (a, b)"""
    return [[(a, b) for a in range(-w, w + 1) for b in range(-w, w + 1) if in_region(R, a, b, w, p)] for R in range(4)]


def cells_pass(bin1, bin2, count, nbins, offsets, E, weights=None, **opts):
    """steps 1 .. 5 -> Cells, one row per cell: status, window, chunk[4], r[4], e[4], bsum[4], esum[4], kept[4] (positions), csum_ll.
    A cell that is no candidate has window 0, chunks 255, NaN r and e, zeros elsewhere."""
    o = options(**opts)
    p, w0, wmax = o["peak"], o["window"], o["window_max"]
    b1 = np.asarray(bin1, dtype=np.int64)
    b2 = np.asarray(bin2, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.int64)
    off = np.asarray(list(offsets), dtype=np.int64)
    E = np.asarray(E, dtype=np.float64)
    n_c = np.diff(np.append(off, nbins))
    w = np.ones(nbins, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    valid = ~np.isnan(w)
    chrom = np.searchsorted(off, np.arange(nbins), side="right") - 1
    nnz = b1.size
    status = np.zeros(nnz, dtype=np.uint8)
    window = np.zeros(nnz, dtype=np.uint8)
    chunk = np.full((nnz, 4), NOCHUNK, dtype=np.uint8)
    r = np.full((nnz, 4), np.nan)
    e = np.full((nnz, 4), np.nan)
    bsum = np.zeros((nnz, 4))
    esum = np.zeros((nnz, 4))
    kept = np.zeros((nnz, 4), dtype=np.uint16)
    csum = np.zeros(nnz, dtype=np.uint64)
    if nnz == 0:
        return Cells(status, window, chunk, r, e, bsum, esum, kept, csum)
    d = b2 - b1
    cis = chrom[b1] == chrom[b2]
    cand = cis & valid[b1] & valid[b2] & (d >= o["min_dist"])
    if o["max_dist"]:
        cand &= d <= o["max_dist"]
    v = (cnt.astype(np.float64) * w[b1]) * w[b2]
    pad = wmax
    Epad = np.concatenate([E, np.zeros(2 * pad + 2)])                       # a distance past the table is never kept
    regions = {ww: region_offsets(ww, p) for ww in range(w0, wmax + 1)}
    for c in np.unique(chrom[b1[cand]]):
        n, lo = int(n_c[c]), int(off[c])
        inc = cis & (chrom[b1] == c)
        stored = inc & valid[b1] & valid[b2] & (d >= 1)                      # the stored cells that can sit at a kept position
        size = n + 2 * pad
        CNT = np.zeros((size, size), dtype=np.int64)
        V = np.zeros((size, size), dtype=np.float64)
        CNT[b1[stored] - lo + pad, b2[stored] - lo + pad] = cnt[stored]
        V[b1[stored] - lo + pad, b2[stored] - lo + pad] = v[stored]
        val = np.zeros(size, dtype=bool)
        val[pad:pad + n] = valid[lo:lo + n]
        idx = np.flatnonzero(cand & inc)
        I, J = b1[idx] - lo + pad, b2[idx] - lo + pad

        def keep(Is, Js, a, b):
            return val[Is + a] & val[Js + b] & ((Js + b) - (Is + a) >= 1)

        # step 3: the LL counts by ring m = max(a, -b), then the window
        ring = np.zeros((idx.size, wmax + 1), dtype=np.int64)
        for a in range(1, wmax + 1):
            for b in range(-wmax, 0):
                if a <= p and b >= -p:
                    continue
                ring[:, max(a, -b)] += np.where(keep(I, J, a, b), CNT[I + a, J + b], 0)
        cum = np.cumsum(ring, axis=1)
        wcell = np.full(idx.size, w0, dtype=np.int64)
        for ww in range(w0, wmax):
            grow = (wcell == ww) & (cum[:, ww] < o["min_ll_count"])
            wcell[grow] = ww + 1
        window[idx] = wcell
        csum[idx] = cum[np.arange(idx.size), wcell].astype(np.uint64)
        # step 4: the region sums in ascending (a, b)
        for ww in np.unique(wcell):
            sel = np.flatnonzero(wcell == ww)
            Is, Js, g = I[sel], J[sel], idx[sel]
            for R in range(4):
                bs = np.zeros(sel.size)
                es = np.zeros(sel.size)
                kp = np.zeros(sel.size, dtype=np.int64)
                for a, b in regions[int(ww)][R]:
                    k = keep(Is, Js, a, b)
                    bs = bs + np.where(k, V[Is + a, Js + b], 0.0)
                    es = es + np.where(k, Epad[np.maximum((Js + b) - (Is + a), 0)], 0.0)
                    kp += k
                bsum[g, R], esum[g, R], kept[g, R] = bs, es, kp
        ok = (kept[idx] > 0) & (esum[idx] != 0.0)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ee = (bsum[idx] / esum[idx]) * E[d[idx]][:, None]
            rr = ee / (w[b1[idx]] * w[b2[idx]])[:, None]
        ee[~ok] = np.nan
        rr[~ok] = np.nan
        e[idx], r[idx] = ee, rr
        with np.errstate(invalid="ignore"):
            fits = ok & (rr <= EDGES[-1])
        ch = np.searchsorted(EDGES, np.where(fits, rr, 0.0), side="left")    # the smallest k with r <= edge_k
        chunk[idx] = np.where(fits, ch, NOCHUNK).astype(np.uint8)
        status[idx] = np.where(~ok.all(axis=1), UNDEFINED, np.where(~fits.all(axis=1), OVER, TESTED)).astype(np.uint8)
    return Cells(status, window, chunk, r, e, bsum, esum, kept, csum)


def histogram(status, chunk, count):
    """step 6 -> uint64 [4][28][2048]"""
    H = np.zeros((4, NCHUNK, NCOL), dtype=np.uint64)
    t = np.asarray(status) == TESTED
    x = np.minimum(np.asarray(count, dtype=np.int64)[t], NCOL - 1)
    for R in range(4):
        np.add.at(H[R], (np.asarray(chunk)[t, R].astype(np.int64), x), 1)
    return H


def tail_table(k):
    """Q(x), x = 0 .. 2048, for lambda = edge_k: plain float arithmetic in the order of the definition"""
    lam = float(EDGES[k])
    pmf = math.exp(-lam)
    cdf = pmf
    Q = [1.0]
    for x in range(1, NCOL + 1):
        q = 1.0 - cdf
        Q.append(q if q > 0.0 else 0.0)
        pmf = (pmf * lam) / x
        cdf = cdf + pmf
    return Q


def thresholds(H, fdr):
    """step 7 -> uint32 [4][28]"""
    T = np.full((4, NCHUNK), NCOL, dtype=np.uint32)
    for k in range(NCHUNK):
        Q = tail_table(k)
        for R in range(4):
            h = [int(x) for x in H[R, k]]
            O = [0] * (NCOL + 1)
            for x in range(NCOL - 1, -1, -1):
                O[x] = O[x + 1] + h[x]
            n = float(O[0])
            for x in range(1, NCOL):
                if O[x] > 0 and n * Q[x] <= fdr * float(O[x]):
                    T[R, k] = x
                    break
    return T


def enriched(status, chunk, count, T):
    """step 8 -> bool per cell"""
    status, chunk, count = np.asarray(status), np.asarray(chunk), np.asarray(count, dtype=np.int64)
    en = status == TESTED
    ck = np.where(chunk < NCHUNK, chunk, 0).astype(np.int64)
    for R in range(4):
        en &= count >= np.asarray(T, dtype=np.int64)[R][ck[:, R]]
    return en


def loops(bin1, bin2, count, offsets, en, window, r, cluster_radius=2):
    """step 9 -> list of Loop, ascending by peak cell index"""
    b1, b2, cnt = (np.asarray(x, dtype=np.int64) for x in (bin1, bin2, count))
    off = np.asarray(list(offsets), dtype=np.int64)
    cells = np.flatnonzero(en)
    chrom = np.searchsorted(off, b1[cells], side="right") - 1
    at = {(int(b1[s]), int(b2[s])): t for t, s in enumerate(cells.tolist())}
    parent = list(range(cells.size))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for t, s in enumerate(cells.tolist()):
        for da in range(-cluster_radius, cluster_radius + 1):
            for db in range(-cluster_radius, cluster_radius + 1):
                u = at.get((int(b1[s]) + da, int(b2[s]) + db))
                if u is None or chrom[u] != chrom[t]:
                    continue
                ra, rb = find(t), find(u)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    comp = collections.OrderedDict()
    for t in range(cells.size):
        comp.setdefault(find(t), []).append(t)
    out = []
    for members in comp.values():
        ss = cells[members]
        peak = int(ss[np.argmax(cnt[ss])])                                  # argmax: the first of equal counts, i.e. the smallest cell index
        out.append(Loop(peak, int(b1[peak]), int(b2[peak]), int(cnt[peak]), int(window[peak]), tuple(float(x) for x in r[peak]), len(members),
                        (int(b1[ss].min()), int(b1[ss].max()), int(b2[ss].min()), int(b2[ss].max()))))
    return sorted(out, key=lambda L: L.cell)


def brute_cell(dense_count, valid, lo, hi, E, w, i, j, **opts):
    """steps 2 .. 5 of ONE candidate cell from a dense symmetric count matrix, position by position: the check of cells_pass itself.
    -> (window, csum_ll, bsum[4], esum[4], kept[4])"""
    o = options(**opts)
    p = o["peak"]

    def keep(a, b):
        x, y = i + a, j + b
        return lo <= x < hi and lo <= y < hi and bool(valid[x]) and bool(valid[y]) and y - x >= 1

    def csum_ll(ww):
        return sum(int(dense_count[i + a, j + b]) for a in range(-ww, ww + 1) for b in range(-ww, ww + 1) if in_region(1, a, b, ww, p) and keep(a, b))
    ww = o["window"]
    while csum_ll(ww) < o["min_ll_count"] and ww < o["window_max"]:
        ww += 1
    bs, es, kp = [0.0] * 4, [0.0] * 4, [0] * 4
    for R in range(4):
        for a in range(-ww, ww + 1):
            for b in range(-ww, ww + 1):
                if in_region(R, a, b, ww, p) and keep(a, b):
                    n = int(dense_count[i + a, j + b])
                    if n:
                        bs[R] += (float(n) * w[i + a]) * w[j + b]
                    es[R] += float(E[(j + b) - (i + a)])
                    kp[R] += 1
    return ww, csum_ll(ww), bs, es, kp
