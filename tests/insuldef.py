"""The insulation definition of include/mkt.h (mkt_matrix_insulation) restated in numpy: dense, brute force per bin, every floating-point
sum in ascending (a, b).  Imports nothing from the package under test.  Steps 1 .. 3 are `sums` and `score`, step 4 `normalise`,
steps 5 .. 7 `call`; `insulation` runs them all."""
import collections
import math

import numpy as np

DEFAULTS = dict(ignore_diags=2, min_frac_valid=0.66, min_strength=0.2)
Sums = collections.namedtuple("Sums", "n_valid csum bsum stored")          # [K, nbins]; stored: stored cells at kept positions (P of the bounds)
Result = collections.namedtuple("Result", "n_valid csum bsum stored score log2_score strength boundary minima")


def bounds_of(off, nbins):
    return list(off) + [nbins]


def n_full(window, ignore_diags):
    return sum(1 for p in range(window) for q in range(window) if p + q >= ignore_diags)


def dense(b1, b2, cnt, nbins):
    """the upper triangle as a dense int64 matrix"""
    C = np.zeros((nbins, nbins), dtype=np.int64)
    C[np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)] = np.asarray(cnt, dtype=np.int64)
    return C


def sums(b1, b2, cnt, nbins, off, windows, weights=None, ignore_diags=2):
    """steps 1 and 2.  weights None: every bin valid, w = 1."""
    C = dense(b1, b2, cnt, nbins)
    valid = np.ones(nbins, dtype=bool) if weights is None else ~np.isnan(weights)
    w = np.ones(nbins) if weights is None else np.asarray(weights, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        V = (C.astype(np.float64) * w[:, None]) * w[None, :]                 # two multiplications in this order
    K = len(windows)
    nv, cs, st = (np.zeros((K, nbins), dtype=np.uint64) for _ in range(3))
    bs = np.zeros((K, nbins), dtype=np.float64)
    bnd = bounds_of(off, nbins)
    for c in range(len(off)):
        lo, hi = bnd[c], bnd[c + 1]
        for i in range(lo, hi):
            for k, W in enumerate(windows):
                a0, b1_ = max(lo, i - W + 1), min(i + W, hi)
                a, b = np.arange(a0, i + 1), np.arange(i, b1_)
                keep = (((i - a)[:, None] + (b - i)[None, :]) >= ignore_diags) & valid[a][:, None] & valid[b][None, :]
                blockC = C[a0:i + 1, i:b1_]
                nv[k, i] = int(keep.sum())
                cs[k, i] = int(blockC[keep].sum())
                st[k, i] = int((blockC[keep] > 0).sum())
                terms = np.where(keep & (blockC > 0), V[a0:i + 1, i:b1_], 0.0).ravel()      # row-major: ascending (a, b); an absent cell adds 0
                bs[k, i] = np.cumsum(terms)[-1] if terms.size else 0.0      # cumsum adds one after the other
    return Sums(nv, cs, bs, st)


def score(n_valid, bsum, windows, ignore_diags=2, min_frac_valid=0.66):
    """step 3"""
    out = np.full(bsum.shape, np.nan)
    for k, W in enumerate(windows):
        nf = n_full(W, ignore_diags)
        for i in range(bsum.shape[1]):
            n = int(n_valid[k, i])
            if nf == 0 or n == 0 or float(n) < min_frac_valid * float(nf):
                continue
            out[k, i] = bsum[k, i] / float(n)
    return out


def normalise(sc, off, nbins):
    """step 4 for one window: score[nbins] -> L[nbins]"""
    L = np.full(nbins, np.nan)
    bnd = bounds_of(off, nbins)
    for c in range(len(off)):
        lo, hi = bnd[c], bnd[c + 1]
        total, n = 0.0, 0
        for i in range(lo, hi):
            x = float(sc[i])
            if math.isfinite(x) and x > 0:
                total += x
                n += 1
        if n == 0:
            continue
        mean = total / float(n)
        for i in range(lo, hi):
            x = float(sc[i])
            if x != x or x == 0.0:
                continue
            y = x / mean
            L[i] = math.log2(y) if 0 < y < math.inf else math.inf if y == math.inf else -math.inf if y == 0 else math.nan
    return L


def call(L, off, nbins, min_strength=0.2):
    """steps 5 .. 7 for one window: L[nbins] -> (strength, boundary, minima)"""
    strength = np.full(nbins, np.nan)
    boundary, minima = np.zeros(nbins, dtype=bool), np.zeros(nbins, dtype=bool)
    bnd = bounds_of(off, nbins)
    fin = np.isfinite(L)
    for c in range(len(off)):
        lo, hi = bnd[c], bnd[c + 1]
        s0 = lo
        while s0 < hi:
            if not fin[s0]:
                s0 += 1
                continue
            e0 = s0
            while e0 + 1 < hi and fin[e0 + 1]:
                e0 += 1
            s = s0
            while s <= e0:
                x = L[s]
                e = s
                while e < e0 and L[e + 1] == x:
                    e += 1
                if s > s0 and e < e0 and L[s - 1] > x and L[e + 1] > x:
                    lm, j = -math.inf, s - 1
                    while j >= s0 and L[j] >= x:
                        lm = max(lm, L[j])
                        j -= 1
                    rm, j = -math.inf, e + 1
                    while j <= e0 and L[j] >= x:
                        rm = max(rm, L[j])
                        j += 1
                    strength[s] = min(lm, rm) - x
                    minima[s] = True
                    boundary[s] = strength[s] >= min_strength
                s = e + 1
            s0 = e0 + 1
    return strength, boundary, minima


def insulation(b1, b2, cnt, nbins, off, windows, weights=None, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    S = sums(b1, b2, cnt, nbins, off, windows, weights, o["ignore_diags"])
    sc = score(S.n_valid, S.bsum, windows, o["ignore_diags"], o["min_frac_valid"])
    K = len(windows)
    L, st = np.full((K, nbins), np.nan), np.full((K, nbins), np.nan)
    bd, mn = np.zeros((K, nbins), dtype=bool), np.zeros((K, nbins), dtype=bool)
    for k in range(K):
        L[k] = normalise(sc[k], off, nbins)
        st[k], bd[k], mn[k] = call(L[k], off, nbins, o["min_strength"])
    return Result(S.n_valid, S.csum, S.bsum, S.stored, sc, L, st, bd, mn)
