"""The compartment-eigenvector definition of include/mkt.h (mkt_matrix_eigs) restated in plain numpy: the CHECKER of the GPU code.
Imports nothing from the package under test.  Modelled on cooltools `eigs-cis`; parity with cooltools and juicer_tools is unpinned
(neither is run).

  cells (bin1 <= bin2, count) of one resolution, nbins, the chromosomes' first bins `offsets`, weights or None (None: every bin valid,
  w = 1), E[d] = the genome-wide expected_smooth, v = (count * w[bin1]) * w[bin2]; options n_eigs, ignore_diags, clip, min_good
  1. good bin of chromosome c: valid, and one stored cell to a valid bin j of c with |j - k| >= ignore_diags; a chromosome with
     n_good < max(min_good, 9) is skipped
  2. A_c: for good i, j with |i - j| >= ignore_diags A[i][j] = oe - 1, oe = v / E[|i - j|] (min(oe, clip) when clip > 0) for a stored
     cell and 0 for an absent one; every other entry is 0.  A = S - (g g^T - B).
  3. the n_eigs eigenpairs largest in |lambda|, descending; unit 2-norm over the good bins, NaN elsewhere
  4. orientation: with a track p, flip when sum x_i (p_i - mean p) over the good bins with a value is negative; without one, or when
     that sum is 0 or empty, the entry of largest |x_i| (ties to the lowest bin) is made positive"""
import collections

import numpy as np

Chrom = collections.namedtuple("Chrom", "lo hi good skipped A S T")      # S: oe at the stored eligible positions; T: their number per row
U = 2.0 ** -52


def options(n_eigs=3, ignore_diags=2, min_good=9, max_iters=300, tol=1e-8, clip=0.0):
    return dict(n_eigs=n_eigs, ignore_diags=ignore_diags, min_good=min_good, max_iters=max_iters, tol=tol, clip=clip)


def chromosomes(bin1, bin2, count, nbins, offsets, E, weights=None, **opts):
    """-> one Chrom per chromosome: the dense A_c built entry by entry from the definition (local indices)"""
    o = options(**opts)
    ig, clip = o["ignore_diags"], o["clip"]
    b1, b2 = np.asarray(bin1, dtype=np.int64), np.asarray(bin2, dtype=np.int64)
    cnt = np.asarray(count, dtype=np.float64)
    w = np.ones(nbins) if weights is None else np.asarray(weights, dtype=np.float64)
    valid = ~np.isnan(w)
    bounds = list(offsets) + [nbins]
    out = []
    for c in range(len(offsets)):
        lo, hi = bounds[c], bounds[c + 1]
        n = hi - lo
        sel = (b1 >= lo) & (b2 < hi)                                     # bin1 <= bin2: both in c
        x, y, k = b1[sel] - lo, b2[sel] - lo, cnt[sel]
        ok = valid[b1[sel]] & valid[b2[sel]] & (y - x >= ig)
        good = np.zeros(n, dtype=bool)
        good[x[ok]] = True
        good[y[ok]] = True
        skipped = int(good.sum()) < max(o["min_good"], 9)
        S = np.zeros((n, n))
        stored = np.zeros((n, n), dtype=bool)
        for i, j, q, use in zip(x.tolist(), y.tolist(), k.tolist(), ok.tolist()):
            if not use or not (good[i] and good[j]):
                continue
            oe = ((q * w[lo + i]) * w[lo + j]) / E[j - i]
            if clip > 0 and oe > clip:
                oe = clip
            S[i, j] = S[j, i] = oe
            stored[i, j] = stored[j, i] = True
        A = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                if good[i] and good[j] and abs(i - j) >= ig:
                    A[i, j] = (S[i, j] if stored[i, j] else 0.0) - 1.0
        out.append(Chrom(lo, hi, good, skipped, A, S, stored.sum(axis=1)))
    return out


def apply(chroms, nbins, x, ignore_diags=2):
    """y = A x through the S - g g^T + B form; x: [nbins] or [nbins, ncols], treated as 0 on the bins that are not good; y is 0 there
    and on skipped chromosomes"""
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    for ch in chroms:
        if ch.skipped:
            continue
        g = ch.good
        xc = np.where(g.reshape((-1,) + (1,) * (x.ndim - 1)), x[ch.lo:ch.hi], 0.0)
        yc = ch.S @ xc - xc.sum(axis=0)
        n = ch.hi - ch.lo
        for i in range(n):
            yc[i] += xc[max(0, i - ignore_diags + 1):min(n, i + ignore_diags)].sum(axis=0)
        yc[~g] = 0.0
        y[ch.lo:ch.hi] = yc
    return y


def apply_bound(chroms, nbins, x, ignore_diags=2):
    """per entry (T_i + 2 ignore_diags + 3) 2^-52 (|A| |x|)_i: the reordering bound of the sums plus the three operations behind oe"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    b = np.zeros_like(x)
    for ch in chroms:
        if ch.skipped:
            continue
        xc = np.where(ch.good.reshape((-1,) + (1,) * (x.ndim - 1)), x[ch.lo:ch.hi], 0.0)
        t = (ch.T + 2 * ignore_diags + 3).astype(np.float64).reshape((-1,) + (1,) * (x.ndim - 1))
        b[ch.lo:ch.hi] = t * U * (np.abs(ch.A) @ xc)
    return b


def orient(x, good, track=None):
    """the orientation rule on one chromosome's vector (NaN outside good); returns the oriented copy"""
    x = x.copy()
    s = 0.0
    if track is not None:
        have = good & ~np.isnan(track)
        if have.any():
            s = float(np.sum(x[have] * (track[have] - track[have].mean())))
    if s != 0.0 and s == s:
        flip = s < 0
    else:
        a = np.where(good, np.abs(x), -1.0)
        flip = x[int(np.argmax(a))] < 0                                   # argmax: the first of equal values
    return -x if flip else x


def reference_eigs(ch, n_eigs, track=None):
    """(lambda [n_good] sorted by |lambda| descending, vectors [n_good columns, n_c] with NaN outside good, oriented) by numpy.linalg.eigh"""
    g = ch.good
    lam, vec = np.linalg.eigh(ch.A[np.ix_(g, g)])
    order = np.argsort(-np.abs(lam), kind="stable")
    lam, vec = lam[order], vec[:, order]
    out = np.full((min(n_eigs, lam.size), g.size), np.nan)
    for j in range(out.shape[0]):
        out[j, g] = vec[:, j]
        out[j] = orient(out[j], g, None if track is None else track[ch.lo:ch.hi])
    return lam, out


def x0_hash(i, col):
    x = (np.asarray(i, dtype=np.uint64) * 8 + col + 1) & 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
    return (x.astype(np.float64) + 0.5) / 2147483648.0 - 1.0


def block_iteration(ch, n_eigs=3, tol=1e-8, max_iters=300, **_):
    """The recommended procedure, plainly: a block of 8 hashed columns, one product per iteration, Rayleigh-Ritz on X^T Y, the residual
    columns Y S - X S Theta, the next X = orth(Y S).  -> (iterations, converged, lambda [n_eigs], vectors [n_eigs, n_c]).  Used only to
    certify inputs."""
    g = ch.good
    n = g.size
    X = np.stack([np.where(g, x0_hash(np.arange(n), c), 0.0) for c in range(8)], axis=1)
    X = X @ np.linalg.inv(np.linalg.cholesky(X.T @ X)).T
    lam, V = np.full(n_eigs, np.nan), np.full((n_eigs, n), np.nan)
    for it in range(1, max_iters + 1):
        Y = ch.A @ X
        H = X.T @ Y
        th, S = np.linalg.eigh((H + H.T) / 2)
        order = np.argsort(-np.abs(th), kind="stable")
        th, S = th[order], S[:, order]
        Vr, Z = X @ S, Y @ S
        R = Z - Vr * th
        res = np.linalg.norm(R, axis=0) / np.linalg.norm(Vr, axis=0)
        lam, V = th[:n_eigs], (Vr / np.linalg.norm(Vr, axis=0)).T[:n_eigs]
        if (res[:n_eigs] <= tol * abs(th[0])).all():
            return it, True, lam, V
        X = Z @ np.linalg.inv(np.linalg.cholesky(Z.T @ Z)).T
    return max_iters, False, lam, V
