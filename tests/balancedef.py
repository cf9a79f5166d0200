"""The balancing definition of include/mkt.h (mkt_matrix_balance) restated in plain numpy: the CHECKER of the GPU code.
Imports nothing from the package under test.  Parity with cooler's `balance` is unpinned (cooler is not run).

  cells (bin1 <= bin2, count) of one resolution, nbins, the chromosomes' first bins `offsets`; float64 throughout.
  1. used cells: bin2 - bin1 >= ignore_diags; marg(x)[k] = sum of x over used cells with bin1 == k + the same with bin2 == k
  2. bias = 1; min_nnz > 0: bias = 0 where marg(1) < min_nnz; m = marg(count * bias[bin1] * bias[bin2]);
     min_count > 0: bias = 0 where m < min_count
  3. mad_max > 0: per chromosome range m /= median(m[m > 0]) (none: left alone); lg = log(m[m > 0]);
     cut = exp(median(lg) - mad_max * median(|lg - median(lg)|)); bias = 0 where m < cut
  4. it = 1 .. max_iters: m = marg(count * bias[bin1] * bias[bin2]); nz = m[m != 0]; empty: all NaN, stop, not converged;
     mean = mean(nz); var = var(nz) / mean; m /= mean; m[m == 0] = 1; bias /= m; var < tol: converged, stop
  5. weight = bias / sqrt(mean), NaN where bias == 0"""
import collections

import numpy as np

DEFAULTS = dict(ignore_diags=2, min_nnz=10, min_count=0, mad_max=5.0, tol=1e-5, max_iters=200)
Result = collections.namedtuple("Result", "weights iterations converged var scale masked variances cut filter_marg longest_row")


def _marg(b1, b2, x, nbins):
    return np.bincount(b1, weights=x, minlength=nbins) + np.bincount(b2, weights=x, minlength=nbins)


def balance(bin1, bin2, count, nbins, offsets, **opts):
    """-> Result: weights float64[nbins]; iterations, converged, var, scale, masked: the stats; variances: var of every
    iteration; cut and filter_marg: step 3's threshold and the normalised marginals it was compared with (None / the step-2
    marginals when mad_max == 0); longest_row: the most used cells any bin's marginal sums (row and column together)."""
    o = dict(DEFAULTS)
    for k in opts:
        if k not in o:
            raise TypeError(k)
    o.update(opts)
    b1 = np.asarray(bin1, dtype=np.int64)
    b2 = np.asarray(bin2, dtype=np.int64)
    c = np.asarray(count, dtype=np.float64)
    used = (b2 - b1) >= o["ignore_diags"]
    b1, b2, c = b1[used], b2[used], c[used]
    ones = np.ones(b1.size, dtype=np.float64)
    nnz_marg = _marg(b1, b2, ones, nbins)
    longest = int(nnz_marg.max()) if nbins else 0
    bias = np.ones(nbins, dtype=np.float64)
    if o["min_nnz"] > 0:
        bias[nnz_marg < o["min_nnz"]] = 0.0
    m = _marg(b1, b2, c * bias[b1] * bias[b2], nbins)
    if o["min_count"] > 0:
        bias[m < o["min_count"]] = 0.0
    cut = None
    if o["mad_max"] > 0:
        m = m.copy()
        bounds = list(offsets) + [nbins]
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            seg = m[lo:hi]
            pos = seg[seg > 0]
            if pos.size:
                m[lo:hi] = seg / np.median(pos)
        pos = m[m > 0]
        if pos.size:
            lg = np.log(pos)
            med = np.median(lg)
            cut = float(np.exp(med - o["mad_max"] * np.median(np.abs(lg - med))))
            bias[m < cut] = 0.0
    filter_marg = m
    variances = []
    converged = False
    mean = var = float("nan")
    iterations = 0
    empty = False
    for it in range(1, o["max_iters"] + 1):
        iterations = it
        m = _marg(b1, b2, c * bias[b1] * bias[b2], nbins)
        nz = m[m != 0]
        if nz.size == 0:
            empty = True
            mean = var = float("nan")
            break
        mean = float(nz.mean())
        var = float(nz.var() / mean)
        variances.append(var)
        m = m / mean
        m[m == 0] = 1.0
        bias = bias / m
        if var < o["tol"]:
            converged = True
            break
    if empty:
        weights = np.full(nbins, np.nan)
    else:
        weights = bias / np.sqrt(mean)
        weights[bias == 0] = np.nan
    return Result(weights, iterations, converged, var, mean, int(np.isnan(weights).sum()), variances, cut, filter_marg, longest)


def balanced_marginals(bin1, bin2, count, nbins, weights, ignore_diags=2):
    """marg(count * weight[bin1] * weight[bin2]) with NaN weights read as 0: the property a balanced matrix has is that these are
    all 1 (to tol) on the unmasked bins"""
    b1 = np.asarray(bin1, dtype=np.int64)
    b2 = np.asarray(bin2, dtype=np.int64)
    used = (b2 - b1) >= ignore_diags
    w = np.nan_to_num(np.asarray(weights, dtype=np.float64), nan=0.0)
    return _marg(b1[used], b2[used], np.asarray(count, dtype=np.float64)[used] * w[b1[used]] * w[b2[used]], nbins)
