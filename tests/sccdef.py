"""The definition of the replicate comparison (mkt_matrix_scc of include/mkt.h: the stratum-adjusted correlation coefficient of two
binned contact matrices) restated in numpy, dense per chromosome.  The order of every floating-point addition is part of the
definition, so the library's results are compared with these as bytes.  Imports nothing from the package under test."""
import collections
import math

import numpy as np

CHUNK = 256
WEIGHT_N, WEIGHT_VAR = 0, 1
WEIGHTINGS = {"n": WEIGHT_N, "var": WEIGHT_VAR}
STRATA = ("n_cand", "n", "sx", "sy", "sxx", "syy", "sxy", "rho", "w")
CHROM = ("scc", "num", "den", "n_scored")
INTS = ("n_chrom", "strata", "candidates", "used", "scored", "count_a", "count_b")
FIELDS = STRATA + CHROM
Scc = collections.namedtuple("Scc", FIELDS + ("info",))
EPS = 2.0 ** -40


def chunk_tree(v):
    """the sum of step 5: chunks of 256 slots (the tail padded with 0.0), inside a chunk s[k] += s[k + half] for half = 128 .. 1,
    then the chunks in ascending order"""
    v = np.asarray(v, dtype=np.float64)
    nq = -(-v.size // CHUNK)
    if nq == 0:
        return 0.0
    s = np.zeros(nq * CHUNK, dtype=np.float64)
    s[:v.size] = v
    s = s.reshape(nq, CHUNK)
    half = CHUNK // 2
    while half >= 1:
        s = s[:, :half] + s[:, half:2 * half]
        half //= 2
    tot = s[0, 0]
    for q in range(1, nq):
        tot = tot + s[q, 0]
    return float(tot)


def joint_valid(nbins, weights_a, weights_b):
    """step 1: every bin without weights, else the bins whose weight is NaN in neither"""
    if weights_a is None:
        return np.ones(nbins, dtype=bool)
    return ~np.isnan(np.asarray(weights_a)) & ~np.isnan(np.asarray(weights_b))


def full_matrix(b1, b2, cnt, w, valid, lo, nc):
    """step 2: the symmetric dense matrix of the chromosome [lo, lo + nc)"""
    F = np.zeros((nc, nc), dtype=np.float64)
    b1, b2, cnt = (np.asarray(a).astype(np.int64) for a in (b1, b2, cnt))
    keep = (b1 >= lo) & (b2 < lo + nc) & (b2 >= b1)
    keep &= valid[np.clip(b1, 0, valid.size - 1)] & valid[np.clip(b2, 0, valid.size - 1)]
    i, j, c = b1[keep], b2[keep], cnt[keep].astype(np.float64)
    v = c if w is None else (c * np.asarray(w)[i]) * np.asarray(w)[j]
    F[i - lo, j - lo] = v
    F[j - lo, i - lo] = v
    return F


def smooth(F, valid_c, h):
    """step 3: the row pass left to right, the column pass in ascending row, the division by the valid bins of both windows"""
    nc = F.shape[0]
    Fp = np.zeros((nc, nc + 2 * h), dtype=np.float64)
    Fp[:, h:h + nc] = F
    R = Fp[:, 0:nc].copy()
    for t in range(1, 2 * h + 1):
        R = R + Fp[:, t:t + nc]
    Rp = np.zeros((nc + 2 * h, nc), dtype=np.float64)
    Rp[h:h + nc] = R
    W = Rp[0:nc].copy()
    for t in range(1, 2 * h + 1):
        W = W + Rp[t:t + nc]
    P = np.concatenate([[0], np.cumsum(valid_c.astype(np.int64))])
    k = np.arange(nc)
    nv = P[np.minimum(k + h, nc - 1) + 1] - P[np.maximum(k - h, 0)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return W / (nv[:, None] * nv[None, :]).astype(np.float64), nv


def score(n, sx, sy, sxx, syy, sxy, weighting, min_n):
    """step 6 -> (rho, w, scored)"""
    if n < min_n:
        return math.nan, 0.0, False
    nd = float(n)
    mx, my = sx / nd, sy / nd
    exx, eyy = sxx / nd, syy / nd
    vx, vy = exx - mx * mx, eyy - my * my
    cv = sxy / nd - mx * my
    if not (vx > EPS * exx) or not (vy > EPS * eyy):
        return math.nan, 0.0, False
    sd = math.sqrt(vx * vy)
    rho = cv / sd
    if rho != rho:
        rho = math.nan
    return rho, (nd * sd if weighting == WEIGHT_VAR else nd), True


def _div(a, b):
    if b == 0.0:
        r = math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    else:
        r = a / b
    return math.nan if r != r else r


def scc(cells_a, cells_b, nbins, off, h=5, min_diag=0, max_diag=0, weights_a=None, weights_b=None, weighting=WEIGHT_N, min_n=3, swap=False):
    """cells_*: (bin1, bin2, count) in the stored order; off: the first bin of every chromosome; weights_*: None (use_weights 0) or
    the weights of both (NaN = masked).  swap: the same with x and y exchanged (what scc(B, A) must give).  -> Scc"""
    weighting = WEIGHTINGS.get(weighting, weighting)
    off = [int(o) for o in off]
    nchr = len(off)
    ncs = [(off[c + 1] if c + 1 < nchr else nbins) - off[c] for c in range(nchr)]
    if max_diag == 0:
        max_diag = max(max(ncs), 1) - 1
    D = max_diag - min_diag + 1
    valid = joint_valid(nbins, weights_a, weights_b)
    rows = nchr * D
    out = {f: np.zeros(rows, dtype=np.uint64 if f in ("n_cand", "n") else np.float64) for f in STRATA}
    out["rho"][:] = np.nan
    ch = {f: np.zeros(nchr, dtype=np.uint64 if f == "n_scored" else np.float64) for f in CHROM}
    ch["scc"][:] = np.nan
    counts = [0, 0]
    num = den = 0.0
    scored = 0
    for c in range(nchr):
        lo, nc = off[c], ncs[c]
        vc = valid[lo:lo + nc]
        xy = []
        for side, (cells, w) in enumerate(((cells_a, weights_a), (cells_b, weights_b))):
            b1, b2, cnt = (np.asarray(a).astype(np.int64) for a in cells)
            F = full_matrix(b1, b2, cnt, w, valid, lo, nc)
            xy.append(smooth(F, vc, h)[0] if nc else F)
            cis = (b1 >= lo) & (b2 < lo + nc)
            cis &= valid[np.clip(b1, 0, nbins - 1)] & valid[np.clip(b2, 0, nbins - 1)] & (b2 - b1 >= min_diag) & (b2 - b1 <= max_diag)
            counts[side] += int(cnt[cis].sum())
        x, y = (xy[1], xy[0]) if swap else (xy[0], xy[1])
        num_c = den_c = 0.0
        for d in range(min_diag, max_diag + 1):
            at = c * D + d - min_diag
            if d < nc:
                i = np.arange(nc - d)
                xs, ys = x[i, i + d], y[i, i + d]
                cand = vc[i] & vc[i + d]
                with np.errstate(invalid="ignore"):
                    used = cand & ((xs != 0) | (ys != 0))
                xs, ys = np.where(used, xs, 0.0), np.where(used, ys, 0.0)
                out["n_cand"][at], out["n"][at] = int(cand.sum()), int(used.sum())
                for f, v in (("sx", xs), ("sy", ys), ("sxx", xs * xs), ("syy", ys * ys), ("sxy", xs * ys)):
                    out[f][at] = chunk_tree(v)
            rho, w, ok = score(int(out["n"][at]), *(float(out[f][at]) for f in ("sx", "sy", "sxx", "syy", "sxy")), weighting, min_n)
            out["rho"][at], out["w"][at] = rho, w
            if ok:
                num_c += w * rho
                den_c += w
                ch["n_scored"][c] += 1
        ch["num"][c], ch["den"][c] = num_c, den_c
        if ch["n_scored"][c]:
            ch["scc"][c] = _div(num_c, den_c)
        num += num_c
        den += den_c
        scored += int(ch["n_scored"][c])
    if swap:
        counts.reverse()
    info = dict(n_chrom=nchr, strata=D, candidates=int(out["n_cand"].sum()), used=int(out["n"].sum()), scored=scored, count_a=counts[0], count_b=counts[1],
                scc=_div(num, den) if scored else math.nan)
    return Scc(*[out[f] for f in STRATA], *[ch[f] for f in CHROM], info)
