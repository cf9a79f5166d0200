"""Inputs of the loop-calling tests, made once and shared (the callers leave them unchanged).  Imports nothing from the package under
test: the cells come from the matrix definition, the expected tables from tests/expecteddef.py."""
import functools

import numpy as np

import expected_inputs as xi
import matrixdef as md

R_EDGE = 1000
EDGE_BINS = [1, 12, 64, 65, 41]
MASKED_LOCAL = {2: (0, 63), 3: (0, 63, 64), 4: (20, 21, 22, 23, 24)}   # chromosome index -> bins left without a contact
# with the five bins of chromosome 4 masked, every LL row of LL_LOST (rows 20 .. 24 at window 5) is masked; LL_KEPT one row up keeps row 19
LL_LOST, LL_KEPT = (4, 19, 30), (4, 18, 30)              # (chromosome, local bin1, local bin2)


def table_of(nbins_per_chrom, r):
    rows = [(f"c{i}", n * r) for i, n in enumerate(nbins_per_chrom)]
    return rows, "".join(f"{n}\t{l}\n" for n, l in rows).encode(), [(n.encode(), l) for n, l in rows]


def text_of(rows, r, off, b1, b2, cnt):
    """.pairs text with cnt[k] lines for the cell (b1[k], b2[k])"""
    names = [n for n, _ in rows]
    offa = np.asarray(off)
    chrom = np.searchsorted(offa, np.arange(offa[-1] + rows[-1][1] // r + 1), side="right") - 1
    out = []
    for x, y, n in zip(np.asarray(b1).tolist(), np.asarray(b2).tolist(), np.asarray(cnt).tolist()):
        ca, cb = chrom[x], chrom[y]
        out.append(f"q\t{names[ca]}\t{(x - off[ca]) * r + 7}\t{names[cb]}\t{(y - off[cb]) * r + 9}\t+\t-\n" * n)
    return "".join(out).encode()


@functools.lru_cache(maxsize=None)
def edge_matrix(masked):
    """Chromosomes of 1, 12, 64, 65 and 41 bins at r = 1000 with nearly dense small integer counts (and a few trans cells).  masked:
    the bins of MASKED_LOCAL have no contact at all.  -> (table text, .pairs text, offsets, nbins, cells (k, 3), empty bins)"""
    rows, ttext, trows = table_of(EDGE_BINS, R_EDGE)
    off, nb = xi.offsets(R_EDGE, trows)
    rng = np.random.default_rng(31)
    empty = {off[c] + k for c, ks in MASKED_LOCAL.items() for k in ks} if masked else set()
    b1, b2, cnt = [], [], []
    for c, n in enumerate(EDGE_BINS):
        for x in range(n):
            for y in range(x, n):
                if rng.random() < 0.9 and not ({off[c] + x, off[c] + y} & empty):
                    b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(int(rng.integers(1, 5)))
    have = set(zip(b1, b2))
    for c, x, y in (LL_LOST, LL_KEPT):                                        # these two cells are there whatever the draw left out
        if (off[c] + x, off[c] + y) not in have:
            b1.append(off[c] + x); b2.append(off[c] + y); cnt.append(2)
    for _ in range(40):                                                       # trans cells: never candidates, never in a region
        x, y = sorted(rng.choice(nb, 2, replace=False).tolist())
        if not ({x, y} & empty) and np.searchsorted(off, x, side="right") != np.searchsorted(off, y, side="right"):
            b1.append(x); b2.append(y); cnt.append(1)
    text = text_of(rows, R_EDGE, off, b1, b2, cnt)
    cells = md.definition(ttext, [R_EDGE], text)[R_EDGE][0]
    bare = set(range(nb)) - set(cells[:, 0].tolist()) - set(cells[:, 1].tolist())     # the chosen bins, and any bin the draw left without a contact
    assert empty <= bare
    return ttext, text, off, nb, cells, bare


@functools.lru_cache(maxsize=None)
def band_matrix():
    """One chromosome of 400 bins: a band whose density falls with the distance, so that the LL count of a cell reaches min_ll_count at
    every window from 5 to 20 somewhere and nowhere at all further out; and one isolated cell with 3000 contacts far from the band."""
    rows, ttext, trows = table_of([400], R_EDGE)
    off, nb = xi.offsets(R_EDGE, trows)
    rng = np.random.default_rng(5)
    b1, b2, cnt = [], [], []
    for x in range(400):
        for y in range(x, min(400, x + 120)):
            lam = 6.0 / (1.0 + ((y - x) / 6.0) ** 2)
            n = int(rng.poisson(lam))
            if n:
                b1.append(x); b2.append(y); cnt.append(n)
    b1.append(40); b2.append(330); cnt.append(3000)
    for d in range(240, 335):                                                 # one contact on every diagonal around it, away from its neighbourhood: E > 0 there
        b1.append(65 + (7 * d) % (400 - d - 65)); b2.append(b1[-1] + d); cnt.append(1)
    text = text_of(rows, R_EDGE, off, b1, b2, cnt)
    cells = md.definition(ttext, [R_EDGE], text)[R_EDGE][0]
    return ttext, text, off, nb, cells


@functools.lru_cache(maxsize=None)
def flat_matrix(k):
    """One chromosome of 30 bins, every cell with exactly k contacts: E[d] = k and Bsum / Esum = 1 exactly, so r = k in every region"""
    rows, ttext, trows = table_of([30], R_EDGE)
    off, nb = xi.offsets(R_EDGE, trows)
    b1, b2 = np.triu_indices(30)
    text = text_of(rows, R_EDGE, off, b1, b2, np.full(b1.size, k))
    cells = np.stack([b1, b2, np.full(b1.size, k)], axis=1).astype(np.uint64)
    return ttext, text, off, nb, cells


# ---- the statistics input: a draw of expected_inputs.generate with planted loops -----------------------------------------------------
STAT_RES = (250000, 100000)
STAT_DRAW, STAT_SEED = 1_000_000, 77
STAT_PLANTS, STAT_EXTRA = 30, 120                          # pixels (chosen at 250 kb) and extra pairs on each
# One chromosome gets a dense background on top of the draw, so that the raw expected of its cells spans several chunks at both
# resolutions (the draw alone stays below edge_0 at 100 kb), and the first STAT_DENSE_PLANTS pixels lie there at different distances.
STAT_DENSE_CHROM, STAT_DENSE_PAIRS, STAT_DENSE_PLANTS = 13, 300_000, 6     # chr21
STAT_OPTS = dict(max_dist=48)


@functools.lru_cache(maxsize=None)
def planted():
    """(.pairs text, {r: cells (k, 3)}, the planted pixels at 250 kb as (bin1, bin2) global bins)"""
    ia, pa, ib, pb = xi.generate(STAT_DRAW, STAT_SEED)
    rng = np.random.default_rng(STAT_SEED + 1)
    L = np.array([l for _, l in xi.HG38], dtype=np.int64)
    big = np.flatnonzero(L > 60_000_000)
    off, nb = xi.offsets(250000)
    pix, ea, epa, epb = [], [], [], []
    Ld = int(L[STAT_DENSE_CHROM])
    da = 1 + (rng.random(STAT_DENSE_PAIRS) * Ld).astype(np.int64)
    db = np.clip(da + np.exp(rng.uniform(np.log(1e5), np.log(6e6), STAT_DENSE_PAIRS)).astype(np.int64) * rng.choice(np.array([-1, 1]), STAT_DENSE_PAIRS), 1, Ld)
    dc = np.full(STAT_DENSE_PAIRS, STAT_DENSE_CHROM)
    ia, pa, ib, pb = np.concatenate([ia, dc]), np.concatenate([pa, da]), np.concatenate([ib, dc]), np.concatenate([pb, db])
    while len(pix) < STAT_PLANTS:
        c = STAT_DENSE_CHROM if len(pix) < STAT_DENSE_PLANTS else int(rng.choice(big))
        n = -(-int(L[c]) // 250000)
        x = int(rng.integers(10, n - 30)) if c == STAT_DENSE_CHROM else int(rng.integers(30, n - 80))
        y = x + int(rng.integers(12, 20))                                 # 30 .. 47 bins at 100 kb: inside max_dist at both
        if any(cc == c and abs(x - xx) < 12 and abs(y - yy) < 12 for cc, xx, yy in pix):
            continue
        pix.append((c, x, y))
        # every extra pair inside the first 50 kb of the pixel on both sides: inside one 100 kb bin, so that the pixel is one cell at both resolutions
        ea.append(np.full(STAT_EXTRA, c))
        epa.append(x * 250000 + 1 + rng.integers(0, 50000, STAT_EXTRA))
        epb.append(y * 250000 + 1 + rng.integers(0, 50000, STAT_EXTRA))
    ea, epa, epb = np.concatenate(ea), np.concatenate(epa), np.concatenate(epb)
    ia, pa, ib, pb = np.concatenate([ia, ea]), np.concatenate([pa, epa]), np.concatenate([ib, ea]), np.concatenate([pb, epb])
    cells = {r: c for r, (c, _sk) in md.definition_arrays(xi.TROWS, list(STAT_RES), ia, pa, ib, pb).items()}
    pixels = {250000: [(off[c] + x, off[c] + y) for c, x, y in pix]}
    off1, _ = xi.offsets(100000)
    pixels[100000] = [(off1[c] + (x * 250000) // 100000, off1[c] + (y * 250000) // 100000) for c, x, y in pix]
    return xi.pairs_text(ia, pa, ib, pb), cells, pixels
