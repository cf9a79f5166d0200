"""Inputs of the expected-table tests: the hg38 table and the pair generator of tests/test_gpu_balance.py (a copy: that file stays as
it is), and the cells of a draw by the matrix definition.  Imports nothing from the package under test."""
import functools
import math

import numpy as np

import matrixdef as md

HG38 = [("chr1", 248956422), ("chr10", 133797422), ("chr11", 135086622), ("chr12", 133275309), ("chr13", 114364328), ("chr14", 107043718),
        ("chr15", 101991189), ("chr16", 90338345), ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr2", 242193529),
        ("chr20", 64444167), ("chr21", 46709983), ("chr22", 50818468), ("chr3", 198295559), ("chr4", 190214555), ("chr5", 181538259),
        ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636), ("chr9", 138394717), ("chrM", 16569), ("chrX", 156040895),
        ("chrY", 57227415)]
TABLE = "".join(f"{n}\t{l}\n" for n, l in HG38).encode()
TROWS = [(n.encode(), l) for n, l in HG38]


def generate(n_draw, seed):
    """Pairs inside the tabulated lengths, two thirds cis with log-uniform distances from 1 kb to 50 Mb, thinned by a visibility factor
    per 250 kb bin (uniform in [0.3, 1], about 3 % of the bins at 0.01) on both sides: (ia, pa, ib, pb) of the kept pairs."""
    rng = np.random.default_rng(seed)
    L = np.array([l for _, l in HG38], dtype=np.int64)
    w = L / L.sum()
    ia = rng.choice(len(L), size=n_draw, p=w)
    ib = np.where(rng.random(n_draw) < 0.67, ia, rng.choice(len(L), size=n_draw, p=w))
    pa = np.minimum(1 + (rng.random(n_draw) * L[ia]).astype(np.int64), L[ia])
    dist = np.exp(rng.uniform(math.log(1e3), math.log(5e7), size=n_draw)).astype(np.int64) * rng.choice(np.array([-1, 1]), size=n_draw)
    near = np.clip(pa + dist, 1, L[ia])
    far = np.minimum(1 + (rng.random(n_draw) * L[ib]).astype(np.int64), L[ib])
    pb = np.where(ia == ib, near, far)
    off, _, nb = md.bin_layout(TROWS, 250000)
    off = np.array(off, dtype=np.int64)
    vis = rng.uniform(0.3, 1.0, size=nb)
    vis[rng.random(nb) < 0.03] = 0.01
    keep = rng.random(n_draw) < vis[off[ia] + (pa - 1) // 250000] * vis[off[ib] + (pb - 1) // 250000]
    return ia[keep], pa[keep], ib[keep], pb[keep]


def pairs_text(ia, pa, ib, pb, table=HG38):
    names = [nm for nm, _ in table]
    return "".join(f"q\t{names[a]}\t{p}\t{names[b]}\t{q}\t+\t-\n" for a, p, b, q in zip(ia.tolist(), pa.tolist(), ib.tolist(), pb.tolist())).encode()


@functools.lru_cache(maxsize=None)
def drawn(n_draw, seed, resolutions):
    """(.pairs text, {r: cells (k, 3) uint64}, pairs) of one draw; computed once and shared: the callers leave it unchanged"""
    ia, pa, ib, pb = generate(n_draw, seed)
    cells = {r: c for r, (c, _sk) in md.definition_arrays(TROWS, list(resolutions), ia, pa, ib, pb).items()}
    return pairs_text(ia, pa, ib, pb), cells, ia.size


def offsets(r, table=TROWS):
    off, _, nb = md.bin_layout(table, r)
    return off, nb
