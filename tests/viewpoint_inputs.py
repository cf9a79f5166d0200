"""Seeded .pairs text for the viewpoint profiles (tests/golden/viewpoint_golden.json stores only the parameters and the expected
texts; the inputs are made again here at test time).  Every pair of a golden case is one the matrix stage accepts: a chromosome of
the table, a position in 1 .. length."""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "viewpoint_golden.json")

VIEWPOINT = "chrEBV"
PARTNER_RE = r"chr\d+$"
# a partner regex keeps chr1, chr2, chr10 and xchr7 (the match is unanchored at its start) and leaves out the other four
TABLE = [("chr1", 3500000), ("chr2", 2400000), ("chr10", 1300000), ("chrX", 900000), ("chrM", 16569), ("chr1_KI270706v1_random", 175055),
         ("xchr7", 800000), ("chrEBV", 20000)]
KEPT = ["chr1", "chr2", "chr10", "xchr7"]
LEFT_OUT = ["chrX", "chrM", "chr1_KI270706v1_random"]


def table_text(table=TABLE):
    return "".join(f"{n}\t{l}\n" for n, l in table).encode()


def _line(rid, c1, p1, c2, p2):
    return f"r{rid}\t{c1}\t{p1}\t{c2}\t{p2}\t+\t-\n"


def _edge_positions(size, length):
    """1, the length, and k * size - 1, k * size, k * size + 1 for a few k, inside 1 .. length"""
    out = {1, length}
    for k in (1, 2, 3, 7, 10, 11, length // size):
        for d in (-1, 0, 1):
            p = k * size + d
            if 1 <= p <= length:
                out.add(p)
    return sorted(out)


def _noise(rng, n, lens):
    """pairs the reference's rule leaves out: the viewpoint on the first side, viewpoint with viewpoint, partners the regex excludes,
    pairs without the viewpoint"""
    rows = []
    names = list(lens)
    for _ in range(n):
        kind = rng.randrange(5)
        if kind == 0:                                                              # the viewpoint first: only second_side_only = 0 sees it
            c = rng.choice(KEPT)
            rows.append((VIEWPOINT, rng.randint(1, lens[VIEWPOINT]), c, rng.randint(1, lens[c])))
        elif kind == 1:
            rows.append((VIEWPOINT, rng.randint(1, lens[VIEWPOINT]), VIEWPOINT, rng.randint(1, lens[VIEWPOINT])))
        elif kind == 2:
            c = rng.choice(LEFT_OUT)
            rows.append((c, rng.randint(1, lens[c]), VIEWPOINT, rng.randint(1, lens[VIEWPOINT])))
        elif kind == 3:
            c = rng.choice(LEFT_OUT)
            rows.append((VIEWPOINT, rng.randint(1, lens[VIEWPOINT]), c, rng.randint(1, lens[c])))
        else:
            a, b = rng.choice(names[:-1]), rng.choice(names[:-1])
            rows.append((a, rng.randint(1, lens[a]), b, rng.randint(1, lens[b])))
    return rows


def _cells_rows(cells):
    """[(partner, partner position, viewpoint position, count)] -> that many pairs each, partner first"""
    rows = []
    for c, pp, vp, k in cells:
        rows += [(c, pp, VIEWPOINT, vp)] * k
    return rows


def make(gen):
    """the .pairs text of a case from its generator parameters (a dict that JSON holds): bytes"""
    rng = random.Random(gen["seed"])
    lens = dict(TABLE)
    vbin, pbin = gen["vbin"], gen["pbin"]
    kind = gen["kind"]
    rows = []
    if kind == "random":                                                           # hot spots on both sides, so that counts pile up
        vhot = [rng.randint(1, lens[VIEWPOINT]) for _ in range(12)]
        phot = [(c, rng.randint(1, lens[c])) for c in KEPT for _ in range(4)]
        for _ in range(gen["n"]):
            c, pp = rng.choice(phot) if rng.random() < 0.8 else (lambda c: (c, rng.randint(1, lens[c])))(rng.choice(KEPT))
            vp = rng.choice(vhot) if rng.random() < 0.8 else rng.randint(1, lens[VIEWPOINT])
            rows.append((c, min(lens[c], pp + rng.randrange(3)), VIEWPOINT, min(lens[VIEWPOINT], vp + rng.randrange(3))))
    elif kind == "edges":                                                          # every edge position of one side against a few of the other
        ve = _edge_positions(vbin, lens[VIEWPOINT])
        for c in KEPT:
            pe = _edge_positions(pbin, lens[c])
            for vp in ve:
                for pp in rng.sample(pe, 3):
                    rows += [(c, pp, VIEWPOINT, vp)] * rng.randint(1, 3)
            for pp in pe:
                for vp in rng.sample(ve, 2):
                    rows += [(c, pp, VIEWPOINT, vp)] * rng.randint(1, 3)
    elif kind == "pow2":                                                           # counts 2^k - 1, 2^k, 2^k + 1, each in a cell of its own
        counts = sorted({(1 << k) + d for k in range(gen["kmax"] + 1) for d in (-1, 0, 1)} - {0})
        slots = [(c, j) for c in KEPT for j in range(lens[c] // pbin)]
        vslots = list(range(lens[VIEWPOINT] // vbin))
        used = rng.sample([(s, v) for s in slots for v in vslots], len(counts))
        cells = [(c, j * pbin + rng.randrange(pbin), max(1, v * vbin + rng.randrange(vbin)), k) for ((c, j), v), k in zip(used, counts)]
        rows = _cells_rows([(c, max(1, pp), vp, k) for c, pp, vp, k in cells])
    elif kind == "counts":                                                         # the counts given, each in a cell of its own
        slots = [(c, j) for c in KEPT for j in range(lens[c] // pbin)]
        vslots = list(range(10, lens[VIEWPOINT] // vbin))
        used = rng.sample([(s, v) for s in slots for v in vslots], len(gen["counts"]))
        rows = _cells_rows([(c, j * pbin + 1 + rng.randrange(pbin - 1), v * vbin + 1 + rng.randrange(vbin - 1), k) for ((c, j), v), k in zip(used, gen["counts"])])
    else:
        raise ValueError(kind)
    rows += _noise(rng, gen.get("noise", 0), lens)
    rng.shuffle(rows)
    out = ["## pairs format v1.0\n", "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"]
    for i, r in enumerate(rows):
        out.append(_line(i, *r))
        if i % 997 == 500:
            out.append("#a comment in the middle\n")
    return "".join(out).encode()


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# the cases of the golden file: name, generator, the scripts' arguments (vbin, pbin, ratio for the first; track bin, min count for the second)
CASE_PARAMS = [
    dict(name="defaults", gen=dict(kind="random", seed=11, n=3000, noise=600, vbin=200, pbin=1000000), vbin=200, pbin=1000000, ratio=0.01, track_bin=1000, min_count=5),
    dict(name="edges", gen=dict(kind="edges", seed=12, noise=300, vbin=333, pbin=7000), vbin=333, pbin=7000, ratio=0.5, track_bin=7000, min_count=2),
    dict(name="edges_track", gen=dict(kind="edges", seed=13, noise=100, vbin=150, pbin=1300), vbin=150, pbin=1300, ratio=0.99, track_bin=1300, min_count=1),
    dict(name="pow2", gen=dict(kind="pow2", seed=14, kmax=12, noise=200, vbin=250, pbin=100000), vbin=250, pbin=100000, ratio=0.99, track_bin=100000, min_count=4),
    # (the cut of the case above leaves only counts of 64 and more in the links text; this one shows the thickness of 4 .. 65)
    dict(name="pow2_low", gen=dict(kind="pow2", seed=18, kmax=6, noise=100, vbin=250, pbin=100000), vbin=250, pbin=100000, ratio=0.99, track_bin=100000, min_count=1),
    # 30 + 20 = 50 = int(100 * 0.5): the sum EQUALS the cutoff at 20, the walk goes on to 10 and min_loop is 11
    dict(name="exact_cutoff", gen=dict(kind="counts", seed=15, counts=[30, 20, 10, 10, 10, 10, 10], noise=50, vbin=200, pbin=100000), vbin=200, pbin=100000, ratio=0.5, track_bin=1000, min_count=5),
    # the largest count alone passes the cutoff: min_loop = 51 is clipped to 50
    dict(name="clipped", gen=dict(kind="counts", seed=16, counts=[50, 3, 2, 1, 1, 1, 1, 1], noise=50, vbin=200, pbin=100000), vbin=200, pbin=100000, ratio=0.01, track_bin=1000, min_count=1),
    dict(name="half", gen=dict(kind="random", seed=17, n=2500, noise=400, vbin=170, pbin=250000), vbin=170, pbin=250000, ratio=0.5, track_bin=500, min_count=3),
]
