"""Seeded pairs of .pairs texts for the pair-level concordance (tests/golden/paircmp_golden.json stores only the parameters and what
the reference's benchmarking/check.consistency.pl printed for them; the inputs are made again here at test time).  Every line of a
golden case is inside the pinned domain: at least five fields, positions decimal in [0, 2^31)."""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "paircmp_golden.json")
CHUNK = 1 << 16                                   # the line index works on chunks of this many bytes


def line(rid, c1, p1, c2, p2, tail="+\t-"):
    return f"{rid}\t{c1}\t{p1}\t{c2}\t{p2}" + ("\t" + tail if tail is not None else "") + "\n"


def _dist_edges(gen, rng):
    """each of the four coordinates off by D - 1, D, D + 1 (both signs), straight and swapped; cis pairs that only the swap saves"""
    D = gen["D"]
    a, b = [], []
    base = ("chr1", 100000, "chr2", 500000)
    k = 0
    for coord in range(4):
        for delta in (D - 1, D, D + 1):
            for sign in (1, -1):
                for swapped in (False, True):
                    p = [base[1], base[3]]
                    c = [base[0], base[2]]
                    if coord < 2:
                        p[coord] += sign * delta                       # a position moves
                    elif delta == D:
                        c[coord - 2] = c[coord - 2] + "x"              # a name differs, the positions agree
                    rid = f"e{k}"
                    k += 1
                    a.append(line(rid, *base))
                    rec = (c[1], p[1], c[0], p[0]) if swapped else (c[0], p[0], c[1], p[1])
                    b.append(line(rid, *rec))
    for both in ((D - 1, D - 1), (D, D - 1), (D - 1, D), (D, D), (D + 1, 0)):       # both positions off at once
        rid = f"e{k}"
        k += 1
        a.append(line(rid, *base))
        b.append(line(rid, base[0], base[1] + both[0], base[2], base[3] - both[1]))
    for gap in (D, D + 1, 3 * D + 7):                                  # one chromosome: straight fails on p1, the swap passes
        rid = f"s{gap}"
        a.append(line(rid, "chr3", 1000, "chr3", 1000 + gap))
        b.append(line(rid, "chr3", 1000 + gap, "chr3", 1000))
        rid = f"t{gap}"                                                # the issue's example scaled: only |a.p2 - b.p1| = D - 1 and |a.p1 - b.p2| < D
        a.append(line(rid, "chr3", 10, "chr3", 10 + min(10, D - 1)))
        b.append(line(rid, "chr3", 10 + min(10, D - 1) + D - 1, "chr3", 10 + min(10, D - 1)))
    return a, b


def _distribution(gen, rng):
    """d at the class edges, trans by a last byte, and per-class counts that print as 0, 3e-06, 1.2e-05 and 0.001234"""
    a, b = [], []
    k = 0
    for d in (0, 999, 1000, 10000, 10001):
        for flip in (False, True):
            p1, p2 = (5000000, 5000000 + d) if not flip else (5000000 + d, 5000000)
            a.append(line(f"d{k}", "chr1", p1, "chr1", p2))
            b.append(line(f"d{k}", "chr1", p2, "chr1", p1))
            k += 1
    a.append(line("tr1", "chr1a", 5, "chr1b", 5))
    b.append(line("tr1", "chr1b", 5, "chr1a", 5))
    # both sides end with 12 cis<1K and 1234 cis>10K lines (the same ones, so they leave no inconsistent text), side A with 3 trans
    # lines; nothing is discordant, so that count prints as 0
    for cls, d, n in (("lt", 10, 12 - 4), ("gt", 20000, 1234 - 2)):
        for _ in range(n):
            a.append(line(f"f{k}", "chr2", 100 + k, "chr2", 100 + k + d, tail=None))
            b.append(a[-1])
            k += 1
    a += [line("tr2", "chr1", 5, "chr10", 5), line("tr3", "chr10", 5, "chr1", 5)]
    return a, b


def _repeats(gen, rng):
    a, b = [], []
    v = ("chr1", 1000, "chr2", 2000)
    far = ("chr1", 9000, "chr2", 2000)
    a += [line("twice", *far), line("only_a1", *v), line("twice", *v)]                           # the last one decides
    a += [line("thrice", *v), line("thrice", *far), line("x", *v), line("thrice", *v)]
    a += [line("twice_bad", *v), line("twice_bad", *far)]                                       # ... also when it is the wrong one
    a += [line("b2_cons", *v), line("b2_disc", *v), line("only_a2", "chr1", 1, "chr1", 50000)]
    b += [line("twice", *v), line("thrice", *v), line("twice_bad", *v), line("only_b1", *v)]
    b += [line("b2_cons", *v), line("b2_cons", *v), line("b2_disc", *far), line("b2_disc", *v)]  # the second is B-only either way
    b += [line("only_b2", *far), line("x", *v), line("x", *v), line("x", *far)]
    return a, b


def _hot(gen, rng):
    """one id n times on each side: A's last value meets B's first line, everything else is superseded or B-only"""
    n = gen["n"]
    a = [line("h", "c", 1 + (k % 7), "c", 2) for k in range(n)] + [line("z", "c", 1, "c", 2, tail=None)]
    b = [line("q", "c", 1, "d", 2, tail=None)] + [line("h", "c", 1 + (k % 5), "c", 2) for k in range(n)]
    return a, b


def _one_side(gen, rng):
    rows = [line(f"r{k}", "chr1", 100 * k, "chr2" if k % 3 else "chr1", 100 * k + 1500 * (k % 9)) for k in range(gen["n"])]
    which = gen["which"]
    return (rows if "a" in which else []), (rows if "b" in which else [])


def _ids(gen, rng):
    """prefixes, long common heads, the lengths around the 64-byte steps, ids across a chunk boundary of the line index"""
    a, b = [], []
    v = ("chr1", 1000, "chr2", 2000)
    w = ("chr1", 7000, "chr2", 2000)
    ids = ["p", "pr", "pre", "prefix", "prefix:1", "prefix:10"]
    for n in (64, 128):
        head = "".join(rng.choice("ACGT:0123456789") for _ in range(n))
        ids += [head + "a", head + "b", head]
    ids += ["".join(rng.choice("abcdefgh") for _ in range(n)) for n in (1, 63, 64, 65, 300)]
    for k, rid in enumerate(ids):                                    # neighbours in the id order get different answers
        a.append(line(rid, *v))
        b.append(line(rid, *(v if k % 2 else w)))
    rng.shuffle(b)
    # filler up to just before the chunk boundary, then ids of 40 and 300 bytes that cross it (A's text starts the joined text)
    def pad_to(rows, at, tag):                                      # (the filler goes to B as well: consistent, so no inconsistent text)
        size = sum(len(r) for r in rows)
        k = 0
        while size < at - 400:
            r = line(f"{tag}{k}", "chr5", 10 * k, "chr5", 10 * k + 100)
            rows.append(r)
            b.append(r)
            size += len(r)
            k += 1
        return size
    for n, cross in ((40, 1), (300, 2)):
        size = pad_to(a, cross * CHUNK, f"fa{cross}_")
        m = cross * CHUNK - n // 2 - size - 12                       # one line that ends n / 2 bytes before the boundary ...
        a.append("pad" + "y" * m + "\tc\t1\tc\t2\n")
        b.append(a[-1])
        rid = "X" * n + str(cross)                                   # ... so this id lies across it
        a.append(line(rid, *v))
        b.append(line(rid, *w))
        b.append(line("X" * n + "9", *v))
    return a, b


def _lines(gen, rng):
    """comment lines, field counts, extreme positions, leading zeros; the last line of both sides has no newline"""
    top = (1 << 31) - 1
    a = ["## pairs format v1.0\n", "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"]
    b = ["#only one header line here\n"]
    a += [line("five", "chr1", 10, "chr1", 20, tail=None), line("many", "chr1", 10, "chr2", 20, tail="+\t-\textra\tfields\t1\t2\t3")]
    b += [line("five", "chr1", 10, "chr1", 20, tail="+\t-\tmore"), line("many", "chr1", 10, "chr2", 20, tail=None)]
    a += ["#a comment in the middle of A\n", line("zero", "chr1", 0, "chr1", top), line("top", "chrX", top, "chrY", 0)]
    b += [line("zero", "chr1", 0, "chr1", top - 200), line("#an_id_like_this_is_a_comment", "chr1", 1, "chr1", 2), "#middle of B\n", line("top", "chrY", 199, "chrX", top - 199)]
    a += [line("lead", "chr1", "007", "chr1", "0000000000012"), line("lead2", "chr2", "00", "chr2", "010")]
    b += [line("lead", "chr1", "0300", "chr1", "12"), line("lead3", "chr2", "00", "chr2", "010")]
    a += [line("empty_tail", "chr1", 5, "chr1", 6, tail=""), "#last comment of A\n", line("last", "chr9", 1, "chr9", 2, tail=None)[:-1]]
    b += [line("empty_tail", "chr1", 5, "chr1", 6), line("last", "chr9", 1, "chr9", 900, tail=None), "#the last line of B is a comment without a newline"]
    return a, b


def _mixed(gen, rng):
    """n reads through two imagined pipelines: most agree, some moved, some swapped, some lost on either side, some repeated"""
    n = gen["n"]
    chroms = [f"chr{k}" for k in range(1, 23)] + ["chrX", "chrUn_KI270742v1"]
    a, b = [], []
    for k in range(n):
        rid = f"K84:{rng.randrange(1, 9)}:{rng.randrange(1101, 2229)}:{k}"
        c1 = rng.choice(chroms)
        c2 = c1 if rng.random() < 0.7 else rng.choice(chroms)
        p1 = rng.randrange(1, 200000000)
        p2 = p1 + rng.choice((rng.randrange(0, 1000), rng.randrange(1000, 10001), rng.randrange(10001, 5000000))) if c1 == c2 else rng.randrange(1, 200000000)
        s = rng.choice(("+\t-", "-\t+", "+\t+", "-\t-"))
        u = rng.random()
        ra = line(rid, c1, p1, c2, p2, s)
        if u < 0.985:
            j1, j2 = rng.randrange(-150, 151), rng.randrange(-150, 151)
            rb = line(rid, c2, max(0, p2 + j2), c1, max(0, p1 + j1), s) if rng.random() < 0.3 else line(rid, c1, max(0, p1 + j1), c2, max(0, p2 + j2), s)
        elif u < 0.989:
            rb = line(rid, c1, p1 + rng.choice((199, 200, 201, 5000)), c2, p2, s)
        elif u < 0.991:
            rb = line(rid, rng.choice(chroms), p1, c2, p2, s)
        elif u < 0.994:
            rb = None
        elif u < 0.997:
            rb, ra = ra, None
        else:
            rb = ra
            a.append(line(rid, c1, p1 + 100000, c2, p2, s))          # an earlier, superseded value
            b.append(ra)                                             # and the id twice in B
        if ra:
            a.append(ra)
        if rb:
            b.append(rb)
    rng.shuffle(b)
    a.insert(0, "## pairs format v1.0\n")
    b.insert(len(b) // 2, "#a comment in the middle\n")
    return a, b


KINDS = {"dist_edges": _dist_edges, "distribution": _distribution, "repeats": _repeats, "hot": _hot, "one_side": _one_side, "ids": _ids, "lines": _lines, "mixed": _mixed}


def make(gen):
    """(text A, text B) of a case from its generator parameters (a dict that JSON holds): bytes"""
    rng = random.Random(gen["seed"])
    a, b = KINDS[gen["kind"]](gen, rng)
    return "".join(a).encode(), "".join(b).encode()


def cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# the cases of the golden file: name, generator, the script's third argument (None: not given)
CASE_PARAMS = [
    dict(name="dist_1", gen=dict(kind="dist_edges", seed=1, D=1), dist="1"),
    dict(name="dist_200", gen=dict(kind="dist_edges", seed=2, D=200), dist=None),
    dict(name="dist_500", gen=dict(kind="dist_edges", seed=3, D=500), dist="500"),
    dict(name="dist_0_is_200", gen=dict(kind="dist_edges", seed=2, D=200), dist="0"),
    dict(name="dist_200_at_500", gen=dict(kind="dist_edges", seed=2, D=200), dist="500"),
    dict(name="distribution", gen=dict(kind="distribution", seed=4), dist=None),
    dict(name="repeats", gen=dict(kind="repeats", seed=5), dist=None),
    dict(name="hot", gen=dict(kind="hot", seed=6, n=50), dist=None),
    dict(name="only_a", gen=dict(kind="one_side", seed=7, n=40, which="a"), dist=None),
    dict(name="only_b", gen=dict(kind="one_side", seed=8, n=40, which="b"), dist=None),
    dict(name="both_empty", gen=dict(kind="one_side", seed=9, n=0, which="ab"), dist=None),
    dict(name="same_file", gen=dict(kind="one_side", seed=10, n=300, which="ab"), dist=None),
    dict(name="ids", gen=dict(kind="ids", seed=11), dist=None),
    dict(name="lines", gen=dict(kind="lines", seed=12), dist=None),
    dict(name="mixed", gen=dict(kind="mixed", seed=13, n=20000), dist=None),
]

# cases that only the definition checks (their inconsistent text would be most of the golden file): one id 5 000 times on each side
EXTRA_PARAMS = [
    dict(name="hot_5000", gen=dict(kind="hot", seed=6, n=5000), dist=None),
]
