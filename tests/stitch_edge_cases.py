"""Directed inputs for the read stitcher at its word, lane, tie and threshold edges, and for each family of them the classes it must
reach.  Plain Python / numpy: nothing here needs a GPU or the program.  A family is a seeded list of cases (name, text, kwargs) --
kwargs as stitchdef.stitch takes them -- and a coverage function that works out, from the definition only (stitchdef.candidates /
choose, never from GPU output), that the family reaches what it was written for; a family that misses a class fails
tests/test_stitch_edges_host.py.  The texts and the definition's results are made once per process and never modified.

What the kernels (mkt_stitch.hip) do at these places: a pair is packed in 64-bit words of 32 bases (17 words), a candidate's overlap
is read through a funnel shift of two neighbouring words and masked in its last, partial word; the candidates are dealt to the 64
lanes in rounds (candidate index c = offset - max(0, n1 - n2), round c // 64, up to 8 rounds); ties in the mismatch density are
broken by a second scan and a cross-lane minimum over (quality sum, scored length, c); the tag scan is another 64-lane loop.
"""
from fractions import Fraction

import numpy as np

import stitchdef as sd

FAMILIES = ("length_grid", "deciding_position", "quality_ties", "parameters", "tags")
LENGTHS = (10, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 255, 256, 257, 319, 320, 321, 479, 480, 481,
           510, 511, 512)
_NEXT = {65: 67, 67: 71, 71: 84, 84: 65}      # A -> C -> G -> T -> A
_cache = {}


# ---- building blocks
def rnd_seq(R, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[R.randint(0, 4, size=n)].tobytes()


def rc(s):
    return bytes(s).translate(sd._COMP)[::-1]


def quals(R, n, phred=33, lo=2, hi=41):
    return (phred + R.randint(lo, hi + 1, size=n)).astype(np.uint8).tobytes()


def record(h1, s1, q1, s2, q2, h2=None):
    """one pair; the headers are given without '@'"""
    return b"@%s\n%s\n+\n%s\n@%s\n%s\n+\n%s\n" % (h1, bytes(s1), bytes(q1), h1 if h2 is None else h2, bytes(s2), bytes(q2))


def planted(R, n1, n2, ov):
    """-> (read 1, the reverse-complemented read 2) as bytearrays, cut from one random fragment so that the last ov bases of read 1
    are the first ov of the other: offset n1 - ov.  Position j of the overlap is s1[n1 - ov + j] and r2[j]."""
    f = rnd_seq(R, n1 + n2 - ov)
    return bytearray(f[:n1]), bytearray(f[n1 - ov:])


def differ(s, positions):
    for p in positions:
        s[p] = _NEXT[s[p]]


def take_pairs(text, index):
    """the pairs of a text whose numbers are in index, in that order"""
    lines = text.split(b"\n")
    return b"".join(b"\n".join(lines[8 * k:8 * k + 8]) + b"\n" for k in index)


def flash_args(kw):
    """a case's kwargs as the program's (and bin/stitch's) options"""
    return ["-m", str(kw.get("m", 10)), "-M", str(kw.get("M", 150)), "-x", repr(float(kw.get("x", 0.25))), "-p", str(kw.get("phred", 33))]


def family(name):
    """-> (cases, meta): cases = [(case name, text, kwargs)]; meta = {case name: [per pair, what the builder planted]}"""
    if name not in _cache:
        _cache[name] = globals()["_build_" + name]()
    return _cache[name]


def cases(name):
    return family(name)[0]


def definition(name):
    """{case name: stitchdef.stitch's result}, made once"""
    key = ("def", name)
    if key not in _cache:
        _cache[key] = {c: sd.stitch(text, **kw) for c, text, kw in cases(name)}
    return _cache[key]


def scored(name):
    """{case name: [(parsed pair, candidates, chosen offset)]} by the plain loops of stitchdef.candidates / choose, made once"""
    key = ("scored", name)
    if key not in _cache:
        out = {}
        for c, text, kw in cases(name):
            m, M, x, phred = kw.get("m", 10), kw.get("M", 150), kw.get("x", 0.25), kw.get("phred", 33)
            rows = []
            for p in sd.parse(text, phred):
                cand = sd.candidates(p, m, M, phred)
                rows.append((p, cand, sd.choose(cand, m, M, x)))
            out[c] = rows
        _cache[key] = out
    return _cache[key]


def _cidx(pair, off):
    return off - max(0, len(pair[1]) - len(pair[3]))


# ---- length_grid
def _build_length_grid():
    """Pairs cut from one random fragment with a planted overlap, n1 and n2 from LENGTHS (every word count, every partial last word
    one below, at and one above a word or lane-round boundary, up to the limit of 512).  Default arguments, and the same text again
    with -M 255."""
    R = np.random.RandomState(4101)
    S = LENGTHS
    T = []                                                    # (n1, n2, overlap or 0 for unrelated reads)
    for k, a in enumerate(S):                                 # every length as n1 and as n2
        b = S[(7 * k + 3) % len(S)]
        T.append((a, b, int(R.randint(10, min(a, b) + 1))))
        b = S[(11 * k + 5) % len(S)]
        T.append((b, a, int(R.randint(10, min(a, b) + 1))))
    for r in range(32):                                       # every residue of the offset mod 32, at 256 or more
        off = 256 + r + 32 * (r % 6)
        n1 = (512, 511, 510, 481)[r % 4]
        ov = n1 - off
        T.append((n1, int(R.choice([s for s in S if s >= ov])), ov))
    for r in range(8):                                        # every round of the candidate loop: its first and last lane, one between
        for e in (0, 63, 17 + r):
            c = 64 * r + e
            if c <= 502:
                T.append((512, 512, 512 - c))
            if c <= 310:
                T.append((512, 320, 320 - c))                 # read 1 longer: the first candidate is offset 192
                T.append((320, 512, 320 - c))
    T += [(512, 512, 512), (512, 512, 10), (512, 300, 11), (300, 512, 300), (511, 257, 33), (193, 481, 64), (512, 512, 256),
          (512, 300, 300), (481, 321, 321), (481, 321, 200), (321, 481, 200), (512, 257, 10), (257, 512, 10)]
    for k in range(12):                                       # unrelated reads
        T.append((S[(5 * k + 19) % len(S)], S[(3 * k + 22) % len(S)], 0))
    recs, meta = [], []
    for k, (n1, n2, ov) in enumerate(T):
        if ov:
            s1, r2 = planted(R, n1, n2, ov)
            rate = 0.0 if ov < 64 else (0.0, 0.02, 0.05)[k % 3]
            differ(r2, [j for j in range(ov) if R.rand() < rate])
            if ov >= 64 and k % 5 == 0:
                for j in R.randint(0, ov, size=2):
                    (s1 if k % 10 == 0 else r2)[(n1 - ov + j) if k % 10 == 0 else j] = ord("N")
        else:
            s1, r2 = bytearray(rnd_seq(R, n1)), bytearray(rnd_seq(R, n2))
        recs.append(record(b"lg%d/1" % k, s1, quals(R, n1), rc(r2), quals(R, n2), b"lg%d/2" % k))
        meta.append(dict(n1=n1, n2=n2, ov=ov))
    text = b"".join(recs)
    return [("length_grid", text, {}), ("length_grid_M255", text, dict(M=255))], {"length_grid": meta, "length_grid_M255": meta}


def cover_length_grid():
    """Asserts the classes of the issue from the definition's chosen offsets (default arguments); returns them."""
    rows = scored("length_grid")["length_grid"]
    comb = [(len(p[1]), len(p[3]), off, _cidx(p, off)) for p, _c, off in rows if off >= 0]
    assert 0 < len(comb) < len(rows) <= 400
    assert {n1 for n1, _n2, _o, _c in comb} >= set(LENGTHS) and {n2 for _n1, n2, _o, _c in comb} >= set(LENGTHS)
    assert {o % 32 for _n1, _n2, o, _c in comb if o >= 256} == set(range(32))
    cs = {c for _n1, _n2, _o, c in comb}
    for r in range(8):
        assert any(c // 64 == r for c in cs), r
        assert 64 * r in cs, r
        assert 64 * r + 63 > 502 or 64 * r + 63 in cs, r
    assert any(n1 == 512 and n1 - o == 10 and c == 502 for n1, _n2, o, c in comb)
    assert any(n1 == 512 and c == 0 for n1, _n2, _o, c in comb)
    big = [(n1, n2, o) for n1, n2, o, _c in comb if n1 > 256 and n2 > 256]
    assert any(n1 > n2 for n1, n2, _o in big) and any(n1 < n2 for n1, n2, _o in big)
    assert any(n1 > n2 and o == n1 - n2 for n1, n2, o in big)                      # read 2 wholly inside read 1
    return dict(pairs=len(rows), combined=len(comb), candidate_indices=len(cs))


# ---- deciding_position
def _dp_positions(L):
    return sorted({0, 31, 32, 63, 64, L - 1} | {p for t in range(1, L // 32 + 1) for p in (32 * t - 1, 32 * t) if p < L})


def _dp_fixed(L, thr):
    """thr places of the overlap, all = 2 mod 4 (so none is a multiple of 32, the one before, or L - 1), spread over its words"""
    pos = [2 + 4 * ((k * (L // 4)) // thr) for k in range(thr)]
    assert len(set(pos)) == thr and max(pos) < L - 1
    return pos


def _build_deciding_position():
    """x = 0.25, M = 150.  An overlap of L bases carries exactly thr[min(L, M)] mismatches at fixed places: combined.  One more at
    position p -- the first and last position of every packed word, and L - 1 -- and it is not; a kernel that misses the bit at p
    combines it.  Form A: both reads L long (offset 0, no funnel shift); form B: 37 more bases before the overlap in read 1 and 50
    behind it in read 2 (offset 37: every word of read 1 comes through the shift).  For L = 128 also one N at p, in read 1 or in
    read 2: 127 called positions allow 31 mismatches where 128 allow 32."""
    recs, meta = [], []
    for L in (128, 150, 151, 256, 512):
        thr = sd.threshold(min(L, 150), 0.25)
        fixed = _dp_fixed(L, thr)
        for form, pre, post in (("A", 0, 0), ("B", 37, 50)):
            if L + max(pre, post) > sd.MAX_READ:
                continue
            R = np.random.RandomState(4200 + 2 * L + (form == "B"))
            f = rnd_seq(R, pre + L + post)
            q1, q2 = quals(R, pre + L), quals(R, L + post)

            def add(kind, p=None, read=0, expect=pre):
                s1, r2 = bytearray(f[:pre + L]), bytearray(f[pre:])
                differ(r2, fixed)
                assert p is None or p not in fixed
                if kind == "mm":
                    differ(s1 if read == 1 else r2, [pre + p if read == 1 else p])
                elif kind == "n":
                    (s1 if read == 1 else r2)[pre + p if read == 1 else p] = ord("N")
                name = b"dp_L%d_%s_%s" % (L, form.encode(), kind.encode()) + (b"_p%d_r%d" % (p, read) if p is not None else b"")
                recs.append(record(name + b"/1", s1, q1, rc(r2), q2, name + b"/2"))
                meta.append(dict(L=L, form=form, kind=kind, p=p, read=read, expect=expect, thr=thr))

            add("base")
            for k, p in enumerate(_dp_positions(L)):
                add("mm", p, 1 + (k + (form == "B")) % 2, expect=-1)
            if L == 128:
                for p in _dp_positions(L):
                    for read in (1, 2):
                        add("n", p, read, expect=-1)
    return [("deciding_position", b"".join(recs), {})], {"deciding_position": meta}


def cover_deciding_position():
    rows, meta = scored("deciding_position")["deciding_position"], family("deciding_position")[1]["deciding_position"]
    assert len(rows) == len(meta) <= 400
    seen = set()
    for (p, cand, off), me in zip(rows, meta):
        assert off == me["expect"], (p[0], off)
        at = next(c for c in cand if c[0] == (len(p[1]) - me["L"]))       # the planted candidate
        if me["kind"] == "base":
            assert (at[1], at[2]) == (me["L"], me["thr"])
        elif me["kind"] == "mm":
            assert (at[1], at[2]) == (me["L"], me["thr"] + 1)
        else:
            assert (at[1], at[2]) == (127, 32) and sd.threshold(127, 0.25) == 31 and sd.threshold(128, 0.25) == 32
        seen.add((me["L"], me["form"], me["kind"], me["p"]))
    for L in (128, 150, 151, 256, 512):
        for form in ("A", "B") if L < 512 else ("A",):
            assert (L, form, "base", None) in seen and all((L, form, "mm", p) in seen for p in _dp_positions(L))
    assert {p for L, _f, k, p in seen if L == 512 and k == "mm"} >= {0, 31, 32, 479, 480, 511}
    return dict(pairs=len(rows))


# ---- quality_ties
def _build_quality_ties():
    """Tandem repeats of unit length 1 .. 6: every offset that is a multiple of the unit matches.  A mismatch that lies in every
    candidate's overlap (in the last bases of read 1, or the first of the reverse-complemented read 2) gives all of them the same
    count, so every candidate with the same scored length ties in the density and the position-dependent qualities decide:
      quality_ties      default arguments: the candidates of 150 bases or more tie (sl = min(eff, 150)), up to c = 362
      quality_ties_M10  -m 10 -M 10: sl = 10 for every candidate, so all of them tie, up to c = 502
      quality_ties_M255 -M 255, poly-A with mismatches at positions 5, 100 and 200 of read 2: exactly the overlaps of 100 (1 / 100)
                        and 200 bases (2 / 200) tie with DIFFERENT scored lengths; the quality sums are set so that the later wins
                        (10 / 100 < 30 / 200), the earlier stays though its raw sum is larger (20 / 100 > 30 / 200), or both tie
    With constant qualities the sums tie too and the earliest candidate wins; so it does in the 512 x 512 homopolymer (503 tied
    candidates without a mismatch)."""
    def pair(R, name, u, n1, n2, win, style, nmis=1, const=False):
        unit = rnd_seq(R, u)
        while u > 1 and len(set(unit)) == 1:
            unit = rnd_seq(R, u)
        rep = unit * (sd.MAX_READ // u + 2)
        s1, r2 = bytearray(rep[:n1]), bytearray(rep[:n2])
        i = -(-(win + max(0, n1 - n2)) // u) * u              # the winner: the first multiple of the unit at or after candidate `win`
        assert i <= n1 - 10
        qa, qb = bytearray([33 + 40]) * n1, bytearray([33 + 40]) * n2
        if style == 1:                                        # mismatches in the last bases of read 1; read 2's qualities decide
            ps = [n1 - 2 - 3 * k for k in range(nmis)]
            differ(s1, ps)
            if not const:
                for j in range(n2):
                    qb[j] = 33 + 10 + (7 * j) % 23
                for p in ps:
                    qb[p - i] = 33 + 2
        else:                                                 # mismatches in the first bases of read 2; read 1's qualities decide
            js = [1 + 4 * k for k in range(nmis)]
            differ(r2, js)
            if not const:
                for p in range(n1):
                    qa[p] = 33 + 10 + (5 * p) % 29
                for j in js:
                    qa[i + j] = 33 + 2
        return record(name + b"/1", s1, qa, rc(r2), bytes(qb)[::-1], name + b"/2"), dict(u=u, want=i, const=const)

    R = np.random.RandomState(4301)
    out, metas = [], {}
    for case, kw, rounds in (("quality_ties", {}, 6), ("quality_ties_M10", dict(m=10, M=10), 8)):
        recs, meta = [], []
        for u in range(1, 7):
            for r in range(rounds):
                n1, n2 = ((512, 512), (511, 512), (480, 512), (512, 449))[(u + r) % 4] if r < 4 else (512, 512)
                e = (63 if r % 2 else 0) if u == 1 else (0, 57, 20, 33, 41, 50)[u - 1]      # the lane; rounding up to the unit adds 5 at most
                if r == rounds - 1:                           # the last round that still holds tied candidates is a short one
                    e = min(e, 30)
                rec, me = pair(R, b"%s_u%d_r%d" % (case.encode(), u, r), u, n1, n2, 64 * r + e, 1 + (u + r) % 2, nmis=1 + (r % 2))
                recs.append(rec)
                meta.append(me)
        for k, (u, n1, n2) in enumerate(((1, 512, 512), (2, 300, 400), (3, 512, 200), (5, 257, 257), (6, 512, 511), (4, 400, 400))):
            rec, me = pair(R, b"%s_const%d" % (case.encode(), k), u, n1, n2, 0, 1 + k % 2, const=True)
            recs.append(rec)
            meta.append(me)
        if case == "quality_ties":
            recs.append(record(b"homopolymer512/1", b"A" * 512, quals(R, 512), b"T" * 512, quals(R, 512), b"homopolymer512/2"))
            meta.append(dict(u=1, want=0, const=True))
        out.append((case, b"".join(recs), kw))
        metas[case] = meta
    recs, meta = [], []
    for k, (q100, qa200, qb200, want) in enumerate(((10, 15, 15, 100), (20, 15, 15, 200), (15, 10, 20, 200), (5, 30, 30, 100), (31, 30, 31, 200),
                                                    (8, 9, 8, 100), (9, 9, 8, 200))):      # (..., the overlap that wins)
        n = 300
        s1, r2 = bytearray(b"A" * n), bytearray(b"A" * n)
        differ(r2, (5, 100, 200))
        qa = bytearray([33 + 35]) * n
        qa[n - 95], qa[n - 195], qa[n - 100] = 33 + q100, 33 + qa200, 33 + qb200
        recs.append(record(b"cross_sl%d/1" % k, s1, qa, rc(r2), bytes([33 + 40]) * n, b"cross_sl%d/2" % k))
        meta.append(dict(u=1, want=want, const=False, cross=True))
    out.append(("quality_ties_M255", b"".join(recs), dict(M=255)))
    metas["quality_ties_M255"] = meta
    return out, metas


def tie_facts(cand, m, M):
    """Of one pair's candidates: ([(offset, sl, mm, mq)] of those that share the minimal density, their quality scores mq / sl),
    both compared as exact fractions (test_stitch.py shows that float32 orders them the same way up to MAX_M)"""
    live = [(i, min(eff, M), mm, mq) for i, eff, mm, mq in cand if eff >= m]
    if not live:
        return [], []
    d = min(Fraction(c[2], c[1]) for c in live)
    tied = [c for c in live if Fraction(c[2], c[1]) == d]
    return tied, [Fraction(c[3], c[1]) for c in tied]


def cover_quality_ties():
    decided, rounds, same, cross = 0, set(), 0, 0
    for case, _text, kw in cases("quality_ties"):
        m, M = kw.get("m", 10), kw.get("M", 150)
        for (p, cand, off), me in zip(scored("quality_ties")[case], family("quality_ties")[1][case]):
            tied, qs = tie_facts(cand, m, M)
            assert off >= 0 and off in [c[0] for c in tied], p[0]
            if not me["const"] and not me.get("cross"):
                assert off == me["want"], (p[0], off, me["want"])
            if len(tied) >= 2 and len(set(qs)) > 1 and off != tied[0][0]:
                decided += 1
                rounds.add(_cidx(p, off) // 64)
                cross += len({c[1] for c in tied}) > 1
            elif len(tied) >= 2 and len(set(qs)) == 1:
                assert off == tied[0][0]
                same += 1
            if me.get("cross"):
                assert [c[0] for c in tied] == [100, 200] and [c[1] for c in tied] == [200, 100] and off == 300 - me["want"], p[0]
            if p[0] == b"homopolymer512":
                assert len(tied) == 503 and all(c[2] == 0 for c in tied) and off == 0
    assert decided >= 20 and rounds == set(range(8)) and same >= 5 and cross >= 2, (decided, rounds, same, cross)
    big = [_cidx(p, off) for rows in scored("quality_ties").values() for p, _c, off in rows]
    assert max(big) >= 448
    return dict(decided_by_quality=decided, rounds=sorted(rounds), quality_ties_too=same, different_scored_lengths=cross)


# ---- parameters
PHREDS = (33, 64)
MIN_MAX = ((1, 1), (1, 255), (10, 255), (255, 255), (150, 150))
DENSITIES = (0, 0.1, 0.2, 0.25, 0.3, 0.3333333, 0.5, 1)


def _build_parameters():
    """One case per (phred_offset, (m, M), x).  Each holds overlaps of M - 1, M and M + 1 bases (the min(eff, M) cap from below,
    at and above) with exactly thr and thr + 1 mismatches, thr = the float32 threshold for the scored length, as whole reads
    (offset 0) and 7 bases into read 1.  The qualities take every value from 0 to 93 above the offset of 33, and to 62 above 64:
    the program reads a byte above 126 as a negative character and refuses it as "under phred_offset", while the C ABI and the
    definition accept offset + 93 for any offset; those bytes (157 for offset 64) are compared with the definition alone, in
    tests/test_gpu_stitch_edges.py::test_quality_bounds."""
    out, metas = [], {}
    for phred in PHREDS:
        top = min(93, 126 - phred)
        for m, M in MIN_MAX:
            for x in DENSITIES:
                case = "p%d_m%d_M%d_x%s" % (phred, m, M, x)
                R = np.random.RandomState(4400 + phred + 7 * m + 11 * M + int(1000 * x))
                recs, meta = [], []
                for s in (M - 1, M, M + 1):
                    if s < m or s < 1:
                        continue
                    t = sd.threshold(min(s, M), x)
                    for pre, post in ((0, 0), (7, 9)):
                        for k in (t, t + 1):
                            if k > s:
                                continue
                            s1, r2 = planted(R, pre + s, s + post, s)
                            differ(r2, [(j * s) // k for j in range(k)])
                            name = b"%s_s%d_o%d_k%d" % (case.encode(), s, pre, k)
                            recs.append(record(name + b"/1", s1, quals(R, pre + s, phred, 0, top), rc(r2), quals(R, s + post, phred, 0, top), name + b"/2"))
                            meta.append(dict(s=s, pre=pre, k=k, thr=t))
                out.append((case, b"".join(recs), dict(m=m, M=M, x=x, phred=phred)))
                metas[case] = meta
    return out, metas


def cover_parameters():
    """Every planted candidate has the scored length and the mismatches it was built with, and one with thr + 1 mismatches is never
    chosen.  Where nothing but the planted overlap can be below the threshold -- m = M of 150 or 255, so that every candidate is at
    least that long, and x <= 0.5 --, thr mismatches combine at the planted offset and thr + 1 do not combine at all, for each
    overlap length at and above M."""
    strict = 0
    for case, _text, kw in cases("parameters"):
        rows, meta = scored("parameters")[case], family("parameters")[1][case]
        assert len(rows) == len(meta) > 0
        hit, miss = set(), set()
        for (p, cand, off), me in zip(rows, meta):
            at = next(c for c in cand if c[0] == me["pre"])
            assert (at[1], at[2]) == (me["s"], me["k"])
            assert not (me["k"] == me["thr"] + 1 and off == me["pre"]), p[0]
            if me["k"] == me["thr"] and off == me["pre"]:
                hit.add(me["s"])
            if me["k"] == me["thr"] + 1 and off == -1:
                miss.add(me["s"])
        if kw["m"] >= 150 and kw["x"] <= 0.5:
            assert hit == miss == {kw["M"], kw["M"] + 1}, (case, hit, miss)
            strict += 1
    assert strict == len(PHREDS) * 2 * (len(DENSITIES) - 1)
    return dict(cases=len(cases("parameters")), strict=strict)


# ---- tags
TAG_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 300)
TAG_SLASHES = (0, 61, 62, 63, 64, 65, "last", None)


def _build_tags():
    """Headers of 0 .. 300 bytes behind the '@', the last '/' at the first byte, around byte 64 (the stride of the tag scan; the
    header's byte k + 1 is the tag's byte k, so 61 .. 65 cover both ways of counting), at the last byte, or absent; with more
    '/' before it on both sides of byte 64.  Each header heads a pair that combines and one that does not (and passes the length
    filter, so the tag reaches all four streams).  The program cuts only a combined pair's tag at the last '/'; an uncombined
    pair's loses a closing "/1" or "/2" and nothing else, and white space at the header's end goes in both (this family showed that:
    the definition and the kernel used to cut both kinds at the last '/'); directed headers for those rules close the family."""
    R = np.random.RandomState(4501)
    fill = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_:.- #", dtype=np.uint8)
    recs, meta = [], []
    f = rnd_seq(R, 60)
    for H in TAG_LENGTHS:
        for k, at in enumerate(TAG_SLASHES):
            pos = H - 1 if at == "last" else at
            if pos is not None and not 0 <= pos < H:
                continue
            for more in ((), (3, 40, 62, 64, 70, 127)):
                h = bytearray(fill[R.randint(0, len(fill), size=H)].tobytes())
                if h.endswith(b" "):                          # (white space at the end is not part of a header: below)
                    h[-1] = ord("x")
                slashes = [] if pos is None else [pos] + [q for q in more if q < pos]
                if more and len(slashes) < 2:
                    continue
                for q in slashes:
                    h[q] = ord("/")
                h2 = bytes(h[:-1]) + b"2" if H > 1 and k % 2 else b"r2"
                for kind, s1, s2 in (("comb", f[:40], rc(f[20:60])), ("unc", f[:50], b"T" * 47 + b"GCA")):
                    recs.append(record(bytes(h), s1, quals(R, len(s1)), s2, quals(R, len(s2)), h2))
                    meta.append(dict(H=H, last=pos, slashes=sorted(slashes), kind=kind))
    # how the two kinds end a tag: a closing "/1" or "/2" (uncombined) against the last '/' (combined), white space at the end
    long = bytes(fill[R.randint(0, len(fill) - 2, size=70)].tobytes())
    for h in (b"/1", b"/2", b"q/1/", b"a/yyy", b"a/3", b"a/12", b"a//1", b"a/1/2", b"a/1 ", b"a/2 \t", b"a b  ", b" ", long + b"/1", long + b"/2 ",
              long[:61] + b"/1", long[:62] + b"/2", long[:63] + b"/1", long[:62] + b"/x", long + b"/" + long):
        for kind, s1, s2 in (("comb", f[:40], rc(f[20:60])), ("unc", f[:50], b"T" * 47 + b"GCA")):
            recs.append(record(h, s1, quals(R, len(s1)), s2, quals(R, len(s2))))
            meta.append(dict(H=None, kind=kind))
    return [("tags", b"".join(recs), {})], {"tags": meta}


def cover_tags():
    rows, meta = scored("tags")["tags"], family("tags")[1]["tags"]
    seen = set()
    for (p, _cand, off), me in zip(rows, meta):
        assert (off >= 0) == (me["kind"] == "comb")
        if me["H"] is None:
            continue
        assert len(sd.tag_of(p[0])) == (me["H"] if me["last"] is None else me["last"])
        seen.add((me["H"], me["last"], me["kind"]))
        if len(me["slashes"]) > 1:
            seen.add(("several", min(me["slashes"]) < 63, max(me["slashes"]) > 64, me["kind"]))
    for kind in ("comb", "unc"):
        for H in TAG_LENGTHS:
            assert (H, None, kind) in seen and (H == 0 or (H, H - 1, kind) in seen and (H, 0, kind) in seen)
        for pos in (61, 62, 63, 64, 65):
            assert all((H, pos, kind) in seen for H in (127, 128, 300))
        assert ("several", True, True, kind) in seen
    return dict(pairs=len(rows))


COVER = dict(length_grid=cover_length_grid, deciding_position=cover_deciding_position, quality_ties=cover_quality_ties,
             parameters=cover_parameters, tags=cover_tags)
