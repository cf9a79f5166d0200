"""The directed families of adapter and quality trimming: the smallest shapes at which the kernels can go wrong.  Every batch is
(name, options for ktrimdef / Trimmer, the reference's argv for them, [(h1, s1, q1, h2, s2, q2)]) with well-formed records only;
REFUSED holds what this project refuses (and why the reference is never asked about it).  Deterministic: the golden stores hashes of
these inputs beside the reference's output."""
import random

import ktrimdef as kd

ILL = kd.KITS["illumina"][0]
A64 = "GATTACAGGCTTAACCGGTTCATGCAATGCCGTAAGCTTGGCAACCTTGGATCCGTAGCATGCA"      # a 64-letter adapter (read 1)
B64 = "CCATGGTTAACGCGTATCGGATCCAAGGTTCCGATATCGGCCAATTGGCTAGCTAGGATCGATC"      # and another (read 2)
assert len(A64) == 64 and len(B64) == 64


def rnd(seed, n, alphabet="ACGT"):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


def clean(s, *words):
    """s with every occurrence of the words' 3-letter heads broken (no accidental seeds)"""
    s = list(s)
    for w in words:
        h = w[:3]
        k = "".join(s).find(h)
        while k >= 0:
            s[k + 1] = next(c for c in "ACGT" if c != h[1] and c != s[k] and c != s[k + 2])
            k = "".join(s).find(h)
    return "".join(s)


def rc(s):
    return kd.revcomp(s.encode()).decode()


def mutate(s, positions, to=None):
    s = list(s)
    for p in positions:
        s[p] = to or {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[s[p]]
    return "".join(s)


def pair(name, insert, L, a1=ILL, a2=None, q1=None, q2=None, L2=None, seed=0, fill=None):
    """a pair of reads of L (L2) cycles over an insert of n letters (or the insert itself), adapters behind it"""
    a2 = a2 or a1
    frag = clean(rnd(1000 + seed, insert), a1, a2, rc(a1), rc(a2)) if isinstance(insert, int) else insert
    f1 = fill or clean(rnd(2000 + seed, 600), a1, a2)
    f2 = fill or clean(rnd(3000 + seed, 600), a1, a2)
    s1 = (frag + a1 + f1)[:L]
    s2 = (rc(frag) + a2 + f2)[:L2 or L]
    return (f"@{name}/1", s1, q1 or "I" * len(s1), f"@{name}/2", s2, q2 or "I" * len(s2))


def text_of(records):
    return ("".join(f"{h1}\n{s1}\n+\n{q1}\n" for h1, s1, q1, _, _, _ in records).encode(), "".join(f"{h2}\n{s2}\n+\n{q2}\n" for _, _, _, h2, s2, q2 in records).encode())


def length_grid():
    R = []
    for L in (36, 37, 63, 64, 65, 127, 128, 129, 255, 256, 257, 509, 510):
        R.append(pair(f"plain{L}", 2 * L, L, seed=L))
        R.append(pair(f"adapter{L}", L - 14, L, seed=L + 1))
        R.append(pair(f"tail2_{L}", L - 2, L, seed=L + 2))
        R.append(pair(f"tail1_{L}", L - 1, L, seed=L + 3))
    for a, b in ((63, 65), (65, 63), (64, 70), (70, 64), (127, 129), (129, 127), (128, 100), (80, 70)):
        R.append(pair(f"unequal{a}_{b}", 300, a, L2=b, seed=a * b))
        R.append(pair(f"unequal_ad{a}_{b}", min(a, b) - 10, a, L2=b, seed=a * b + 1))
    return [("length_grid", {}, [], R)]


def quality_window():
    B = []
    R = []
    for good in (60, 40, 37, 36, 35):
        q = "I" * good + "#" * (100 - good)
        R.append(pair(f"prefix{good}", 300, 100, q1=q, q2=q, seed=good))
    R.append(pair("thr4", 300, 100, q1="I" * 50 + "4" * 50, seed=1))
    R.append(pair("thr5", 300, 100, q1="I" * 50 + "5" * 50, seed=2))
    for run in (4, 5):      # w - 1 and w good cycles inside a bad tail
        q = "I" * 50 + "#" * 20 + "I" * run + "#" * (30 - run)
        R.append(pair(f"island{run}", 300, 100, q1=q, seed=run))
        R.append(pair(f"island{run}_r2", 300, 100, q2=q, seed=run + 10))
    for edge in (64, 128):      # a window straddling a word boundary, and one cycle short of it
        for lo in (edge - 4, edge - 3, edge - 2, edge - 1):
            q = "I" * 40 + "#" * (lo - 40) + "I" * 5 + "#" * (150 - lo - 5)
            R.append(pair(f"straddle{edge}_{lo}", 400, 150, q1=q, q2="I" * 150, seed=lo))
            q4 = "I" * 40 + "#" * (lo - 40) + "I" * 4 + "#" * (150 - lo - 4)
            R.append(pair(f"short{edge}_{lo}", 400, 150, q1="I" * 150, q2=q4, seed=lo + 1))
    R.append(pair("bad_cycle_r2", 300, 100, q2="I" * 70 + "#" + "I" * 29, seed=5))
    R.append(pair("bad_last_r2", 300, 100, q2="I" * 99 + "#", seed=6))
    R.append(pair("all_bad", 300, 100, q1="#" * 100, seed=7))
    R.append(pair("good_then_adapter", 58, 100, q1="I" * 60 + "#" * 40, q2="I" * 60 + "#" * 40, seed=8))
    B.append(("quality_default", {}, [], R))
    R = [pair(f"w1_{k}", 300, 100, q1="I" * 40 + "#" * k + "I" + "#" * (59 - k), seed=k) for k in (0, 1, 30)]
    B.append(("quality_w1", dict(window=1), ["-w", "1"], R))
    R = [pair("wmax_all_good", 2000, 510, seed=1), pair("wmax_one_bad", 2000, 510, q1="I" * 200 + "#" + "I" * 309, seed=2), pair("wmax_short", 300, 100, seed=3)]
    B.append(("quality_wmax", dict(window=510, min_size=510), ["-w", "510", "-s", "510"], R))
    R = [pair("w40_fit", 300, 100, q1="#" * 10 + "I" * 40 + "#" * 50, seed=1), pair("w40_short", 300, 100, q1="#" * 10 + "I" * 39 + "#" * 51, seed=2),
         pair("w40_from0", 300, 100, q1="I" * 40 + "#" * 60, seed=3)]
    B.append(("quality_w40_s12", dict(window=40, min_size=12), ["-w", "40", "-s", "12"], R))
    R = [pair("q1_all", 300, 100, q1="\"" * 100, seed=1), pair("q1_none", 300, 100, q1="!" * 100, seed=2)]
    B.append(("quality_q1", dict(min_qual=1), ["-q", "1"], R))
    R = [pair("p64_pass", 300, 100, q1="T" * 100, q2="h" * 100, seed=1), pair("p64_fail", 300, 100, q1="T" * 60 + "S" * 40, q2="h" * 100, seed=2)]
    B.append(("quality_p64", dict(phred=64), ["-p", "64"], R))
    R = [pair("s50_50", 300, 100, q1="I" * 50 + "#" * 50, seed=1), pair("s50_49", 300, 100, q1="I" * 49 + "#" * 51, seed=2), pair("s50_ad50", 50, 100, seed=3),
         pair("s50_ad49", 49, 100, seed=4)]
    B.append(("min_size_50", dict(min_size=50), ["-s", "50"], R))
    return B


def adapter_position():
    B = []
    for kit, flag in (("illumina", "illumina"), ("nextera", "Nextera"), ("transposase", "transposase"), ("bgi", "BGI")):
        a1, a2 = kd.KITS[kit]
        R = [pair(f"{kit}_ins{n}", n, 100, a1, a2, seed=n) for n in range(0, 101)]
        for n in list(range(60, 69)) + list(range(124, 133)) + [147, 148, 149, 150]:
            R.append(pair(f"{kit}_150_ins{n}", n, 150, a1, a2, seed=500 + n))
        B.append((f"adapter_position_{kit}", dict(kit=flag), ["-k", flag], R))
    return B


def mismatch_limit():
    B = []
    for m, flags in ((0.125, []), (0.0, ["-m", "0"]), (0.3, ["-m", "0.3"])):
        lim = kd.limit_table(m)
        R = []
        for Lc in sorted({3, 4, 7, 8, 9, 10, 15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 47, 48, 49, 55, 56, 57, 63, 64} | {k for k in range(3, 64) if lim[k] != lim[k + 1]}
                         | {k + 1 for k in range(3, 64) if lim[k] != lim[k + 1]}):
            n = 100 - Lc
            base = pair(f"L{Lc}", n, 100, A64, B64, seed=Lc)
            for extra in (0, 1):
                mm = lim[Lc] + extra
                if mm > Lc - 3:
                    continue
                pos = [n + 3 + j for j in range(mm)]      # behind the seed letters
                h1, s1, q1, h2, s2, q2 = base
                R.append((f"@L{Lc}_r1_mm{mm}/1", mutate(s1, pos), q1, f"@L{Lc}_r1_mm{mm}/2", s2, q2))
                R.append((f"@L{Lc}_r2_mm{mm}/1", s1, q1, f"@L{Lc}_r2_mm{mm}/2", mutate(s2, pos), q2))
                if mm:
                    R.append((f"@L{Lc}_r1_n{mm}/1", mutate(s1, pos, "N"), q1, f"@L{Lc}_r1_n{mm}/2", s2, q2))
                    R.append((f"@L{Lc}_r2_n{mm}/1", s1, q1, f"@L{Lc}_r2_n{mm}/2", mutate(s2, pos, "N"), q2))
            h1, s1, q1, h2, s2, q2 = base      # mismatches between the reads inside the insert do not matter
            if n >= 10:
                R.append((f"@L{Lc}_insert/1", mutate(s1, (1, 4, 7)), q1, f"@L{Lc}_insert/2", mutate(s2, (2, 5)), q2))
        B.append((f"mismatch_limit_m{m}", dict(adapter1=A64, adapter2=B64, mismatch=m), ["-a", A64, "-b", B64] + flags, R))
    return B


def decoy_seeds():
    R = []
    frag = clean(rnd(77, 70), ILL, rc(ILL))
    for k, name in ((1, "once"), (4, "several")):
        f = list(frag)
        for j in range(k):
            f[10 + 9 * j:13 + 9 * j] = "AGA"
        R.append(pair(f"decoy_{name}", "".join(f), 100, seed=k))
        f2 = rc("".join(f))
        R.append((f"@decoy_r2_{name}/1", (frag + ILL + rnd(5, 100))[:100], "I" * 100, f"@decoy_r2_{name}/2", (f2 + ILL + rnd(6, 100))[:100], "I" * 100))
    R.append(pair("decoy_close", frag[:40] + "AGATCGGTTTTTT" + frag[53:], 100, seed=9))      # 7 of 13 letters: does not verify
    R.append(pair("two_sites", frag[:40] + ILL + frag[53:], 100, seed=10))                   # the first of two verifying sites wins
    h1, s1, q1, h2, s2, q2 = pair("r1_only", 60, 100, seed=11)
    R.append((h1, s1, q1, h2, clean(rnd(12, 100), ILL), q2))
    R.append(("@r2_only/1", clean(rnd(13, 100), ILL), q1, "@r2_only/2", s2, q2))
    R.append(("@seed_r2_only/1", mutate(s1, (60,)), q1, "@seed_r2_only/2", s2, q2))          # read 1's seed broken, one mismatch: read 2 seeds it
    R.append(("@polyA/1", "A" * 100, "I" * 100, "@polyA/2", "T" * 100, "I" * 100))
    R.append(("@aga_repeat/1", "AG" * 50, "I" * 100, "@aga_repeat/2", "CT" * 50, "I" * 100))
    B = [("decoy_seeds", {}, [], R)]
    c1, c2 = "ACGGTCAATGCCA", "TTGACCGTAAGGCTA"
    R = [pair(f"custom_same_{n}", n, 100, c1, c1, seed=n) for n in (0, 1, 2, 35, 36, 60, 97, 98, 99, 100)]
    B.append(("custom_same", dict(adapter1=c1), ["-a", c1], R))
    R = [pair(f"custom_diff_{n}", n, 100, c1, c2[:13], seed=n) for n in (0, 1, 2, 35, 36, 60, 97, 98, 99, 100)]
    B.append(("custom_different", dict(adapter1=c1, adapter2=c2), ["-a", c1, "-b", c2], R))
    return B


def text():
    R = []
    h1, s1, q1, h2, s2, q2 = pair("x", 60, 100, seed=1)
    R.append(("@lower/1", s1.lower(), q1, "@lower/2", s2.lower(), q2))
    R.append(("@lower_insert/1", s1[:60].lower() + s1[60:], q1, "@lower_insert/2", s2[:60].lower() + s2[60:], q2))
    R.append(("@dots/1", mutate(s1, (3, 50, 62), "."), q1, "@dots/2", mutate(s2, (4, 61), "N"), q2))
    R.append(("@a b c", s1, q1, "@a b c", s2, q2))
    R.append(("@tab\there \t", s1, q1, "@zz", s2, q2))
    R.append(("@" + "h" * 125, s1, q1, "@" + "k" * 125, s2, q2))
    R.append(("@", s1, q1, "@", s2, q2))
    return [("text", {}, [], R)]


def all_batches():
    return length_grid() + quality_window() + adapter_position() + mismatch_limit() + decoy_seeds() + text()


def _one(h1="@r/1", s1=None, p1="+", q1=None, h2="@r/2", s2=None, p2="+", q2=None, n=60):
    s1 = s1 if s1 is not None else rnd(1, n)
    s2 = s2 if s2 is not None else rnd(2, n)
    q1 = q1 if q1 is not None else "I" * len(s1)
    q2 = q2 if q2 is not None else "I" * len(s2)
    good = f"@g/1\n{rnd(3, 50)}\n+\n{'I' * 50}\n", f"@g/2\n{rnd(4, 50)}\n+\n{'I' * 50}\n"
    return (good[0] * 2 + f"{h1}\n{s1}\n{p1}\n{q1}\n" + good[0]).encode(), (good[1] * 2 + f"{h2}\n{s2}\n{p2}\n{q2}\n" + good[1]).encode()


# (name, stream 1, stream 2, options, what the message holds): the bad pair is number 2 where a pair is at fault.  The reference
# damages such records (its line buffers hold 127 and 511 bytes; it trusts the shape), so none of them is a golden.
REFUSED_INPUT = [
    ("qual_short", *_one(q1="I" * 59), {}, "read pair 2"),
    ("qual_long_r2", *_one(q2="I" * 61), {}, "read pair 2"),
    ("no_at", *_one(h1="r/1"), {}, "read pair 2"),
    ("no_plus_r2", *_one(p2="-"), {}, "read pair 2"),
    ("empty_plus", *_one(p1=""), {}, "read pair 2"),
    ("qual_below_phred", *_one(q1="I" * 30 + " " + "I" * 29), {}, "read pair 2"),
    ("qual_below_phred64", *_one(q2="h" * 59 + "?", q1="h" * 60), dict(phred=64), "read pair 2"),
    ("qual_127", *_one(q2="I" * 59 + "\x7f"), {}, "read pair 2"),
    ("header_127", *_one(h1="@" + "h" * 126), {}, "read pair 2"),
    ("header_200", *_one(h2="@" + "h" * 199), {}, "read pair 2"),
    ("read_511", *_one(n=511), {}, "read pair 2"),
    ("read_512_r2", *_one(s2=rnd(9, 512)), {}, "read pair 2"),
    ("lines_not_4", _one()[0] + b"@x\nACGT\n", _one()[1], {}, "lines"),
    ("pair_counts", _one()[0] + b"@x\nACGT\n+\nIIII\n", _one()[1], {}, "read pairs in stream"),
]
# (name, options, the reference's exit code for the same argv or None where it accepts them)
REFUSED_OPTIONS = [
    ("q0", dict(min_qual=0), 12), ("p0", dict(phred=0), 12), ("w0", dict(window=0), 12), ("s9", dict(min_size=9), 11), ("s_over", dict(min_size=511), None),
    ("w_over", dict(window=511), None), ("q_sum", dict(phred=64, min_qual=63), None), ("m_neg", dict(mismatch=-0.1), None), ("m_over", dict(mismatch=1.5), None),
    ("kit_unknown", dict(kit="foo"), 13), ("kit_clip", dict(kit="CLIP"), None), ("adapter_7", dict(adapter1="ACGTACG"), 20), ("adapter_65", dict(adapter1="ACGTA" * 13), 20),
    ("b_without_a", dict(adapter2="ACGTACGTAA"), 14),
]
