"""The definition of paired-end adapter and quality trimming (the driver's `ktrim -k KIT -o PREFIX -1 R1 -2 R2 -c`, microcket:371 /
405 / 413 / 430 / 444: Ktrim 1.6.0) in plain Python, and a seeded generator of paired FASTQ for it.  This file is what mkt_trim_*
(include/mkt.h) and bin/ktrim are compared with byte for byte; it is itself pinned against the program it restates by
tests/golden/ktrim_golden.json (made by tests/golden/make_ktrim_golden.py).

The rule, per pair (all comparisons are of bytes as they stand: lower case never equals upper case, N equals only N):
  common length   n = min(len1, len2); all four strings are cut to n
  quality         a cycle passes when byte >= phred + min_qual in both reads.  k = the largest i + 1, i >= min_size - 1, such that the
                  `window` cycles i - window + 1 .. i all pass (a window that would start before cycle 0 does not pass); no such i:
                  the pair is dropped.  All four strings are cut to k.
  seeds           every position at which the first 3 letters of adapter 1 stand in read 1, or the first 3 of adapter 2 in read 2
                  (wholly inside the k cycles), ascending, each position once
  verification    at a seed p, L = min(k - p, adapter length), limit = ceil(float32(L) * float32(mismatch)) in float32: read 1's
                  [p, p + L) differs from adapter 1's first L letters in at most `limit` places AND read 2's from adapter 2's.
                  The first seed that verifies wins (counter Aadaptor): p >= min_size keeps p cycles; else the pair is dropped,
                  and counts as a dimer when p <= 1.
  tail            when no seed verifies.  With i = k - 2: the number of failures among  r1[i] == a1[0], r1[i+1] == a1[1], r2[i] == a2[0],
                  r2[i+1] == a2[1], revcomp(r1[5], r2[i-6]), revcomp(r2[5], r1[i-6])  is at most 1: tail hit, i cycles are kept (dropped
                  if i < min_size).  Otherwise with i = k - 1: failures among  r1[i] == a1[0], r2[i] == a2[0], revcomp(r1[5], r2[i-6]),
                  revcomp(r2[5], r1[i-6]), revcomp(r1[6], r2[i-7]), revcomp(r2[6], r1[i-7])  at most 1: tail hit, i cycles kept.
                  revcomp(x, y) holds for (A,T) (C,G) (G,C) (T,A) only.
  output          header lines whole, the third line is "+"; interleaved: read 1's record, then read 2's
  log             Total, Dropped, Aadaptor, TailHit, Dimer, Pass: "name\\tcount\\n" each
Deliberately different from the program (it damages such records; here they are refused with the pair's ordinal): sequence and
quality of different lengths, a header line longer than MAX_HEADER bytes, a read longer than MAX_READ, a record without '@' or '+',
a quality byte outside phred .. 126, streams of different pair counts, a line count that is no multiple of 4.
"""
import hashlib
import random

import numpy as np

MAX_READ = 510          # MKT_TRIM_MAX_READ: the program reads a line into 512 bytes (510 letters, the newline, the terminator)
MAX_HEADER = 126        # MKT_TRIM_MAX_HEADER: and a header line into 128
MIN_ADAPTER, MAX_ADAPTER = 8, 64
SEED_LEN = 3
DIMER_INSERT = 1
KITS = {  # name -> (adapter 1, adapter 2); the names as the program spells them
    "illumina": ("AGATCGGAAGAGC", "AGATCGGAAGAGC"),
    "nextera": ("CTGTCTCTTATACACATCT", "CTGTCTCTTATACACATCT"),
    "transposase": ("TCGTCGGCAGCGTC", "GTCTCGTGGGCTCG"),
    "bgi": ("AAGTCGGAGGCCAAGCGGTC", "AAGTCGGATCGTAGCCATGT"),
}
KIT_NAMES = {"illumina": "illumina", "ILLUMINA": "illumina", "Illumina": "illumina", "Nextera": "nextera", "nextera": "nextera",
             "Transposase": "transposase", "transposase": "transposase", "BGI": "bgi", "bgi": "bgi"}
DEFAULTS = dict(kit=None, adapter1=None, adapter2=None, min_size=36, phred=33, min_qual=20, window=5, mismatch=0.125)
PASS, DROP_QUALITY, ADAPTER, TAILHIT = 0, 1, 2, 3
STAT_NAMES = ("Total", "Dropped", "Aadaptor", "TailHit", "Dimer", "Pass")
_PAIR = {(65, 84), (67, 71), (71, 67), (84, 65)}
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def sha(b):
    return hashlib.sha256(b).hexdigest()


def resolve(**opts):
    """-> dict(a1, a2, min_size, phred, min_qual, window, mismatch) or ValueError: the argument check"""
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise ValueError(f"unknown option {k}")
        o[k] = v
    if o["kit"] is not None:      # the kit wins over adapter1 / adapter2
        if o["kit"] in ("CLIP", "clip"):
            raise ValueError("the CLIP kit is not supported")
        if o["kit"] not in KIT_NAMES:
            raise ValueError(f"unknown kit {o['kit']}")
        a1, a2 = KITS[KIT_NAMES[o["kit"]]]
    elif o["adapter1"] is None:
        if o["adapter2"] is not None:
            raise ValueError("adapter2 without adapter1")
        a1, a2 = KITS["illumina"]
    else:
        a1 = o["adapter1"]
        a2 = o["adapter2"] if o["adapter2"] is not None else a1
        n = min(len(a1), len(a2))      # the common length is what is compared
        if not MIN_ADAPTER <= n <= MAX_ADAPTER:
            raise ValueError(f"adapter size {n}: need {MIN_ADAPTER} .. {MAX_ADAPTER}")
        a1, a2 = a1[:n], a2[:n]
        if any(c in "\n\r\0" for c in a1 + a2):
            raise ValueError("adapter with a line end in it")
    if not 10 <= o["min_size"] <= MAX_READ:
        raise ValueError(f"min size {o['min_size']}: need 10 .. {MAX_READ}")
    if not 1 <= o["phred"] <= 126 or not 1 <= o["min_qual"] <= 126 or o["phred"] + o["min_qual"] > 126:
        raise ValueError("phred / min quality: need 1 .. 126 each and a sum of at most 126")
    if not 1 <= o["window"] <= MAX_READ:
        raise ValueError(f"window {o['window']}: need 1 .. {MAX_READ}")
    if not 0.0 <= o["mismatch"] <= 1.0:
        raise ValueError(f"mismatch {o['mismatch']}: need 0 .. 1")
    return dict(a1=a1.encode() if isinstance(a1, str) else a1, a2=a2.encode() if isinstance(a2, str) else a2, min_size=o["min_size"], phred=o["phred"],
                min_qual=o["min_qual"], window=o["window"], mismatch=float(o["mismatch"]))


def limit_table(mismatch, upto=MAX_ADAPTER):
    """limit[L], L = 0 .. upto: the mismatches allowed over L compared letters (float32 product, float32 ceiling)"""
    m = np.float32(mismatch)
    return [int(np.ceil(np.float32(L) * m)) for L in range(upto + 1)]


def _rc(x, y):
    return (x, y) in _PAIR


def trim_pair(s1, q1, s2, q2, P, limit=None):
    """-> (kept cycles, class, dimer): class PASS / DROP_QUALITY / ADAPTER / TAILHIT; kept < min_size (0 for DROP_QUALITY) = dropped"""
    a1, a2, s, w = P["a1"], P["a2"], P["min_size"], P["window"]
    thr = P["phred"] + P["min_qual"]
    limit = limit or limit_table(P["mismatch"])
    n = min(len(s1), len(s2))
    k, run = 0, 0
    for i in range(n):
        run = run + 1 if (q1[i] >= thr and q2[i] >= thr) else 0
        if run >= w and i >= s - 1:
            k = i + 1
    if k == 0:
        return 0, DROP_QUALITY, False
    r1, r2 = s1[:k], s2[:k]
    seeds = set()
    for r, a in ((r1, a1), (r2, a2)):
        p = r.find(a[:SEED_LEN])
        while p >= 0:
            seeds.add(p)
            p = r.find(a[:SEED_LEN], p + 1)
    for p in sorted(seeds):
        L = min(k - p, len(a1))
        if sum(r1[p + j] != a1[j] for j in range(L)) <= limit[L] and sum(r2[p + j] != a2[j] for j in range(L)) <= limit[L]:
            return p, ADAPTER, p <= DIMER_INSERT
    i = k - 2
    bad = (r1[i] != a1[0]) + (r1[i + 1] != a1[1]) + (r2[i] != a2[0]) + (r2[i + 1] != a2[1]) + (not _rc(r1[5], r2[i - 6])) + (not _rc(r2[5], r1[i - 6]))
    if bad <= 1:
        return i, TAILHIT, False
    i = k - 1
    bad = ((r1[i] != a1[0]) + (r2[i] != a2[0]) + (not _rc(r1[5], r2[i - 6])) + (not _rc(r2[5], r1[i - 6])) + (not _rc(r1[6], r2[i - 7])) +
           (not _rc(r2[6], r1[i - 7])))
    if bad <= 1:
        return i, TAILHIT, False
    return k, PASS, False


def parse(text, phred=33, first=0):
    """One FASTQ stream -> [(header line, seq, qual)].  A last line without its newline still counts."""
    if not text:
        return []
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    if len(lines) % 4:
        raise ValueError(f"{len(lines)} lines: not whole records (4 lines each)")
    out = []
    for k in range(0, len(lines), 4):
        h, s, p, q = lines[k:k + 4]
        o = first + k // 4
        if not h.startswith(b"@") or not p.startswith(b"+"):
            raise ValueError(f"read pair {o}: a record without '@' or '+'")
        if len(h) > MAX_HEADER:
            raise ValueError(f"read pair {o}: a header line longer than {MAX_HEADER} bytes")
        if len(s) > MAX_READ:
            raise ValueError(f"read pair {o}: a read longer than {MAX_READ} bases")
        if len(s) != len(q):
            raise ValueError(f"read pair {o}: sequence and quality differ in length")
        if any(not phred <= c <= 126 for c in q):
            raise ValueError(f"read pair {o}: a quality byte outside {phred} .. 126")
        out.append((h, s, q))
    return out


def split_interleaved(text):
    """interleaved FASTQ -> (stream 1, stream 2)"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if len(lines) % 8:
        raise ValueError(f"{len(lines)} lines: not whole read pairs (8 lines each)")
    a, b = [], []
    for k in range(0, len(lines), 8):
        a += lines[k:k + 4]
        b += lines[k + 4:k + 8]
    return b"".join(x + b"\n" for x in a), b"".join(x + b"\n" for x in b)


def trim_stream(text1, text2, **opts):
    """-> (interleaved, read1, read2, stats): stats = (total, dropped, adapter, tailhit, dimer, pass)"""
    P = resolve(**opts)
    A, B = parse(text1, P["phred"]), parse(text2, P["phred"])
    if len(A) != len(B):
        raise ValueError(f"{len(A)} records in stream 1, {len(B)} in stream 2")
    limit = limit_table(P["mismatch"])
    il, o1, o2 = [], [], []
    dropped = adapter = tailhit = dimer = npass = 0
    for (h1, s1, q1), (h2, s2, q2) in zip(A, B):
        if min(len(s1), len(s2)) < P["min_size"]:      # (nothing to look at: the quality rule finds no cycle)
            dropped += 1
            continue
        k, cls, dim = trim_pair(s1, q1, s2, q2, P, limit)
        adapter += cls == ADAPTER
        tailhit += cls == TAILHIT
        dimer += dim
        if k < P["min_size"]:
            dropped += 1
            continue
        npass += 1
        a = b"%s\n%s\n+\n%s\n" % (h1, s1[:k], q1[:k])
        b = b"%s\n%s\n+\n%s\n" % (h2, s2[:k], q2[:k])
        il.append(a + b)
        o1.append(a)
        o2.append(b)
    return b"".join(il), b"".join(o1), b"".join(o2), (len(A), dropped, adapter, tailhit, dimer, npass)


def log_text(stats):
    return "".join(f"{n}\t{v}\n" for n, v in zip(STAT_NAMES, stats))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def synth(seed, pairs, read_len=None, kit="illumina", adapters=None):
    """-> (stream 1, stream 2): seeded paired FASTQ with a mix of inserts shorter than, equal to and longer than the reads, adapter
    read-through with sequencing errors, degraded quality tails, N, unequal read lengths"""
    r = random.Random(seed)
    a1, a2 = adapters or KITS[kit]
    o1, o2 = [], []
    for k in range(pairs):
        L = read_len or r.choice((50, 75, 100, 100, 125, 150, 150))
        u = r.random()
        if u < 0.02:
            ins = r.randrange(0, 4)
        elif u < 0.45:
            ins = r.randrange(4, L + 3)
        else:
            ins = r.randrange(L, 3 * L)
        frag = "".join(r.choice("ACGT") for _ in range(ins))
        fill = "".join(r.choice("ACGT") for _ in range(L))
        s1 = (frag + a1 + fill)[:L]
        s2 = (revcomp(frag.encode()).decode() + a2 + fill[::-1])[:L]
        L2 = L if r.random() < 0.9 else L - r.randrange(1, 8)
        s2 = s2[:L2]
        reads = []
        for s in (s1, s2):
            s = list(s)
            q = []
            tail = r.randrange(len(s) // 2, 2 * len(s)) if r.random() < 0.5 else 10 ** 6
            for j in range(len(s)):
                good = r.random() < (0.97 if j < tail else 0.4)
                q.append(chr(33 + (r.randrange(20, 41) if good else r.randrange(2, 20))))
                e = r.random()
                if e < 0.01:
                    s[j] = r.choice("ACGT")
                elif e < 0.013:
                    s[j] = "N"
            reads.append(("".join(s), "".join(q)))
        o1.append(f"@r{k}/1\n{reads[0][0]}\n+\n{reads[0][1]}\n")
        o2.append(f"@r{k}/2\n{reads[1][0]}\n+\n{reads[1][1]}\n")
    return "".join(o1).encode(), "".join(o2).encode()
