"""Directed inputs for the FASTQ duplicate remover (mkt_rmdup.hip: k_rm_keys / insert / mark / rehash / order / sums / copy) at its
batch, table, key and copy edges.  Plain Python / numpy: nothing here needs a GPU or the program.  A case has a name, the bytes of an
interleaved FASTQ, krmdup's arguments, how it is to be run (interleaved too, the streaming pieces, MKT_RMDUP_SEGMENT_MB) and a check
that works out, from the numpy restatement below only -- never from GPU output --, that the input really sits at the edge it was
written for; a case that misses its edge fails tests/test_krmdup_edges_host.py.  Texts and results are made once per process and
never modified.

What the kernels do at these places: a pair's 64-bit key is 2 bits per base (C=0 A=1 T=2 G=3) over seq1[hskip1, epos1) then
seq2[hskip2, epos2); its bucket is the letter seq1[hskip1] (0 'A', 1 'C', 2 'G', 3 anything else, 'N' discards); the set of
(key, bucket) is an open-addressing table of pair ordinals, slot rm_mix(key + bucket) & mask, linear probing, the smaller ordinal
wins a slot by atomicMin; keys and buckets start with room for 2^17 ordinals and the table with 2^18 slots, both double; the output is
written per batch of 2^16 input pairs, buckets A, C, G, T inside it, 1024 kept records per workgroup of the copy.
"""
import numpy as np

import util

BATCH = 1 << 16
U64 = np.uint64
_CODE = np.full(256, 255, dtype=np.uint8)
for _c, _v in ((b"Cc", 0), (b"Aa", 1), (b"Tt", 2), (b"Gg", 3)):
    for _b in _c:
        _CODE[_b] = _v
_BASES = np.frombuffer(b"CATG", dtype=np.uint8)
_BUCKET = np.full(256, 3, dtype=np.uint8)                      # of the letter at seq1[hskip1]
_BUCKET[ord("A")], _BUCKET[ord("C")], _BUCKET[ord("G")] = 0, 1, 2
_TOP2_BUCKET = np.array([1, 0, 3, 2], dtype=np.uint8)          # bucket of an upper-case first base, from its 2-bit code
_ID = np.frombuffer(b"0123456789abcdefghijklmnopqrstuv", dtype=np.uint8)
_cache = {}


# ---- the numpy restatement: key, bucket, slot, who stays, in which order
def params(args):
    """krmdup's -k -K -s -S -> (hskip1, keylen1, hskip2, keylen2)"""
    p = {"-k": 5, "-s": 16, "-K": 5, "-S": 16}
    for i in range(0, len(args), 2):
        p[args[i]] = int(args[i + 1])
    return p["-k"], p["-s"], p["-K"], p["-S"]


def kwargs(args):
    h1, k1, h2, k2 = params(args)
    return dict(hskip1=h1, keylen1=k1, hskip2=h2, keylen2=k2)


def lines_of(text):
    """-> (bytes as uint8, start of every line, its end without the newline), a last line without newline counted as getline does"""
    buf = np.frombuffer(text, dtype=np.uint8)
    ends = np.flatnonzero(buf == 10)
    if len(buf) and buf[-1] != 10:
        ends = np.append(ends, len(buf))
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64) if len(ends) else np.zeros(0, dtype=np.int64)
    return buf, starts, ends.astype(np.int64)


def mix(x):
    return util._mix64_np(np.asarray(x, dtype=U64))


def slot(keys, bucket, mask):
    """rm_mix(key + bucket) & mask; the sum wraps at 2^64 as it does on the GPU"""
    with np.errstate(over="ignore"):
        return (mix(np.asarray(keys, dtype=U64) + np.asarray(bucket).astype(U64)) & U64(mask)).astype(np.int64)


def key_bases(keys, n):
    """the inverse of the key: n bases per key, most significant pair of bits first -> uint8 [len(keys), n]"""
    sh = (2 * (n - 1 - np.arange(n))).astype(U64)
    return _BASES[((np.asarray(keys, dtype=U64)[:, None] >> sh[None, :]) & U64(3)).astype(np.intp)]


def keys_of(text, args=()):
    """-> (key per pair, bucket per pair: 0 A, 1 C, 2 G, 3 other, 4 discarded)"""
    h1, k1, h2, k2 = params(args)
    e1, e2 = h1 + k1, h2 + k2
    buf, st, en = lines_of(text)
    n = len(st) // 8
    keys, bucket = np.zeros(n, dtype=U64), np.full(n, 4, dtype=np.uint8)
    if n == 0:
        return keys, bucket
    pad = np.concatenate([buf, np.full(64, 10, dtype=np.uint8)])             # (a line's end reads as its newline)
    s1, s2 = st[1:8 * n:8], st[5:8 * n:8]
    l1, l2 = en[1:8 * n:8] - s1, en[5:8 * n:8] - s2
    first = np.where(l1 >= e1, pad[np.minimum(s1 + h1, len(pad) - 1)], ord("N"))
    idx = np.flatnonzero((first != ord("N")) & (l2 >= e2))
    win = np.concatenate([pad[s1[idx, None] + np.arange(h1, e1)[None, :]], pad[s2[idx, None] + np.arange(h2, e2)[None, :]]], axis=1)
    code = _CODE[win]
    good = ~(code == 255).any(axis=1)
    k = np.zeros(len(idx), dtype=U64)
    for j in range(k1 + k2):
        k = (k << U64(2)) | (code[:, j] & 3).astype(U64)
    keys[idx[good]] = k[good]
    bucket[idx[good]] = _BUCKET[first[idx[good]]]
    return keys, bucket


def restate(text, args=()):
    """keys, bucket, state per pair (0 discarded, 1 duplicate, 2 + bucket kept), order (the kept ordinals as they are written: batch
    after batch, buckets A, C, G, T inside, input order inside those), kept[batch][bucket], (total, uniq, dup, discard)"""
    keys, bucket = keys_of(text, args)
    n = len(keys)
    live = np.flatnonzero(bucket < 4)
    o = np.lexsort((live, bucket[live], keys[live]))
    ks, bs = keys[live][o], bucket[live][o]
    new = np.ones(len(o), dtype=bool)
    new[1:] = (ks[1:] != ks[:-1]) | (bs[1:] != bs[:-1])
    state = np.zeros(n, dtype=np.uint8)
    state[live] = 1
    firsts = live[o][new]
    state[firsts] = 2 + bucket[firsts]
    kept = np.flatnonzero(state >= 2)
    order = kept[np.lexsort((kept, state[kept], kept // BATCH))]
    nb = (n + BATCH - 1) // BATCH
    per = np.zeros((nb, 4), dtype=np.int64)
    np.add.at(per, (kept // BATCH, state[kept] - 2), 1)
    uniq, dup, disc = int((state >= 2).sum()), int((state == 1).sum()), int((state == 0).sum())
    return dict(keys=keys, bucket=bucket, state=state, order=order, kept=per, stats=(n, uniq, dup, disc))


def plain(text, args=()):
    """krmdup.cpp:88-227 once more, line by line in plain Python and independent of everything above: load_batch sorts a batch's
    pairs into four lists by the letter seq1[hskip1], do_rmdup keeps one set per letter, the lists are written in A, C, G, T
    order.  -> (read 1 bytes, read 2 bytes, log)"""
    h1, k1, h2, k2 = params(args)
    e1, e2 = h1 + k1, h2 + k2
    L = text.split(b"\n")
    if L and L[-1] == b"":
        L.pop()
    n = len(L) // 8
    code = {65: 1, 97: 1, 84: 2, 116: 2, 67: 0, 99: 0, 71: 3, 103: 3}
    seen = {c: set() for c in "ACGT"}
    uniq = dup = disc = 0
    o1, o2 = [], []
    for b0 in range(0, n, BATCH):
        lists = {c: [] for c in "ACGT"}
        for r in range(b0, min(b0 + BATCH, n)):
            rec = L[8 * r:8 * r + 8]
            first = rec[1][h1:h1 + 1] if len(rec[1]) >= e1 else b"N"         # (the line's end is no letter: the T list)
            if first == b"N":
                disc += 1
                continue
            lists[first.decode() if first in (b"A", b"C", b"G") else "T"].append(rec)
        for c in "ACGT":
            for id1, s1, _p1, q1, id2, s2, _p2, q2 in lists[c]:
                if len(s1) < e1 or len(s2) < e2:
                    disc += 1
                    continue
                key, bad = 0, False
                for ch in s1[h1:e1] + s2[h2:e2]:
                    if ch not in code:
                        bad = True
                        break
                    key = (key << 2) | code[ch]
                if bad:
                    disc += 1
                elif key in seen[c]:
                    dup += 1
                else:
                    seen[c].add(key)
                    uniq += 1
                    o1.append(b"%s\n%s\n+\n%s\n" % (id1, s1, q1))
                    o2.append(b"%s\n%s\n+\n%s\n" % (id2, s2, q2))
    return b"".join(o1), b"".join(o2), util.krmdup_log(uniq + dup + disc, uniq, dup, disc)


def interleave(r1, r2):
    """the read-1 and read-2 records of two outputs alternating (what krmdup.pipe writes, in krmdup's order)"""
    l1, l2 = r1.split(b"\n")[:-1], r2.split(b"\n")[:-1]
    return b"".join(b"\n".join(l1[i:i + 4] + l2[i:i + 4]) + b"\n" for i in range(0, len(l1), 4))


# ---- building blocks
def rand_keys(R, n):
    return (R.randint(0, 1 << 32, size=n, dtype=np.uint64) << U64(32)) | R.randint(0, 1 << 32, size=n, dtype=np.uint64)


def rand_bases(R, shape):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[R.randint(0, 4, size=shape)]


def top_bucket(keys):
    """the bucket of a 32-base key whose first base is upper case"""
    return _TOP2_BUCKET[(np.asarray(keys, dtype=U64) >> U64(62)).astype(np.intp)]


def with_repeats(R, keys, rate, ok=None):
    """keys with a share of them replaced by the key of an earlier entry that is itself no repeat (and for which ok holds)"""
    n = len(keys)
    rep = R.rand(n) < rate
    rep[0] = False
    src = np.flatnonzero(~rep if ok is None else (~rep & ok))
    at = np.flatnonzero(rep)
    c = np.searchsorted(src, at)                                             # sources before each repeat
    at, c = at[c > 0], c[c > 0]
    out = keys.copy()
    out[at] = keys[src[(R.rand(len(at)) * c).astype(np.int64)]]
    return out


def reads(R, keys, L1, L2, lower=None, discard=None):
    """reads of L1 / L2 bases that carry the 32-base keys under the default arguments (5 bases, 16 of the key, a tail), everything
    outside the key random; lower: pairs whose first key base is lower case; discard: pairs that get an N inside the key window"""
    n = len(keys)
    kb = key_bases(keys, 32)
    s1, s2 = rand_bases(R, (n, L1)), rand_bases(R, (n, L2))
    s1[:, 5:21], s2[:, 5:21] = kb[:, :16], kb[:, 16:]
    if lower is not None:
        s1[lower, 5] |= 0x20
    if discard is not None:
        d = np.flatnonzero(discard)
        col = 5 + R.randint(0, 16, size=len(d))
        m2 = R.rand(len(d)) < 0.5
        s1[d[~m2], col[~m2]] = ord("N")
        s2[d[m2], col[m2]] = ord("N")
    return s1, s2


def fixed_text(s1, s2, first=0):
    """n pairs of fixed shape as bytes: ids '@' + 5 characters of the ordinal, a bare '+', qualities that differ pair by pair"""
    n, L1 = s1.shape
    L2 = s2.shape[1]
    o = np.arange(first, first + n, dtype=np.int64)
    ids = _ID[(o[:, None] >> (5 * np.arange(4, -1, -1))[None, :]) & 31]
    c = lambda b: np.broadcast_to(np.frombuffer(b, dtype=np.uint8), (n, len(b)))
    q = lambda L, k: (65 + (o[:, None] * k + np.arange(L)[None, :]) % 26).astype(np.uint8)
    return np.concatenate([c(b"@"), ids, c(b"\n"), s1, c(b"\n+\n"), q(L1, 7), c(b"\n@"), ids, c(b"\n"), s2, c(b"\n+\n"), q(L2, 11), c(b"\n")], axis=1).tobytes()


def pair_bytes(id1, s1, q1, id2, s2, q2, plus1=b"+", plus2=b"+", nl=b"\n"):
    return nl.join((id1, bytes(s1), plus1, q1, id2, bytes(s2), plus2, q2)) + nl


class Case:
    """segment_mb: MKT_RMDUP_SEGMENT_MB for the streaming runs (None: the default); pieces: the piece sizes of the streaming runs
    (0: the whole text in one push); golden: whether the reference build's output is pinned; small: few enough pairs for plain();
    marks: {ordinal: what sits there}"""

    def __init__(self, name, text, args=(), check=None, interleaved=False, segment_mb=None, pieces=(1 << 22,), golden=True, small=False, marks=None,
                 zero=()):
        self.name, self.text, self.args, self._check, self.interleaved = name, text, tuple(args), check, interleaved
        self.segment_mb, self.pieces, self.golden, self.small, self.marks, self.zero = segment_mb, pieces, golden, small, marks or {}, zero

    def check(self):
        """every case: Total = uniq + dup + discard, none of them zero unless the case is about that; then the case's own edge"""
        r = restated(self.name)
        total, uniq, dup, disc = r["stats"]
        assert total == uniq + dup + disc == len(lines_of(self.text)[1]) // 8 and total > 0, self.name
        for what, v in (("uniq", uniq), ("dup", dup), ("discard", disc)):
            assert (v == 0) == (what in self.zero), (self.name, what, v)
        return self._check(self, r) if self._check else {}

    def label(self, ordinal):
        o = int(ordinal)
        return "pair %d (batch %d, place %d)%s" % (o, o // BATCH, o % BATCH, ": " + self.marks[o] if o in self.marks else "")


GROUPS = {
    "key_window": ("kw_default", "kw_k0_s8_S8", "kw_k2_K4_s10_S14", "kw_s16_S16", "kw_s0_S16", "kw_s16_S0"),
    "chains": ("chains",),
    "one_key": ("one_key",),
    "batch": ("be_65535", "be_65536", "be_65537", "be_131073"),
    "copy": ("copy_1023", "copy_1024", "copy_1025"),
    "growth": ("grow_131072", "grow_131073", "grow_stream"),
    "carry": ("carry",),
    "ragged": ("rag_nonl",) + tuple("rag_extra%d" % k for k in range(1, 8)) + ("rag_crlf", "rag_discard_only"),
}
NAMES = tuple(n for g in GROUPS.values() for n in g)
SMALL_GROUPS = ("key_window", "one_key", "copy", "ragged")
KW_ARGS = {"kw_default": (), "kw_k0_s8_S8": ("-k", "0", "-s", "8", "-S", "8"), "kw_k2_K4_s10_S14": ("-k", "2", "-K", "4", "-s", "10", "-S", "14"),
           "kw_s16_S16": ("-s", "16", "-S", "16"), "kw_s0_S16": ("-s", "0", "-S", "16"), "kw_s16_S0": ("-s", "16", "-S", "0")}


def get(name):
    group = next(g for g, names in GROUPS.items() if name in names)
    if group not in _cache:
        built = globals()["_build_" + group]()
        assert tuple(c.name for c in built) == GROUPS[group]
        _cache[group] = {c.name: c for c in built}
    return _cache[group][name]


def restated(name):
    if ("r", name) not in _cache:
        c = get(name)
        _cache[("r", name)] = restate(c.text, c.args)
    return _cache[("r", name)]


def oracle(name):
    """(read 1, read 2, log) of oracle/krmdup_oracle.c, made once"""
    if ("o", name) not in _cache:
        c = get(name)
        _cache[("o", name)] = util.krmdup_oracle(c.text, **kwargs(c.args))
    return _cache[("o", name)]


# ---- 1. the key window
def _build_key_window():
    """Per argument set a few hundred pairs.  Every probe pair sits at one edge of the window and is followed later by a twin that
    has the same bases without the edge (a 'C' where the probe has a byte that is no base: the code a kernel that forgot the check
    would give it), so that kept / duplicate / discarded of both follows from the edge alone.  The pairs' ids name their edges."""
    out = []
    for name in GROUPS["key_window"]:
        args = KW_ARGS[name]
        h1, k1, h2, k2 = params(args)
        e1, e2 = h1 + k1, h2 + k2
        R = np.random.RandomState(5100 + 1000 * h1 + 100 * k1 + 10 * h2 + k2)
        phases, expect = ([], [], []), {}

        def clean():
            s1, s2 = bytearray(rand_bases(R, 30).tobytes()), bytearray(rand_bases(R, 27).tobytes())
            if k1 == 0:
                s1[h1] = ord("T")          # the letter at hskip1 is not part of the key: keep probe and twin in one bucket
            return [s1, s2]

        def put(phase, label, s1, s2, want, crlf=False):
            assert label not in expect
            expect[label] = want
            phases[phase].append((label, bytes(s1), bytes(s2), crlf))

        def both(label, x, t, ex, et, crlf=False):
            put(0, label, x[0], x[1], ex, crlf)
            put(1, label + ".twin", t[0], t[1], et)

        def retail(s, e):
            """the same read with other bases behind its window"""
            return s[:e] + bytearray(rand_bases(R, len(s) - e).tobytes())

        # read length exactly epos and epos - 1, for each mate
        for mate, e in ((0, e1), (1, e2)):
            t = clean()
            x = [bytearray(t[0]), bytearray(t[1])]
            x[mate] = x[mate][:e]
            both("len%d_epos" % (mate + 1), x, t, "kept", "dup")
            t = clean()
            x = [bytearray(t[0]), bytearray(t[1])]
            x[mate] = x[mate][:e - 1]
            both("len%d_epos-1" % (mate + 1), x, t, "disc", "kept")
        # a byte that is no base at the first and last place inside the window and just outside it
        for mate, h, e in ((0, h1, e1), (1, h2, e2)):
            for p in sorted({h, e - 1, h - 1, e} - {-1}):
                for ch in b"NX":
                    t = clean()
                    x = [bytearray(t[0]), bytearray(t[1])]
                    x[mate][p], t[mate][p] = ch, ord("C")
                    if h <= p < e:
                        want = ("disc", "kept")
                    elif mate == 0 and p == h1:                # keylen1 = 0: only the bucket letter
                        want = ("disc", "kept") if ch == ord("N") else ("kept", "kept")      # X: the T bucket, C: its own
                    else:
                        want = ("kept", "dup")
                    both("%s%d_at%d" % (chr(ch), mate + 1, p), x, t, *want)
        # the letter at hskip1
        for ch in b"ACGTacgtNnX":
            t = clean()
            x = [bytearray(t[0]), bytearray(t[1])]
            x[0][h1] = ch
            t[0][h1] = ch & ~0x20 if ch in b"ACGTacgt" else ord("C")
            t[0] = retail(t[0], max(e1, h1 + 1))
            if ch in b"ACGTt":
                want = ("kept", "dup")                         # 't' and 'T': both the T bucket
            elif ch in b"acg":
                want = ("kept", "kept")                        # same key, other bucket
            elif ch == ord("N") or k1 > 0:
                want = ("disc", "kept")
            else:
                want = ("kept", "kept")                        # 'n' / 'X' outside the key: the T bucket; the twin's 'C' its own
            both("first_%s" % chr(ch), x, t, *want)
            if ch == ord("a"):
                put(2, "first_a.again", retail(x[0], max(e1, h1 + 1)), x[1], "dup")
        # (K, 'A') and (K - 3, 'a'): one hash input, two members
        if k1 > 0:
            a = clean()
            a[0][h1] = ord("A")
            b = [bytearray(a[0]), bytearray(a[1])]
            b[0][h1] = ord("a")
            m, p = (1, e2 - 1) if k2 else (0, e1 - 1)
            a[m][p], b[m][p] = ord("G"), ord("C")
            put(0, "hash_K_A", a[0], a[1], "kept")
            put(1, "hash_K-3_a", b[0], b[1], "kept")
            put(2, "hash_K_A.again", retail(a[0], e1), retail(a[1], e2), "dup")
            put(2, "hash_K-3_a.again", retail(b[0], e1), retail(b[1], e2), "dup")
        # every key bit set, every key bit clear; the same behind a lower-case letter
        for base in b"GC":
            t = clean()
            t[0][h1] = base
            t[0][h1:e1], t[1][h2:e2] = bytes([base]) * k1, bytes([base]) * k2
            both("all_%s" % chr(base), t, (retail(t[0], max(e1, h1 + 1)), retail(t[1], e2)), "kept", "dup")
            x = [bytearray(t[0]), bytearray(t[1])]
            x[0][h1] |= 0x20
            both("all_%s_lower" % chr(base), x, (retail(x[0], max(e1, h1 + 1)), retail(x[1], e2)), "kept", "dup")
        # CRLF lines: the '\r' is the window's last byte (epos - 1 bases) or the first behind it (epos bases)
        for mate, h, e in ((0, h1, e1), (1, h2, e2)):
            t = clean()
            x = [bytearray(t[0]), bytearray(t[1])]
            x[mate] = x[mate][:e - 1]
            t[mate][e - 1] = ord("C")
            both("crlf%d_epos-1" % (mate + 1), x, t, *(("disc", "kept") if e > h else ("kept", "dup")), crlf=True)
            t = clean()
            x = [bytearray(t[0]), bytearray(t[1])]
            x[mate] = x[mate][:e]
            both("crlf%d_epos" % (mate + 1), x, t, "kept", "dup", crlf=True)
        # ordinary pairs around them
        fill = [clean() for _ in range(120)]
        for k, f in enumerate(fill):
            put(0, "fill%d" % k, f[0], f[1], "kept")
        for k in range(30):
            f = fill[int(R.randint(0, len(fill)))]
            put(1 + k % 2, "fill.dup%d" % k, retail(f[0], max(e1, h1 + 1)), retail(f[1], e2), "dup")
        recs = []
        for ph in phases:
            recs += [ph[i] for i in R.permutation(len(ph))]
        text = b"".join(pair_bytes(b"@" + lb.encode() + b"/1", s1, b"F" * len(s1), b"@" + lb.encode() + b"/2", s2, b"#" * len(s2), nl=b"\r\n" if crlf else b"\n")
                        for lb, s1, s2, crlf in recs)
        labels = [lb for lb, _a, _b, _c in recs]

        def check(case, r, labels=labels, expect=expect, k=(h1, k1, h2, k2)):
            kind = {0: "disc", 1: "dup"}
            for o, lb in enumerate(labels):
                assert kind.get(int(r["state"][o]), "kept") == expect[lb], (case.name, lb, int(r["state"][o]), expect[lb])
            at = {lb: o for o, lb in enumerate(labels)}
            h1, k1, h2, k2 = k
            bits = 2 * (k1 + k2)
            full = (1 << bits) - 1
            assert int(r["keys"][at["all_G"]]) == full and int(r["keys"][at["all_C"]]) == 0 and r["bucket"][at["all_C"]] == 1
            assert int(r["keys"][at["all_G_lower"]]) == full and r["bucket"][at["all_G_lower"]] == 3 and r["bucket"][at["all_G"]] == 2
            if k1 > 0:
                a, b = at["hash_K_A"], at["hash_K-3_a"]
                assert int(r["keys"][a]) - 3 == int(r["keys"][b]) and (r["bucket"][a], r["bucket"][b]) == (0, 3)
                assert slot(r["keys"][[a]], r["bucket"][[a]], (1 << 18) - 1) == slot(r["keys"][[b]], r["bucket"][[b]], (1 << 18) - 1)
            if k1 == 0:                                        # the letter is read at the line's end
                o = at["len1_epos"]
                assert r["bucket"][o] == 3 and lines_of(case.text)[2][8 * o + 1] - lines_of(case.text)[1][8 * o + 1] == h1
            return dict(pairs=len(labels), key_bits=bits)

        out.append(Case(name, text, args, check, interleaved=True, small=True, marks=dict(enumerate(labels))))
    return out


# ---- 2. probe chains
def crowd(R, mask, width, least, tail=0, tail_least=0, tries=1 << 22):
    """from `tries` random 32-base keys: at least `least` members (key, bucket) whose slots under mask fall in `width` consecutive
    slots well inside the table, and at least tail_least in its last `tail` slots (their chain wraps to slot 0)"""
    keys = np.unique(rand_keys(R, tries))
    b = top_bucket(keys)
    s = slot(keys, b, mask)
    cnt = np.bincount(s, minlength=mask + 1)
    win = np.convolve(cnt, np.ones(width, dtype=np.int64))[width - 1:len(cnt)]      # win[w] = members in [w, w + width)
    w = 4096 + int(np.argmax(win[4096:mask - 4096]))
    a = np.flatnonzero((s >= w) & (s < w + width))[:least + least // 3]
    z = np.flatnonzero(s > mask - tail)[:2 * tail_least] if tail else np.zeros(0, dtype=np.int64)
    assert len(a) >= least and len(z) >= tail_least
    return keys[a], w, keys[z]


def chain_facts(keys, mask, width):
    """members pairwise distinct, and how many of them one window of `width` consecutive slots holds"""
    b = top_bucket(keys)
    assert len(set(zip(keys.tolist(), b.tolist()))) == len(keys)
    s = np.sort(slot(keys, b, mask))
    return int(max(np.searchsorted(s, s + width) - np.arange(len(s))))


def _scatter(R, n, members, where, times):
    """places in `where` (a range of ordinals) for 1 .. times copies of every member -> (ordinals, member index per ordinal)"""
    reps = R.randint(1, times + 1, size=len(members))
    who = np.repeat(np.arange(len(members)), reps)
    at = where[0] + R.choice(where[1] - where[0], size=len(who), replace=False)
    return at, who


def _build_chains():
    R = np.random.RandomState(5201)
    mask = (1 << 18) - 1
    a, w, z = crowd(R, mask, 8, 48, tail=4, tail_least=8)
    members = np.concatenate([a, z])
    n = 20000
    keys = with_repeats(R, rand_keys(R, n), 0.2)
    at, who = _scatter(R, n, members, (0, n), 4)
    keys[at] = members[who]
    disc = R.rand(n) < 0.02
    disc[at] = False
    # one key behind 'A' and behind 'a' (buckets 0 and 3) whose two hash inputs, K and K + 3, fall on ONE slot: the second of them
    # meets the first's key there, and only the bucket tells them apart
    c = (rand_keys(R, 1 << 22) & U64((1 << 62) - 1)) | U64(1 << 62)
    both = np.unique(c[slot(c, 0, mask) == slot(c, 3, mask)])
    free = np.setdiff1d(np.arange(n), at)
    two_at = free[R.choice(len(free), size=4 * len(both), replace=False)].reshape(4, -1)      # upper, lower, upper again, lower again
    two_at.sort(axis=0)
    lower = np.zeros(n, dtype=bool)
    for row in range(4):
        keys[two_at[row]] = both
        lower[two_at[row]] = row % 2 == 1
    disc[two_at.ravel()] = False
    text = fixed_text(*reads(R, keys, 22, 22, lower=lower, discard=disc))
    marks = {int(o): "member %d of the %s" % (m, "8-slot crowd at slot %d" % w if m < len(a) else "crowd in the table's last 4 slots") for o, m in zip(at, who)}

    def check(case, r):
        assert r["stats"][0] == n <= 1 << 17
        assert (r["keys"][at] == members[who]).all() and (r["bucket"][at] == top_bucket(members)[who]).all()
        sa, sz = slot(a, top_bucket(a), mask), slot(z, top_bucket(z), mask)
        assert len(a) >= 48 and sa.min() >= w and sa.max() < w + 8 and chain_facts(a, mask, 8) >= 48
        assert len(z) >= 8 and sz.min() >= mask - 3 and chain_facts(members, mask, 8) >= 48
        times = np.bincount(who, minlength=len(members))
        assert times.min() >= 1 and times.max() <= 4 and (times > 1).sum() > 20
        firsts = {m: int(at[who == m].min()) for m in range(len(members))}
        assert all(r["state"][o] >= 2 for o in firsts.values()) and all(r["state"][o] == 1 for o, m in zip(at, who) if o != firsts[m])
        assert len(both) >= 4 and (slot(both, 0, mask) == slot(both, 3, mask)).all()
        assert (r["keys"][two_at] == both[None, :]).all() and (r["bucket"][two_at[0::2]] == 0).all() and (r["bucket"][two_at[1::2]] == 3).all()
        assert (r["state"][two_at[:2]] >= 2).all() and (r["state"][two_at[2:]] == 1).all()
        return dict(crowd=len(a), at=w, wrapping=len(z), one_slot_two_buckets=len(both))

    marks.update({int(o): "key %d behind 'A' and 'a' on one slot (%s)" % (k, ("upper", "lower", "upper again", "lower again")[row])
                  for row in range(4) for k, o in enumerate(two_at[row])})
    return [Case("chains", text, (), check, interleaved=True, marks=marks)]


# ---- 3. one key many times
def _build_one_key():
    R = np.random.RandomState(5301)
    n = 20000
    keys = rand_keys(R, n)
    k1, k2 = rand_keys(R, 2)
    k2 = (k2 & U64((1 << 62) - 1)) | U64(1 << 62)            # first base A
    where = 7 + R.permutation(n - 7)
    at1, at2 = where[:8000], where[8000:8100]
    keys[at1], keys[at2] = k1, k2
    lower = np.zeros(n, dtype=bool)
    lower[at2[::2]] = True
    disc = R.rand(n) < 0.02
    disc[at1] = disc[at2] = False
    text = fixed_text(*reads(R, keys, 22, 22, lower=lower, discard=disc))
    marks = {int(o): "the key that occurs 8000 times" for o in at1}
    marks.update({int(o): "the key with both cases of its first base (%s)" % ("lower" if lower[o] else "upper") for o in at2})

    def check(case, r):
        assert at1.min() > 0 and (r["keys"][at1] == k1).all() and (r["keys"][at2] == k2).all()
        assert (r["state"][at1] >= 2).sum() == 1 and r["state"][at1.min()] >= 2 and (r["state"][at1] == 1).sum() == 7999
        up, lo = at2[~lower[at2]], at2[lower[at2]]
        assert set(r["bucket"][up]) == {0} and set(r["bucket"][lo]) == {3}
        assert sorted(int(o) for o in at2 if r["state"][o] >= 2) == sorted([int(up.min()), int(lo.min())])
        return dict(first=int(at1.min()))

    return [Case("one_key", text, (), check, interleaved=True, small=True, marks=marks)]


# ---- 4. batch edges
def _batch0(R, n, last_first=True):
    """a mixed batch: repeats, scattered discards, 300 discarded pairs before its end and, last, a first occurrence"""
    keys = with_repeats(R, rand_keys(R, n), 0.2)
    disc = R.rand(n) < 0.01
    disc[n - 301:n - 1] = True
    if last_first:
        keys[n - 1] = rand_keys(R, 1)[0]
        disc[n - 1] = False
    return keys, disc


def _build_batch():
    out = []
    G = U64(3 << 62)

    def counts(case, r, pairs, only_g=(), empty=(), mixed=()):
        assert r["stats"][0] == pairs and len(r["kept"]) == (pairs + BATCH - 1) // BATCH
        for b in only_g:
            assert r["kept"][b][2] > 1000 and r["kept"][b][[0, 1, 3]].sum() == 0, (case.name, b, r["kept"][b])
        for b in empty:
            assert r["kept"][b].sum() == 0, (case.name, b)
        for b in mixed:
            assert r["kept"][b].min() > 1000, (case.name, b)
        return dict(kept=r["kept"].tolist())

    R = np.random.RandomState(5401)
    keys, disc = _batch0(R, 65535, last_first=False)
    out.append(Case("be_65535", fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), lambda c, r: counts(c, r, 65535, mixed=(0,)), segment_mb=1,
                    marks={65534: "the last pair, discarded"}))
    # one batch exactly, and all its survivors in bucket G
    R = np.random.RandomState(5402)
    keys, disc = _batch0(R, 65536)
    keys |= G
    out.append(Case("be_65536", fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), lambda c, r: counts(c, r, 65536, only_g=(0,)), segment_mb=1,
                    marks={65535: "the last pair of the only batch, a first occurrence"}))
    # the first occurrence that ends batch 0 and its twin, the whole of batch 1
    R = np.random.RandomState(5403)
    keys, disc = _batch0(R, 65536)
    keys, disc = np.append(keys, keys[-1]), np.append(disc, False)

    def check_37(c, r):
        assert r["state"][65535] >= 2 and r["state"][65536] == 1 and (r["state"][65235:65535] == 0).all()
        return counts(c, r, 65537, mixed=(0,), empty=(1,))

    out.append(Case("be_65537", fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), check_37, segment_mb=1,
                    marks={65535: "the last pair of batch 0, a first occurrence", 65536: "its twin, the only pair of batch 1"}))
    # batch 1 opens with that twin and keeps bucket G only; batch 2 is one duplicate
    R = np.random.RandomState(5404)
    k0, d0 = _batch0(R, 65536)
    u = R.rand(65536)
    src = np.flatnonzero(~d0)
    k1 = k0[src[R.randint(0, len(src), size=65536)]]                        # duplicates of batch 0, any bucket
    fresh = u < 0.35
    k1[fresh] = rand_keys(R, int(fresh.sum())) | G
    d1 = (u >= 0.35) & (u < 0.4)
    d1[65536 - 300:] = True
    k1[0], d1[0] = k0[-1], False
    last = np.flatnonzero(fresh & ~d1)[-1]
    keys, disc = np.concatenate([k0, k1, k1[[last]]]), np.concatenate([d0, d1, [False]])

    def check_73(c, r):
        assert r["state"][65535] >= 2 and r["state"][65536] == 1 and r["state"][131072] == 1 and r["state"][65536 + last] == 4
        assert (r["state"][65235:65535] == 0).all() and (r["state"][131072 - 300:131072] == 0).all()
        return counts(c, r, 131073, mixed=(0,), only_g=(1,), empty=(2,))

    out.append(Case("be_131073", fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), check_73, interleaved=True, segment_mb=1,
                    marks={65535: "the last pair of batch 0, a first occurrence", 65536: "its twin, the first pair of batch 1",
                           131072: "the only pair of batch 2, a duplicate"}))
    return out


# ---- 5. copy edges
def _build_copy():
    """1023 / 1024 / 1025 survivors (one workgroup of the copy less one, exactly, plus one) of every record shape, one of them
    with a read 1 of 70 000 bases"""
    out = []
    for want in (1023, 1024, 1025):
        R = np.random.RandomState(5500 + want)
        total = want + 200
        extra = np.sort(1 + R.choice(total - 1, size=200, replace=False))
        kind = np.zeros(total, dtype=np.int8)                   # 0 a new key, 1 a duplicate, 2 discarded
        kind[extra] = 1 + (R.rand(200) < 0.25)
        long_at, pos = None, 0
        uniq = []
        recs = []
        for i in range(total):
            ids = (b"", b"@", b"@" + bytes(R.randint(97, 123, size=299).astype(np.uint8)), b"@c%d" % i)
            id1, id2 = ids[i % 4], ids[(i // 4) % 4]
            L1, L2 = int(R.randint(21, 31)), int(R.randint(21, 31))
            if long_at is None and kind[i] == 0 and 500 <= -(pos + len(id1) + 1) % BATCH <= 4000:
                long_at, L1 = i, 70000                           # the read begins shortly before a 64 KiB chunk and ends behind it
            s1, s2 = bytearray(rand_bases(R, L1).tobytes()), bytearray(rand_bases(R, L2).tobytes())
            if kind[i] == 1:
                a, b = uniq[int(R.randint(0, len(uniq)))]
                s1[5:21], s2[5:21] = a, b
            elif kind[i] == 2:
                (s1 if i % 2 else s2)[5 + i % 16] = ord("N")
            else:
                uniq.append((bytes(s1[5:21]), bytes(s2[5:21])))
            plus1, plus2 = (b"+", b"+" + id1[1:], b"+ some text")[i % 3], (b"+", b"+x")[(i // 3) % 2]
            q1 = b"I" * (L1 if i % 5 else L1 // 2)
            q2 = b"5" * (L2 if i % 7 else 0)
            recs.append(pair_bytes(id1, s1, q1, id2, s2, q2, plus1, plus2))
            pos += len(recs[-1])
        text = b"".join(recs)

        def check(case, r, want=want, long_at=long_at):
            assert r["stats"][1] == want and r["state"][long_at] >= 2
            buf, st, en = lines_of(case.text)
            ln = en - st
            assert ln[8 * long_at + 1] == 70000 and ln[8 * long_at + 3] == 70000
            nl = np.flatnonzero(buf == 10)
            assert (np.bincount(nl >> 16, minlength=(len(buf) >> 16) + 1)[:len(buf) >> 16] == 0).any()      # a 64 KiB chunk without newline
            idl = np.concatenate([ln[0::8], ln[4::8]])
            assert {0, 1, 300} <= set(idl.tolist()) and (ln[2::8] > 1).any() and (ln[6::8] > 1).any()
            assert (ln[3::8] < ln[1::8]).any() and (ln[7::8] == 0).any()
            return dict(survivors=want, bytes=len(case.text))

        out.append(Case("copy_%d" % want, text, (), check, interleaved=True, small=True, marks={long_at: "the pair with the 70 000-base read 1"}))
    return out


# ---- 6. growth at its step
def _build_growth():
    out = []
    for n in (131072, 131073):
        R = np.random.RandomState(5600 + n % 10)
        keys = with_repeats(R, rand_keys(R, n), 0.25)
        disc = R.rand(n) < 0.01
        keys[n - 1], disc[n - 1] = keys[np.flatnonzero(~disc)[0]], False      # the last pair: a duplicate of the first live one

        def check(case, r, n=n):
            assert r["stats"][0] == n and r["state"][n - 1] == 1
            return dict(pairs=n, room_for=1 << 17)

        out.append(Case("grow_%d" % n, fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), check, segment_mb=1,
                        marks={n - 1: "the last pair (ordinal 2^17%s), a duplicate" % (" - 1" if n == 131072 else "")}))
    # three batches and five pairs through segments: the table doubles to 2^19 slots when the third batch arrives
    R = np.random.RandomState(5603)
    n = 3 * BATCH + 5
    mask = (1 << 19) - 1
    members, w, _z = crowd(R, mask, 8, 32)
    half = len(members) // 2
    keys = with_repeats(R, rand_keys(R, n), 0.2)
    disc = R.rand(n) < 0.01
    early = R.choice(2 * BATCH, size=half, replace=False)                     # first seen while the table has 2^18 slots
    late = 2 * BATCH + R.choice(20000, size=len(members) - half, replace=False)
    first_at = np.concatenate([early, late])
    at, who = _scatter(R, n, members, (2 * BATCH + 20000, n), 3)
    keys[first_at] = members
    keys[at] = members[who]
    disc[first_at] = disc[at] = False
    marks = {int(o): "member %d of the crowd at slot %d of 2^19, first seen %s the table grows" % (m, w, "before" if m < half else "after")
             for o, m in zip(np.concatenate([first_at, at]), np.concatenate([np.arange(len(members)), who]))}

    def check(case, r):
        assert r["stats"][0] == n
        assert (r["keys"][first_at] == members).all() and (r["keys"][at] == members[who]).all()
        assert len(members) >= 32 and chain_facts(members, mask, 8) >= 32 and chain_facts(members, mask >> 1, 8) >= 32
        assert half >= 16 and early.max() < 2 * BATCH <= late.min() and at.min() >= 2 * BATCH
        assert (r["state"][first_at] >= 2).all() and (r["state"][at] == 1).all()
        return dict(crowd=len(members), at=w)

    out.append(Case("grow_stream", fixed_text(*reads(R, keys, 22, 22, discard=disc)), (), check, interleaved=True, segment_mb=1, pieces=(1 << 22, 999983),
                    marks=marks))
    return out


# ---- 7. the carry through the temporary
def _build_carry():
    R = np.random.RandomState(5701)
    na, nb = BATCH, 30000
    ka = with_repeats(R, rand_keys(R, na), 0.2)
    da = R.rand(na) < 0.02
    kb = rand_keys(R, nb)
    rep = R.rand(nb) < 0.4
    src = np.flatnonzero(~da)
    kb[rep] = ka[src[R.randint(0, len(src), size=int(rep.sum()))]]
    db = R.rand(nb) < 0.02
    a = fixed_text(*reads(R, ka, 21, 21, discard=da))
    b = fixed_text(*reads(R, kb, 150, 150, discard=db), first=na)

    def check(case, r):
        assert r["stats"][0] == na + nb and len(b) > len(a) > 1 << 20 and case.text[:len(a)].count(b"\n") == 8 * na
        return dict(first_segment=len(a), left=len(b))

    return [Case("carry", a + b, (), check, segment_mb=1, pieces=(0, 999983), marks={na: "the first pair of 150-base reads"})]


# ---- 8. ragged ends
def _build_ragged():
    R = np.random.RandomState(5801)
    n = 300
    keys = with_repeats(R, rand_keys(R, n), 0.3)
    disc = R.rand(n) < 0.05
    keys[n - 1], disc[n - 1] = rand_keys(R, 1)[0], False                      # the last pair stays
    base = fixed_text(*reads(R, keys, 30, 30, discard=disc))
    more = fixed_text(*reads(R, rand_keys(R, 1), 30, 30), first=n).split(b"\n")

    def check_last(c, r):
        assert r["stats"][0] == n and r["state"][n - 1] >= 2
        return {}

    out = [Case("rag_nonl", base[:-1], (), check_last, interleaved=True, small=True, marks={n - 1: "the last pair, its last line without newline"})]
    for k in range(1, 8):
        out.append(Case("rag_extra%d" % k, base + b"\n".join(more[:k]) + b"\n", (), check_last, interleaved=True, golden=False, small=True))
    out.append(Case("rag_crlf", base.replace(b"\n", b"\r\n"), (), check_last, interleaved=True, small=True))
    s1, s2 = reads(R, rand_keys(R, 200), 30, 30, discard=np.ones(200, dtype=bool))
    body = fixed_text(s1, s2).split(b"\n")
    for r in range(0, 200, 3):                                                # a third of them: too short instead
        body[8 * r + 1] = body[8 * r + 1][:20].replace(b"N", b"A")
    out.append(Case("rag_discard_only", b"\n".join(body), (), lambda c, r: {}, interleaved=True, small=True, zero=("uniq", "dup")))
    return out
