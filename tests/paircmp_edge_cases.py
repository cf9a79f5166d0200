"""Directed inputs for the pair-level concordance (mkt_paircmp.hip, microcket_amd.PairCompare, bin/pairscmp) at the places where its
kernels work in words, workgroups, key bits, lanes and line counts.  tests/paircmp_inputs.py is organised around the rules of the
definition; the cases here are organised around the mechanics.  Plain Python, deterministic, nothing of the package under test.

What the kernels do at these places:
 * pc_load8 / pc_bytes_eq compare two byte strings eight bytes a step from any offset (two aligned loads and a shift per operand, a
   masked last word).  They serve the ids in the join, the two chromosome names of a line (cis or trans) and the straight and the
   swapped test of a claimed pair.  An operand's alignment is its offset in the joined text (A, then B) modulo 8.
 * k_pc_join classifies a sorted record from its two neighbours, 256 records a workgroup (SWG), so the value of an id (its last A
   line) and its claimant (the id's first B line) can lie in two workgroups.
 * a key narrowed to hash_bits bits is sorted over (hash_bits + 3) / 4 * 4 bits; width 32 takes the branch without the shift.
 * k_pc_emit copies every part of an output line with 16 lanes (kPcCopyLanes).
 * k_pc_parse reports the smallest refused line over all its workgroups through an atomicMin.

A case is a dict: name, family, a and b (bytes), dist (None or the string given to the script), hash_bits (the widths to run), golden
(inside the pinned domain, so tests/golden/paircmp_edges_golden.json holds what the reference's script printed), refused (None or
(side, line)), and for some families a few numbers the tests compare with what they work out from the texts (k, shape).
tests/test_paircmp_edges_host.py proves from the texts that every case sits at the edge it is named for.

Not reachable from here: two different ids with one full 96-bit key cannot be made, so at hash_bits 0 the host resolution of a
collision is exercised only through the narrowed widths."""
import paircmp_inputs as pi

D = 200                                            # the default distance
SWG = 256                                          # records per workgroup of the parse and the join (mkt_blockscan.h)
LANES = 16                                         # kPcCopyLanes
ALPHA = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
NAME_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25)
NAME_DIFFS = (0, 6, 7, 8, -1)                      # the byte at which two names of one length differ (-1: the last)
ID_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 24)
ID_DIFFS = (0, 7, 8, -1)
EDGE_KS = (255, 256, 257, 511, 512, 513)
COUNT_TOTALS = (255, 256, 257)
EMIT_LENGTHS = (15, 16, 17, 31, 32, 33, 47, 48, 49)
EMIT_I_MIN = 18                                    # "I\t" "\t" four empty-named fields twice "\tvs\t" "\n": no I line is shorter
EMIT_PARTS = (15, 16, 17, 31, 32, 33)              # lengths of the three copied parts of an I line
KEY_WIDTHS = (2, 5, 13, 31, 32)
PREFIX_PAIR = (b"ABCDEFGH", b"ABCDEFGH\x01")       # a proper prefix; the longer name's next byte looks like a tab in the same word
NAME_REPS = 8                                      # every pairing of two names meets every alignment of its first operand


def _b(x):
    return x if isinstance(x, bytes) else str(x).encode()


def row(*fields):
    """one line without its newline"""
    return b"\t".join(_b(f) for f in fields)


def text(rows, final_newline=True):
    t = b"".join(r + b"\n" for r in rows)
    return t if final_newline or not t else t[:-1]


def differing(base, diffs):
    """the strings of base's length that differ from it only at one of the bytes `diffs` (those that exist), in the byte's order"""
    at = sorted({d % len(base) for d in diffs if -len(base) <= d < len(base)}) if base else []
    return [base[:p] + base[p:p + 1].lower() + base[p + 1:] for p in at]


def name_pairings():
    """(X, Y): every length with itself and with the equal-length names that differ at one byte; the proper prefix both ways"""
    out = []
    for n in NAME_LENGTHS:
        base = ALPHA[:n]
        out.append((base, base))
        out += [(base, v) for v in differing(base, NAME_DIFFS)]
    return out + [PREFIX_PAIR, PREFIX_PAIR[::-1]]


class Aligned:
    """The lines of one side, each started at a chosen offset modulo 8 of the joined text: the line before gets one more field of
    the needed length (a comment line goes in front of the first line)."""

    def __init__(self, base=0):
        self.rows, self.at = [], base

    def add(self, core, start_mod=None):
        if start_mod is not None:
            k = (start_mod - self.at) % 8
            if k and self.rows and not self.rows[-1].startswith(b"#"):
                self.rows[-1] += b"\t" + b"p" * (k - 1)
                self.at += k
            elif k:
                k += 8 if k < 2 else 0
                self.rows.append(b"#" + b"c" * (k - 2))
                self.at += k
        start = self.at
        self.rows.append(core)
        self.at += len(core) + 1
        return start


def _padded_id(tag, at, want):
    """an id that starts with tag and ends so that the byte behind its tab lies at `want` modulo 8 when the line starts at `at`"""
    return tag + b"x" * ((want - 1 - at - len(tag)) % 8)


def _names():
    """Every pairing of name_pairings() in three roles, NAME_REPS times each with other alignments:
    ids c..: X is c1 and Y is c2 of one line (cis or trans), the same line on both sides, |p2 - p1| at the edges of the distribution;
    ids s..: X is A's c1 and Y is B's c1; the positions agree, the second names are equal and the swap fails on its positions;
    ids w..: X is A's c1 and Y is B's c2; the same the other way round.
    The first operand lies at r modulo 8 and the second at (3 r + q) modulo 8 for pairing q and repetition r, so every role meets all 64
    pairs of alignments and every pairing all eight alignments of either operand.  Behind equal names stand positions whose first
    digits differ."""
    pairs = name_pairings()
    A = Aligned(0)
    plan = []                                                        # what B needs: (role, id, X, Y, alignment of B's operand, number)
    edges = (0, 999, 1000, 10000, 10001)
    n = 0
    for q, (X, Y) in enumerate(pairs):
        for r in range(NAME_REPS):
            ta, tb = r, (3 * r + q) % 8
            d = edges[n % 5]
            lo, hi = str(20000 - d).encode(), b"20000"
            p1, p2 = (hi, lo) if n % 2 == 0 else (lo, hi)
            rid = _padded_id(b"c%d." % n, A.at, ta)
            p1 = b"0" * ((tb - ta - len(X) - 2 - len(p1)) % 8) + p1  # leading zeros move c2
            A.add(row(rid, X, p1, Y, p2))
            plan.append((b"c", rid, X, Y, p1, p2))
            rid = _padded_id(b"s%d." % n, A.at, ta)
            A.add(row(rid, X, 1000, b"Zfill", 5000000))
            plan.append((b"s", rid, X, Y, tb, None))
            rid = _padded_id(b"w%d." % n, A.at, ta)
            A.add(row(rid, X, 1000, b"Zfill", 5000000))
            plan.append((b"w", rid, X, Y, tb, None))
            n += 1
    a = text(A.rows)
    B = Aligned(len(a))
    for role, rid, X, Y, u, v in reversed(plan):
        if role == b"c":
            B.add(row(rid, X, u, Y, v))
        elif role == b"s":
            B.add(row(rid, Y, 999, b"Zfill", 5000000), (u - len(rid) - 1) % 8)
        else:
            core = row(rid, b"Zfill", 5000001, Y, 999)
            B.add(core, (u - core.index(Y + b"\t999")) % 8 if Y else (u - len(core) + 4) % 8)
    return a, text(B.rows)


def _ids_words():
    """ids of every length and, for each, the equal-length ids that differ at one byte: in turn consistent, discordant, in A only, in B
    only, so that two ids taken for one change a class; B in the reverse order"""
    ids = []
    for n in ID_LENGTHS:
        base = ALPHA[:n]
        ids += [base] + differing(base, ID_DIFFS)
    v = ("chr1", 1000, "chr2", 2000)
    w = ("chr1", 7000, "chr2", 2000)
    a, b = [], []
    for k, rid in enumerate(ids):
        if k % 4 != 3:
            a.append(row(rid, *v))
        if k % 4 != 2:
            b.append(row(rid, *(w if k % 4 == 1 else v)))
    return text(a), text(b[::-1])


def _with_comments(rows, tag):
    out = []
    for k, r in enumerate(rows):
        if k % 3 == 0 or len(rows) < 3:
            out.append(b"#%s %d" % (tag, k))
        out.append(r)
    return out + [b"#the last line of %s" % tag]


def _edge(k, shape):
    """one id.  a_long: k lines in A, the last of them the value, and two in B, the first of them the claimant; b_long: one line in A
    and k in B.  The claimant is 199 from the value for an even k (consistent) and 200 for an odd k (discordant: the bound is strict)."""
    val = ("c", 1000, "c", 2000)
    claim = ("c", 1199 if k % 2 == 0 else 1200, "c", 2000)
    if shape == "b_long":
        a = [row("h", *val)]
        b = [row("h", *claim)] + [row("h", "c", 1000 + j % 7, "c", 2000) for j in range(k - 1)]
    else:
        a = [row("h", "c", 9000 + j, "c", 2000) for j in range(k - 1)] + [row("h", *val)]
        b = [row("h", *claim), row("h", *val)]
    if shape == "comments":
        a, b = _with_comments(a, b"A"), _with_comments(b, b"B")
    return text(a), text(b)


def _plain(n, first=0, moved=False):
    """n lines with ids r<first> ..; with moved every even line is 500 away (discordant against the unmoved one)"""
    return [row(f"r{j}", "chr1", 100 * j + (500 if moved and j % 2 == 0 else 0), "chr2" if j % 3 else "chr1", 100 * j + 1500 * (j % 9))
            for j in range(first, first + n)]


def _count(na, nb):
    return text(_plain(na)), text(_plain(nb, moved=True))


def _emit():
    """A-only, B-only and I lines of the lengths in EMIT_LENGTHS (no I line has fewer than EMIT_I_MIN bytes), I lines whose three
    copied parts -- the id with its tab, A's four fields, B's four fields -- have the lengths in EMIT_PARTS, lines of five fields
    against lines of twelve, a fifth field before the newline against one before a tab; the three kinds alternate in B's order."""
    a_only, b_only, pairs = [], [], []                                # pairs: (A line, B line)
    for n in EMIT_LENGTHS:
        a_only.append(row((b"a%d" % n).ljust(n - 11, b"x"), "c", 1, "c", 2))               # "A\t" + id + 8 + "\n"
        b_only.append(row((b"b%d" % n).ljust(n - 11, b"x"), "c", 1, "c", 2, "+", "-"))
        if n >= EMIT_I_MIN + 4:
            rid = (b"i%d" % n).ljust(n - 22, b"x")                                         # "I\t" + id + "\t" + 7 + "\tvs\t" + 7 + "\n"
            pairs.append((row(rid, "c", 1, "c", 2), row(rid, "d", 1, "c", 2)))
    for n in EMIT_PARTS:
        rid = (b"s%d" % n).ljust(n - 1, b"x")                                              # the id and its tab: n bytes
        pairs.append((row(rid, "c", 1, "c", 2, "+"), row(rid, "d", 1, "c", 2)))
        pairs.append((row(b"ta%d" % n, b"C" * (n - 6), 1, "c", 2), row(b"ta%d" % n, "d", 1, "c", 2, "-")))      # A's four fields: n bytes
        pairs.append((row(b"tb%d" % n, "c", 1, "c", 2), row(b"tb%d" % n, b"D" * (n - 6), 1, "c", 2)))           # B's four fields: n bytes
    more = ("+", "-", "a", "b", "c", "d", "e")
    pairs.append((row("f5_12", "c", 1, "c", 2), row("f5_12", "c", 1, "d", 2, *more)))
    pairs.append((row("f12_5", "c", 1, "c", 2, *more), row("f12_5", "c", 1, "d", 2)))
    pairs.append((row("f5_12ok", "c", 1, "c", 2), row("f5_12ok", "c", 1, "c", 2, *more)))
    pairs.append((row("f12_5ok", "c", 1, "c", 2, *more), row("f12_5ok", "c", 1, "c", 2)))
    pairs.append((row("end_tab", "c", 1, "c", 222), row("end_tab", "c", 1, "c", 2, "")))   # ... 222\n against ... 2\t\n
    pairs.append((row("tab_end", "c", 1, "c", 2, ""), row("tab_end", "c", 1, "c", 222)))
    a, b = [], []
    for k, (ra, rb) in enumerate(pairs):
        a.append(ra)
        b.append(rb)
        if k < len(a_only):
            a.append(a_only[k])
            b.append(b_only[k])
    assert len(pairs) >= len(a_only)
    return text(a), text(b)


def _refused_cases():
    out = []
    short, letter, top = row("bad", "chr1", 5), row("bad", "chr1", "12a", "chr1", 6), row("bad", "chr1", 1, "chr1", 1 << 31)

    def put(name, na, nb, bad_a, bad_b, want):
        a, b = _plain(na), _plain(nb)
        for k, r in bad_a:
            a[k - 1] = r
        for k, r in bad_b:
            b[k - 1] = r
        out.append(dict(name=name, a=text(a), b=text(b), refused=want))

    put("two_in_b", 800, 800, [], [(10, short), (700, letter)], ("B", 10))
    put("two_in_a", 800, 800, [(700, short), (10, top)], [], ("A", 10))
    put("a600_b3", 800, 800, [(600, letter)], [(3, short)], ("A", 600))
    put("joined_255", SWG, 300, [(SWG, short)], [], ("A", SWG))                             # A has 256 lines: the last of the first workgroup,
    put("joined_256", SWG, 300, [], [(1, short)], ("B", 1))                                 # the first of the second,
    put("joined_257", SWG, 300, [], [(2, short)], ("B", 2))                                 # and the one behind it
    put("both_workgroups_of_b", SWG - 1, 600, [], [(300, short), (2, letter)], ("B", 2))
    for k, (name, r) in enumerate((
            ("pos_20_digits", row("bad", "chr1", "99999999999999999999", "chr1", 6)),
            ("pos_small_mod_2_32", row("bad", "chr1", 6, "chr1", "4294967301")),
            ("pos_plus", row("bad", "chr1", "+5", "chr1", 6)),
            ("pos_minus", row("bad", "chr1", 6, "chr1", "-5")),
            ("pos_blank_first", row("bad", "chr1", " 5", "chr1", 6)),
            ("pos_blank_last", row("bad", "chr1", 6, "chr1", "5 ", "+")),
            ("cr_behind_the_fifth_field", row("bad", "chr1", 6, "chr1", "5\r")),
            ("four_tabs_only", b"\t\t\t\t"),
            ("empty_fifth_field", row("bad", "chr1", 5, "chr1", "")),
            ("tabs_2000", b"\t" * 2000))):
        at = 21 + k
        if k % 2:
            put(name, 40, 40, [(at, r)], [], ("A", at))
        else:
            put(name, 40, 40, [], [(at, r)], ("B", at))
    return out


def _case(name, family, a, b, dist=None, hash_bits=(0,), golden=True, refused=None, **more):
    return dict(name=name, family=family, a=a, b=b, dist=dist, hash_bits=list(hash_bits), golden=golden, refused=refused, **more)


def _build():
    out = []
    na, nb = _names()
    out.append(_case("names", "names", na, nb, hash_bits=(0, 3)))
    out.append(_case("ids_words", "ids_words", *_ids_words(), hash_bits=(0, 1, 2)))
    for shape in ("a_long", "comments", "b_long"):
        for k in EDGE_KS:
            out.append(_case(f"edge_{shape}_{k}", "run_at_block_edge", *_edge(k, shape), hash_bits=(0, 5), k=k, shape=shape))
    for n in COUNT_TOTALS:
        for tag, ca in (("0", 0), ("n", n), ("1", 1), ("128", 128)):
            out.append(_case(f"count_{n}_{tag}", "line_counts", *_count(ca, n - ca), hash_bits=(0, 3), total=n))
    comments = [b"## pairs format v1.0", b"#columns: readID chr1 pos1 chr2 pos2", b"#"]
    data = _plain(5)
    for name, a, b in (("comments_both", text(comments), text(comments[::-1])),
                       ("comments_a_data_b", text(comments), text(data)),
                       ("data_a_comments_b", text(data), text(comments)),
                       ("empty_a_b_unterminated", b"", text(data, final_newline=False)),
                       ("a_unterminated_empty_b", text(data, final_newline=False), b""),
                       ("one_hash", b"#", b"")):
        out.append(_case(name, "line_counts", a, b, hash_bits=(0, 3), total=None))
    out.append(_case("emit_lengths", "emit_lengths", *_emit(), hash_bits=(0, 3)))
    empty = row("", "c", 1, "c", 2)
    for name, a, b in (("empty_id_a_only", [empty, row("x", "c", 1, "c", 2)], [row("x", "c", 1, "c", 2)]),
                       ("empty_id_b_only", [row("x", "c", 1, "c", 2)], [row("x", "c", 1, "c", 2), empty]),
                       ("empty_id_discordant", [row("x", "c", 1, "c", 2), empty], [row("", "d", 1, "c", 2), row("x", "c", 1, "c", 2)])):
        out.append(_case(name, "emit_lengths", text(a), text(b), hash_bits=(0, 3)))
    for name, gen in (("repeats", dict(kind="repeats", seed=5)), ("lines", dict(kind="lines", seed=12)), ("mixed_3000", dict(kind="mixed", seed=13, n=3000))):
        a, b = pi.make(gen)
        out.append(_case("widths_" + name, "key_widths", a, b, hash_bits=KEY_WIDTHS))
    for c in _refused_cases():
        out.append(_case("refused_" + c["name"], "refused", c["a"], c["b"], hash_bits=(0, 2), golden=False, refused=c["refused"]))
    for d in (1 << 31, (1 << 32) - 1):
        out.append(_case(f"max_dist_{d}", "max_dist", na, nb, dist=str(d), golden=False))
    return out


_cache = []


def cases():
    """every case, made once and never modified"""
    if not _cache:
        _cache.extend(_build())
    return _cache


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def accepted():
    return [c for c in cases() if c["refused"] is None]


def refused():
    return [c for c in cases() if c["refused"] is not None]
