"""The .pairs sorter (mkt_sort.hip) at the constants where it changes route, byte for byte against the system's GNU sort
(LANG=C sort -k2,2d -k4,4d -k3,3n -k5,5n, util.gnu_sort), as tests/test_gpu_sort.py does for ordinary data:

  runs of equal keys   <= 48 lines in one thread (k_tie_small), 49 .. 2048 by one workgroup (k_tie_big), longer ones by the whole
                       chip (k_tie_huge); the list of long runs holds nl / 49 + 1 heads
  radix passes         256-record sub-tiles, tiles of 8192 records, at most 1024 workgroups (records per workgroup grow beyond
                       8192 * 1024 lines); the gather takes 2048 lines per workgroup
  key widths           4-bit passes over the rank bits of the chromosome names (steps at 16, 256, 4096 distinct dictionary
                       forms), at most 8192 names of at most 62 bytes, positions of 32 bits
  line index           64 KiB of text per workgroup, 16 KiB per wave, 16 bytes per lane and round; the text buffer starts at
                       64 MiB and doubles

The one case above the workgroup cap (8192 * 1024 + 1 lines, 226 MB) is checked against numpy's lexsort of the same rows, which
was itself checked equal to GNU sort when the test was written: GNU sort needs a quarter of a minute for it.  tests/sortdef.py
(the same order in Python, proved against GNU sort by tests/test_sortdef_host.py) words every failure: the first differing line
and both keys.

Not covered: more than kHugeCap = 4096 runs of more than 2048 lines each (MKT_E_CAPACITY).  That needs over 8 million tied lines
and O(L^2) whole-line comparisons per run; it is left out on purpose."""
import random
import time

import numpy as np
import pytest

import microcket_amd as m
import sortdef
import util

pytestmark = pytest.mark.gpu

ALNUM = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789"


def gpu_sort(data: bytes) -> bytes:
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    with m.PairsSorter(0) as s:
        for k in range(0, len(data), 1 << 20):                     # fed in pieces, as tests/test_gpu_sort.py does
            s.add(data[k:k + (1 << 20)])
        return s.sort()


def check(data: bytes, tmp_path):
    got = gpu_sort(data)
    want = util.gnu_sort(data if data.endswith(b"\n") else data + b"\n", tmp_path)
    assert got == want, sortdef.explain(got, want)


def text(lines) -> bytes:
    return b"".join(l + b"\n" for l in lines)


# ---- runs of equal keys ----------------------------------------------------------------------------------------------
def lines_for(key, L, seed):
    """L lines with the same (chr1, chr2, pos1, pos2) (fields as bytes), in shuffled order: only the whole-line comparison orders
    them.  Mixed in one run: read names that are prefixes of one another, a 5-field line that is a prefix of a 7-field line, bytes
    >= 0x80 in names (the comparison is unsigned), two fully identical lines, lines that differ in their last byte only after a
    200-byte common read name.  A run shorter than the ten special lines takes as many of them as fit."""
    c1, c2, p1, p2 = key
    rnd = random.Random(seed)
    mid = b"\t" + b"\t".join((c1, p1, c2, p2))

    def line(name, strands=(b"+", b"-")):
        return name + mid + (b"\t" + b"\t".join(strands) if strands else b"")

    tag = b"s%d." % seed
    long_name = tag + b"L" * (200 - len(tag))
    special = [
        [line(tag + b"q1"), line(tag + b"q12")],                                    # a name that is a prefix of another
        [line(tag + b"f", None), line(tag + b"f")],                                  # five fields, a prefix of seven
        [line(tag + b"q\xc3\xa9"), line(tag + b"\xff1")],                            # sort after every ASCII name: unsigned bytes
        [line(tag + b"dup", (b"-", b"+"))] * 2,                                      # identical lines
        [line(long_name, (b"+", b"-")), line(long_name, (b"+", b"+"))],              # the last byte decides, 200 bytes in
    ]
    r = seed % len(special)
    out = [l for g in special[r:] + special[:r] for l in g][:L]
    for n, v in enumerate(rnd.sample(range(20, 20 + 10 * L), L - len(out))):         # distinct numbers: q20, q203, q2031 ... prefixes again
        if n % 7 == 3:
            name = tag + b"q\x80%d" % v
        elif n % 61 == 5:
            name = long_name[:-1] + b"%d" % v
        else:
            name = tag + b"q%d" % v
        out.append(line(name, None if n % 11 == 4 else (rnd.choice((b"+", b"-")), rnd.choice((b"+", b"-")))))
    assert len(out) == L
    rnd.shuffle(out)
    return out


def singletons(n, seed):
    """n lines with a key of their own each (pos1 is 100000 + a distinct number), over 25 chromosome names"""
    rnd = random.Random(seed)
    names = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrUn_KI270742v1", b"chrM"]
    p1 = rnd.sample(range(100000, 100000 + 20 * n), n)
    return [b"u%d\t%s\t%d\t%s\t%d\t%s\t%s" % (i, rnd.choice(names), p1[i], rnd.choice(names), rnd.randrange(1, 1 << 28), rnd.choice((b"+", b"-")), rnd.choice((b"+", b"-")))
            for i in range(n)]


RUN_LENGTHS = [2, 47, 48, 49, 50, 255, 256, 257, 1023, 2047, 2048, 2049, 2050]


def runs_input(first=None, last=None):
    """One run of every length in RUN_LENGTHS, each under its own key (pos1 < 100000: no singleton shares it), and 5000 singleton
    lines, all interleaved by one fixed permutation.  first / last: the run length whose key is made the smallest / the greatest
    of the whole input ("0_first" sorts before, "zz.last" after every chr... name), so that this run starts at record 0 / ends at the
    last record."""
    lines = singletons(5000, 4242)
    for n, L in enumerate(RUN_LENGTHS):
        c1 = b"0_first" if L == first else b"zz.last" if L == last else b"chr%d" % (1 + n % 22)
        lines += lines_for((c1, b"chr_%d" % (22 - n), b"%d" % (1000 * n + 7), b"5000"), L, 100 + n)
    random.Random(77).shuffle(lines)
    return text(lines)


@pytest.mark.parametrize("first,last", [(None, None), (49, 2048), (2048, 49)], ids=["as_is", "49_first_2048_last", "2048_first_49_last"])
def test_run_lengths(tmp_path, first, last):
    """(a) runs at 48 / 49 (thread -> workgroup) and 2048 / 2049 (workgroup -> chip), and a run that ends at the last record"""
    check(runs_input(first, last), tmp_path)


def test_200_runs_of_49_fill_the_long_run_list(tmp_path):
    """(b) 9800 lines, nothing but runs of 49: the list of long runs has 9800 / 49 + 1 = 201 places and 200 are used"""
    lines = []
    for k in range(200):
        lines += lines_for((b"chr%d" % (k % 20), b"chr.%d" % (k // 20), b"%d" % (1 + k % 3), b"%d" % (k % 7)), 49, 1000 + k)
    assert len({sortdef.key(l)[:4] for l in lines}) == 200
    random.Random(78).shuffle(lines)
    check(text(lines), tmp_path)


def test_64_runs_of_2048(tmp_path):
    """(b) 64 workgroups of k_tie_big, each with a run of the greatest length it takes"""
    lines = []
    for k in range(64):
        lines += lines_for((b"chr%d" % (k % 8), b"chr%d" % (k // 8), b"%d" % (1 << (k % 32)), b"%d" % ((1 << 32) - 1 - k)), 2048, 2000 + k)
    random.Random(79).shuffle(lines)
    check(text(lines), tmp_path)


# ---- line counts --------------------------------------------------------------------------------------------------------
def mixed_lines(nl, seed):
    """nl lines of 10 to 300 bytes (with the newline); keys random over 30 names, about one line in twenty repeats an earlier key"""
    rnd = random.Random(seed)
    names = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY", b"chrM", b"chrUn_GL000195v1", b"chrUn.GL000195v1", b"chr1_KI270706v1_random", b"c", b"EBV"]
    keys, out = [], []
    for i in range(nl):
        if keys and rnd.random() < 0.05:
            k = rnd.choice(keys)
        else:
            k = (rnd.choice(names), rnd.choice(names), rnd.randrange(0, 250_000_000), rnd.randrange(0, 250_000_000))
        keys.append(k)
        if i % 16 == 0:                                            # the shortest line there is: 9 bytes and the newline
            k = (b"c", b"c", k[2] % 10, k[3] % 10)
            keys[-1] = k
            out.append(b"%s\tc\t%d\tc\t%d" % (ALNUM[i // 16 % 62:i // 16 % 62 + 1], k[2], k[3]))
            continue
        rest = b"\t%s\t%d\t%s\t%d\t%s\t%s" % (k[0], k[2], k[1], k[3], rnd.choice((b"+", b"-")), rnd.choice((b"+", b"-")))
        want = rnd.randrange(len(rest) + 2, 301) if i % 5 else 300
        name = b"r%d" % i
        name = (name + b":" + bytes(rnd.choices(ALNUM, k=max(0, want - 2 - len(rest) - len(name)))))[:want - 1 - len(rest)]
        out.append(name + rest)
        assert 10 <= len(out[-1]) + 1 <= 300
    return out


# the steps: radix sub-tile 256, gather 2048 lines per workgroup, radix tile 8192 (one workgroup -> two -> three)
LINE_COUNTS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16385]


@pytest.mark.parametrize("nl", LINE_COUNTS)
def test_line_counts(tmp_path, nl):
    """(c)"""
    lines = mixed_lines(nl, 3000 + nl)
    assert len(lines) == nl and min(map(len, lines)) == 9 and (nl < 8 or max(map(len, lines)) == 299)
    check(text(lines), tmp_path)


# ---- above the cap of 1024 workgroups in the radix passes ---------------------------------------------------------------------
def test_more_than_8192_lines_per_workgroup(capsys):
    """(d) 8192 * 1024 + 1 lines: the radix passes' workgroups take 8193 records each (9 sub-tiles of 256 and one record), the text
    (226 MB, fed in 1 MiB pieces) outgrows the sorter's first 64 MiB twice.  Every (pos1, pos2) is unique: no tie path runs, the
    order is the radix sort's alone.  Expected: the rows in numpy's lexsort order (see the module's docstring)."""
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    t0 = time.perf_counter()
    nl = 8192 * 1024 + 1
    i = np.arange(nl, dtype=np.int64)
    pos1 = (i * 7919) % 9973
    pos2 = (i * 104729) % nl                                       # 104729 does not divide nl = 3 * 2796203: a permutation, unique keys
    rows = np.empty((nl, 27), dtype=np.uint8)
    rows[:] = np.frombuffer(b"r\tc\t0000000\tc\t00000000\t+\t-\n", dtype=np.uint8)
    for d in range(7):
        rows[:, 10 - d] = 48 + (pos1 // 10 ** d) % 10
    for d in range(8):
        rows[:, 21 - d] = 48 + (pos2 // 10 ** d) % 10
    assert bytes(rows[1]) == b"r\tc\t%07d\tc\t%08d\t+\t-\n" % (7919, 104729)
    want = rows[np.lexsort((pos2, pos1))]
    sample = [sortdef.key(bytes(r[:-1]))[:4] for r in want[::2048]]
    assert sample == sorted(sample) and len(set(sample)) == len(sample)
    data = rows.tobytes()
    del rows
    t1 = time.perf_counter()
    got = np.frombuffer(gpu_sort(data), dtype=np.uint8)
    t2 = time.perf_counter()
    assert got.size == want.size
    got = got.reshape(nl, 27)
    if not np.array_equal(got, want):
        r = int(np.flatnonzero((got != want).any(axis=1))[0])
        pytest.fail(f"first difference at line {r} of {nl}: got key {sortdef.key(bytes(got[r, :-1]))[:4]}, want key {sortdef.key(bytes(want[r, :-1]))[:4]}")
    with capsys.disabled():
        print(f"\n[sort edges (d)] {nl} lines, {got.size} bytes: host text and expected order {t1 - t0:.2f} s, feed + GPU sort + fetch {t2 - t1:.2f} s, "
              f"compare {time.perf_counter() - t2:.2f} s")


# ---- key widths ----------------------------------------------------------------------------------------------------------
def dict_names(D):
    """D names with D distinct dictionary forms, spelled so that the dictionary order is neither the order of first appearance nor
    plain byte order: a '_' (above the digits and capitals, below the small letters) and a '.' (below all of them) sit at places
    that change from name to name, and whether a number is zero-padded ("chr00017" < "chr2") decides its place."""
    out = []
    for k in range(D):
        s = (b"chr%d" % k) if k % 3 == 0 else (b"chr%05d" % k) if k % 3 == 1 else (b"Chr%dv" % k)
        a = k % (len(s) + 1)
        s = s[:a] + b"_" + s[a:]
        a = (7 * k) % (len(s) + 1)
        out.append(s[:a] + b"." + s[a:])
    assert len({sortdef.dict_form(s) for s in out}) == D
    return out


@pytest.mark.parametrize("D", [1, 2, 16, 17, 256, 257, 4097])
def test_key_widths(tmp_path, D):
    """(e) the rank bits step at 16 / 17, 256 / 257 and 4096 / 4097 distinct dictionary forms (one 4-bit pass more per name field).
    D = 17 and 257 get five more spellings of names that are already there ('-' and ':' are dropped by -d as well): more table
    slots than ranks, and equal keys across different spellings."""
    rnd = random.Random(5000 + D)
    names = dict_names(D)
    if D in (17, 257):
        extra = [b"-" + names[(3 * j + 1) % D].replace(b"_", b":") for j in range(5)]
        assert not set(extra) & set(names) and {sortdef.dict_form(s) for s in extra} <= {sortdef.dict_form(s) for s in names}
        names += extra
    order = list(range(len(names)))
    rnd.shuffle(order)                                            # every name is there at least once, in an order of its own
    lines = []
    for i in range(20000):
        c1 = names[order[i]] if i < len(names) else rnd.choice(names)
        lines.append(b"k%d\t%s\t%d\t%s\t%d\t+\t-" % (rnd.randrange(0, 1000), c1, rnd.randrange(0, 40), rnd.choice(names), rnd.randrange(0, 40)))
    check(text(lines), tmp_path)


def test_names_of_62_bytes(tmp_path):
    """(e) the longest name the table keeps, 62 bytes: names that differ in byte 62 only, two of them ('_', '.') equal under -d to
    the 61-byte name"""
    rnd = random.Random(62)
    names = [b"A" * 61 + c for c in (b"a", b"b", b"0", b"_", b".")] + [b"A" * 61, b"A" * 60 + b"_a", b"A" * 60 + b"a"]
    assert max(map(len, names)) == 62
    lines = [b"n%d\t%s\t%d\t%s\t%d\t-\t+" % (rnd.randrange(0, 100), rnd.choice(names), rnd.randrange(0, 4), rnd.choice(names), rnd.randrange(0, 4)) for _ in range(3000)]
    check(text(lines), tmp_path)


# ---- position widths -------------------------------------------------------------------------------------------------------
POSITIONS = [0, 1, 15, 16, (1 << 16) - 1, 1 << 16, (1 << 28) - 1, 1 << 28, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]


def test_position_widths(tmp_path):
    """(f) every 4-bit digit of the two 32-bit positions carries weight somewhere; leading zeros (one, or a field of 25 digits) leave
    the key as it is, so the whole line decides among those lines"""
    rnd = random.Random(32)

    def field(v):
        r = rnd.random()
        return b"%d" % v if r < 0.5 else b"0%d" % v if r < 0.7 else b"%012d" % v if r < 0.9 else b"%025d" % v

    lines = [b"p%d\t%s\t%s\t%s\t%s\t+\t-" % (rnd.randrange(0, 50), rnd.choice((b"chr1", b"chr2")), field(rnd.choice(POSITIONS)), rnd.choice((b"chr1", b"chr_1", b"chr2")),
                                              field(rnd.choice(POSITIONS))) for _ in range(6000)]
    lines.append(b"z\tchr1\t0000000000000000000000007\tchr1\t0000000000000000000000007\t+\t-")
    lines.append(b"z\tchr1\t7\tchr1\t7\t+\t-")
    lines.append(b"y\tchr1\t6\tchr1\t0000000000000000000000008")
    check(text(lines), tmp_path)


# ---- line-index geometry -----------------------------------------------------------------------------------------------------
def fit_line(rnd, total, i):
    """one pairs line of exactly `total` bytes, newline included: the read name is padded"""
    if total < 40:
        rest = b"\tc\t%d\tc\t%d\n" % (rnd.randrange(0, 10), rnd.randrange(0, 10))
    else:
        rest = b"\tchr%d\t%d\tchr%d\t%d\t%s\t%s\n" % (rnd.randrange(1, 23), rnd.randrange(0, 1 << 20), rnd.randrange(1, 23), rnd.randrange(0, 1 << 20), rnd.choice((b"+", b"-")),
                                                        rnd.choice((b"+", b"-")))
    n = total - len(rest)
    assert n >= 1
    name = (b"g%d_" % i)[:n]
    return name + bytes(rnd.choices(ALNUM, k=n - len(name))) + rest


def layout(ends, seed, tail=25):
    """Text in which a newline sits at every byte offset of `ends` (ascending); ordinary lines of 20 to 100 bytes fill the room
    before each, `tail` more lines follow the last."""
    rnd = random.Random(seed)
    out = bytearray()
    i = 0
    for e in ends:
        while e + 1 - len(out) > 200:
            out += fit_line(rnd, rnd.randrange(20, 101), i)
            i += 1
        out += fit_line(rnd, e + 1 - len(out), i)
        i += 1
        assert out[e] == 10
    for _ in range(tail):
        out += fit_line(rnd, rnd.randrange(20, 101), i)
        i += 1
    return bytes(out)


@pytest.mark.parametrize("off", [15, 16, 16383, 16384, 65535, 65536])
def test_newline_at_an_edge(tmp_path, off):
    """(g) a newline as the last byte of a 16-byte vector / a wave's quarter / a workgroup's chunk, and as the first byte of the next"""
    check(layout([off], 7000 + off), tmp_path)


@pytest.mark.parametrize("total", [65536, 131072])
@pytest.mark.parametrize("final_newline", [True, False], ids=["final_newline", "no_final_newline"])
def test_text_that_ends_on_a_chunk_edge(tmp_path, total, final_newline):
    """(g) exactly one / two chunks of text with their final newline; and the same number of bytes without it, so that the newline
    the sorter appends is the only byte of a chunk of its own"""
    data = layout([total - 1], 7100 + total, tail=0) if final_newline else layout([total], 7200 + total, tail=0)[:-1]
    assert len(data) == total and data.endswith(b"\n") == final_newline
    check(data, tmp_path)


@pytest.mark.parametrize("start,length", [(16380, 40000), (5000, 70000)], ids=["40000_bytes", "70000_bytes"])
def test_long_lines(tmp_path, start, length):
    """(g) a line of 40,000 bytes from byte 16380 on (two whole wave quarters, [16384, 49152), hold no newline), and a line of
    70,000 bytes (longer than a chunk: a chunk edge inside it, a whole chunk's worth of bytes without a newline)"""
    data = layout([start - 1], 7300 + length, tail=0) + fit_line(random.Random(length), length, 99999) + layout([150], 7400 + length)
    assert data[start - 1] == 10 and data[start - 1 + length] == 10 and max(map(len, data.split(b"\n"))) == length - 1
    check(data, tmp_path)


# ---- what the sorter must refuse -------------------------------------------------------------------------------------------
GOOD = [b"a\tchr2\t10\tchr1\t5\t+\t-", b"b\tchr1\t10\tchr1\t5\t+\t-", b"c\tchr1\t9\tchr1\t7\t-\t-"]


def _with(bad):
    return text(GOOD[:2] + [bad] + GOOD[2:])


REJECTED = {
    "position_2^32": _with(b"x\tchr1\t4294967296\tchr1\t5\t+\t-"),
    "position_2^64+1": _with(b"x\tchr1\t18446744073709551617\tchr1\t5\t+\t-"),       # wraps to 1 in 64 bits
    "pos2_2^64+1": _with(b"x\tchr1\t5\tchr1\t18446744073709551617\t+\t-"),
    "position_of_25_digits": _with(b"x\tchr1\t5\tchr1\t1234567890123456789012345\t+\t-"),
    "12a": _with(b"x\tchr1\t12a\tchr1\t5\t+\t-"),
    "-5": _with(b"x\tchr1\t-5\tchr1\t5\t+\t-"),
    "three_tabs": _with(b"x\tchr1\t5\tchr1"),
    "empty_line": _with(b""),
    "name_of_63_bytes": _with(b"x\t" + b"N" * 63 + b"\t5\tchr1\t5\t+\t-"),
    "8193_names": text(b"x\tctg%d\t5\tctg0\t5\t+\t-" % k for k in range(8193)),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejections(tmp_path, case):
    """(h) each of these is an error, never a line sorted under a made-up key; a fresh sorter afterwards works"""
    with pytest.raises(m.MktError):
        gpu_sort(REJECTED[case])
    check(text(GOOD), tmp_path)


def test_accepted_at_the_limits(tmp_path):
    """(h) what lies just inside: 8192 distinct names in 8192 lines (the name table full to its last slot), eight of them 62 bytes
    long, positions of 2^32 - 1"""
    names = [b"ctg_" + b"0" * 57 + b"%d" % k if k < 8 else b"ctg.%d" % k if k % 5 == 0 else b"ctg%d" % k for k in range(8192)]
    assert len(names[0]) == 62 and len({sortdef.dict_form(s) for s in names}) == 8192
    lines = [b"x%d\t%s\t%d\t%s\t4294967295\t+\t-" % (k, names[k], (1 << 32) - 1 - k % 3, names[(k * 37) % 8192]) for k in range(8192)]
    check(text(lines), tmp_path)
