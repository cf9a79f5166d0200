"""tests/sortdef.py (the sorter's order restated in Python) against the system's GNU sort, run as the driver runs it
(util.gnu_sort: LANG=C sort -k2,2d -k4,4d -k3,3n -k5,5n).  CPU only.  The GPU tests lean on sortdef for their one large case and
for their failure messages, so it has to be the same order, byte for byte."""
import random

import sortdef
import util

P31, P32 = 1 << 31, 1 << 32
POSITIONS = [0, 15, 16, 65535, 65536, P31 - 1, P31, P32 - 1]


def _names():
    eq = [b"chr2", b"chr_2", b"chr2_", b"chr.2", b"HLA-A*01:01", b"HLAA0101"]          # -d: chr2 four times, HLAA0101 twice
    case = [b"Chr2"]                                                                   # case counts: another key than chr2
    long_ = [b"L" * 60 + b"a", b"L" * 60 + b"b", b"L" * 61 + b"a", b"L" * 61 + b"b", b"L" * 30 + b"_" + b"L" * 30 + b"a"]   # 61 / 62 bytes
    contigs = [b"chrUn_KI%06dv%d" % (270000 + 37 * k, 1 + k % 2) if k % 3 else b"ctg.%d_random" % k for k in range(300)]
    return eq + case + long_ + contigs


def _mixed_input(n=40000, seed=20240611):
    rnd = random.Random(seed)
    names = _names()
    out = []
    for i in range(n):
        a, b = rnd.choice(names), rnd.choice(names)
        if rnd.random() < 0.3:
            a = rnd.choice(names[:7])                    # many lines on the -d-equal spellings: the whole line decides among them
            b = rnd.choice(names[:7])
        p1, p2 = rnd.choice(POSITIONS), rnd.choice(POSITIONS)
        if rnd.random() < 0.5:
            p1 = rnd.randrange(0, 200)
        f1 = (b"%d" % p1) if rnd.random() < 0.7 else (b"000%d" % p1 if rnd.random() < 0.5 else b"%012d" % p1)
        f2 = (b"%d" % p2) if rnd.random() < 0.7 else b"0%d" % p2
        rid = b"r%d" % rnd.randrange(0, 3000)            # repeated read names: fully identical lines happen
        if rnd.random() < 0.1:
            out.append(b"\t".join((rid, a, f1, b, f2)))  # five fields: no strands
        else:
            out.append(b"\t".join((rid, a, f1, b, f2, rnd.choice((b"+", b"-")), rnd.choice((b"+", b"-")))))
    out += [b"z\tchr2\t0\tchr2\t0", b"z\tchr_2\t000\tchr.2\t0", b"z\tchr2\t0\tchr2\t000\t+\t-"]
    return b"".join(l + b"\n" for l in out)


def test_key_fields():
    assert sortdef.dict_form(b"HLA-A*01:01") == b"HLAA0101"
    assert sortdef.dict_form(b"chr_2") == sortdef.dict_form(b"chr.2") == sortdef.dict_form(b"chr2_") == b"chr2"
    assert sortdef.dict_form(b"Chr2") != sortdef.dict_form(b"chr2")
    assert sortdef.dict_form(b"a b\xc3\xa9c") == b"a bc"
    assert sortdef.key(b"r\tchr_2\t007\tchrX\t\t+\t-") == (b"chr2", b"chrX", 7, 0, b"r\tchr_2\t007\tchrX\t\t+\t-")
    assert sortdef.sort_pairs(b"") == b""
    assert sortdef.sort_pairs(b"b\tc\t2\tc\t1\na\tc\t10\tc\t1") == b"b\tc\t2\tc\t1\na\tc\t10\tc\t1\n"


def test_sortdef_equals_gnu_sort(tmp_path):
    data = _mixed_input()
    assert data.count(b"\n") >= 40000
    got = sortdef.sort_pairs(data)
    want = util.gnu_sort(data, tmp_path)
    assert got == want, sortdef.explain(got, want)


def test_explain_names_the_first_differing_line():
    a = b"r\tc\t1\tc\t1\nr\tc\t2\tc\t1\n"
    b = b"r\tc\t1\tc\t1\nr\tc\t3\tc\t1\n"
    msg = sortdef.explain(a, b)
    assert "line 1" in msg and "2" in msg and "3" in msg
