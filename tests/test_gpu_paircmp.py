"""Pair-level concordance of two .pairs texts on the GPU (mkt_paircmp_* of include/mkt.h, microcket_amd.PairCompare, bin/pairscmp):
counters, class bytes, report bytes and inconsistent bytes equal the definition (tests/paircmpdef.py) and, where the golden file has
the case, what the reference's benchmarking/check.consistency.pl printed (its A lines as a sorted multiset: the script walks a Perl
hash there), for every key width, by every route and on every call."""
import ctypes as C
import os
import subprocess

import pytest

import microcket_amd as m
import paircmp_inputs as pi
import paircmpdef as pd

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairscmp")
INFO_KEYS = ("lines", "data_lines", "distinct_a", "consistent", "discordant", "a_only", "b_only", "dist", "lines_bytes")
_cache = {}


def golden():
    """{name: (case, text A, text B, {max_dist: the definition's result})}, made once and left unchanged"""
    if "g" not in _cache:
        _cache["g"] = {}
        for c in pi.cases() + pi.EXTRA_PARAMS:                                      # (the extra cases have no reference bytes)
            a, b = pi.make(c["gen"])
            _cache["g"][c["name"]] = (c, a, b, {})
    return _cache["g"]


def expected(name, max_dist):
    c, a, b, res = golden()[name]
    if max_dist not in res:
        res[max_dist] = pd.compare(a, b, max_dist)
    return res[max_dist]


def sorted_lines(b):
    return b"".join(sorted(b.splitlines(keepends=True)))


def distinct_ids(a, b):
    return len({r[0] for t, s in ((a, "A"), (b, "B")) for r in pd.parse(t, s) if r is not None})


def feed(pc, a, b, piece=None):
    for add, text in ((pc.add_a, a), (pc.add_b, b)):
        if piece is None:
            add(text)
        else:
            for k in range(0, len(text), piece):
                add(text[k:k + piece])


def check(pc, want, info, name="", lines=True):
    assert {k: info[k] for k in INFO_KEYS if k != "lines_bytes"} == {k: want.info[k] for k in INFO_KEYS if k != "lines_bytes"}, name
    assert pc.classes("a").tobytes() == want.classes_a and pc.classes("b").tobytes() == want.classes_b, name
    assert pc.report("{A}", "{B}") == pd.report(want, "{A}", "{B}"), name
    if lines:
        assert info["lines_bytes"] == len(want.lines) and pc.lines() == want.lines, name
    else:
        assert info["lines_bytes"] == 0 and pc.lines() == b"", name


@pytest.mark.parametrize("hash_bits", [0, 1, 4, 12])
@pytest.mark.parametrize("name", [p["name"] for p in pi.CASE_PARAMS + pi.EXTRA_PARAMS])
def test_every_family_at_every_key_width(name, hash_bits):
    """the distance, distribution, repeat, id, line and mixed families of the golden file; the narrow keys put different ids into one run,
    which the host resolves, and nothing but host_runs may change"""
    c, a, b, _ = golden()[name]
    D = int(c["dist"] or 0)
    want = expected(name, D)
    with m.PairCompare(device=0) as pc:
        feed(pc, a, b)
        info = pc.run(max_dist=D, hash_bits=hash_bits)
        check(pc, want, info, name)
        if "stdout" in c:                                                            # a golden case: the reference's bytes
            assert pc.report("{A}", "{B}").decode() == c["stdout"]
            got = pc.lines()
            assert got[:len(c["inconsistent_ib"])].decode() == c["inconsistent_ib"]
            assert sorted_lines(got[len(c["inconsistent_ib"]):]).decode() == c["inconsistent_a_sorted"]
        if hash_bits and distinct_ids(a, b) > (1 << hash_bits):                      # more ids than keys: some run holds two of them
            assert info["host_runs"] > 0, (name, hash_bits)
        if hash_bits == 0:
            t = pc.timing_ms()
            assert set(t) == {"parse", "sort", "join", "emit"} and all(v >= 0 for v in t.values())


@pytest.mark.parametrize("name,piece", [("dist_200", 1), ("lines", 1), ("repeats", 7), ("lines", 7), ("ids", 4096), ("mixed", 4096)])
def test_any_chunking_of_add_gives_the_same_bytes(name, piece):
    c, a, b, _ = golden()[name]
    D = int(c["dist"] or 0)
    with m.PairCompare(device=0) as pc:
        feed(pc, a, b, piece)
        check(pc, expected(name, D), pc.run(max_dist=D), name)


@pytest.mark.parametrize("name", ["lines", "ids", "hot_5000"])
def test_device_bytes_give_the_same_bytes(name):
    from microcket_amd import capi
    c, a, b, _ = golden()[name]
    hip = C.CDLL(capi.hip_runtimes()[0])
    ptrs = []
    try:
        with m.PairCompare(device=0) as pc:
            for side, text in (("a", a), ("b", b)):
                d = C.c_void_p()
                assert hip.hipMalloc(C.byref(d), C.c_size_t(len(text))) == 0
                ptrs.append(d)
                assert hip.hipMemcpy(d, text, C.c_size_t(len(text)), 1) == 0        # hipMemcpyHostToDevice
                half = len(text) // 2                                                # in two pieces, the cut inside a line
                pc.add_device(side, d.value, half)
                pc.add_device(side, d.value + half, len(text) - half)
            check(pc, expected(name, 200), pc.run(), name)
    finally:
        for d in ptrs:
            hip.hipFree(d)


def test_run_again_and_with_other_options_on_the_same_texts():
    c, a, b, _ = golden()["dist_200"]
    with m.PairCompare(device=0) as pc:
        feed(pc, a, b)
        first = pc.run()
        check(pc, expected("dist_200", 200), first)
        kept = (pc.classes("a").tobytes(), pc.classes("b").tobytes(), pc.lines())
        again = pc.run()
        first.pop("host_runs"), again.pop("host_runs")
        assert again == first and (pc.classes("a").tobytes(), pc.classes("b").tobytes(), pc.lines()) == kept
        for D in (500, 1, 0, 201):
            check(pc, expected("dist_200", D), pc.run(max_dist=D), D)
        check(pc, expected("dist_200", 500), pc.run(max_dist=500, want_lines=False, hash_bits=4), "no lines", lines=False)
        check(pc, expected("dist_200", 200), pc.run(max_dist=0), "dist 0 is 200")
        assert pc.report("x.pairs", "y.pairs").startswith(b"Using Distance: 200\nLoading file A: x.pairs ...\nLoading file B: y.pairs ...\n\n")
        pc.add_b(b"late\tchr1\t1\tchr1\t2\n")                                     # more text after a run: the next run sees it
        more = pd.compare(a, b + b"late\tchr1\t1\tchr1\t2\n", 200)
        check(pc, more, pc.run())


def test_swap_on_one_chromosome_and_the_strict_bound():
    """the issue's example: A = (chr3, 10, chr3, 20) and B = (chr3, 210, chr3, 20) at D = 200 are consistent through the swap only"""
    a = b"r\tchr3\t10\tchr3\t20\ns\tchr3\t10\tchr3\t20\n"
    b = b"r\tchr3\t210\tchr3\t20\ns\tchr3\t220\tchr3\t20\n"
    want = pd.compare(a, b, 200)
    assert want.classes_b == bytes([pd.CONSISTENT, pd.DISCORDANT])
    with m.PairCompare(device=0) as pc:
        feed(pc, a, b)
        check(pc, want, pc.run(max_dist=200))


@pytest.mark.parametrize("side,bad,number", [
    ("b", b"#c\nok\tchr1\t1\tchr1\t2\nfour\tchr1\t5\tchr1\n", 3),
    ("a", b"x\tchr1\t1\tchr1\t2\n#c\n#d\ny\tchr1\t12a\tchr1\t6\nz\tchr1\t1\n", 4),
    ("b", b"y\tchr1\t1\tchr1\t2147483648\n", 1),
    ("a", b"y\tchr1\t\tchr1\t5\n", 1),
    ("b", b"ok\tchr1\t1\tchr1\t2\n\n", 2),
])
def test_lines_outside_the_domain_are_refused_by_file_and_line(side, bad, number):
    good = b"ok\tchr1\t1\tchr1\t2\n"
    a, b = (bad, good) if side == "a" else (good, bad)
    with pytest.raises(pd.BadLine) as e:
        pd.compare(a, b)
    assert (e.value.side, e.value.number) == (side.upper(), number)
    with m.PairCompare(device=0) as pc:
        feed(pc, a, b)
        for bits in (0, 2):
            with pytest.raises(m.MktError, match=rf"bad argument: file {side.upper()} line {number}:"):
                pc.run(hash_bits=bits)
    with m.PairCompare(device=0) as pc:
        feed(pc, good, good)
        with pytest.raises(m.MktError, match="hash_bits"):
            pc.run(hash_bits=33)


def _cli(args, stdin=None):
    return subprocess.run([EXE, *args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("name", ["dist_500", "dist_0_is_200", "distribution", "repeats", "lines", "both_empty", "mixed"])
def test_cli_prints_the_reference_bytes(name, tmp_path):
    c, a, b, _ = golden()[name]
    fa, fb, fo = tmp_path / "a.pairs", tmp_path / "b.pairs", tmp_path / "inconsistent.txt"
    fa.write_bytes(a)
    fb.write_bytes(b)
    args = [str(fa), str(fb)] + ([c["dist"]] if c["dist"] is not None else [])
    r = _cli(args)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == c["stdout"].replace("{A}", str(fa)).replace("{B}", str(fb))
    r = _cli([str(fa), str(fb), c["dist"] or "", str(fo)])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == c["stdout"].replace("{A}", str(fa)).replace("{B}", str(fb))
    got = fo.read_bytes()
    assert got[:len(c["inconsistent_ib"])].decode() == c["inconsistent_ib"]
    assert sorted_lines(got[len(c["inconsistent_ib"]):]).decode() == c["inconsistent_a_sorted"]


def test_cli_usage_stdin_gz_and_bad_input(tmp_path):
    c, a, b, _ = golden()["repeats"]
    fa, fb = tmp_path / "a.pairs", tmp_path / "b.pairs"
    fa.write_bytes(a)
    fb.write_bytes(b)
    for args in ([], [str(fa)]):
        r = _cli(args)
        assert r.returncode == 2 and b"Usage" in r.stderr and r.stdout == b""
    r = _cli([str(fa), "-"], stdin=b)
    assert r.returncode == 0 and r.stdout.decode() == c["stdout"].replace("{A}", str(fa)).replace("{B}", "-")
    for args in ([str(fa) + ".gz", str(fb)], [str(fa), str(fb) + ".gz"], [str(fa), str(fb), "200", str(tmp_path / "out.gz")]):
        r = _cli(args)
        assert r.returncode not in (0, 2) and b"no GPU inflate" in r.stderr and r.stdout == b""
    assert not (tmp_path / "out.gz").exists()
    fb.write_bytes(b + b"short\tchr1\t5\n")
    r = _cli([str(fa), str(fb)])
    assert r.returncode not in (0, 2) and b"file B line 13" in r.stderr and r.stdout == b""
    r = _cli([str(tmp_path / "missing.pairs"), str(fa)])
    assert r.returncode == 10
