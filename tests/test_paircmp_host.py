"""The pair-level concordance without a GPU.  tests/golden/paircmp_golden.json holds what the reference's
benchmarking/check.consistency.pl printed for seeded pairs of .pairs texts; tests/paircmp_inputs.py makes those texts again.
 * tests/paircmpdef.py, the definition of include/mkt.h in plain Python, gives the report and the I/B part of the inconsistent text to
   the byte and the A part as a sorted multiset (the script walks a Perl hash there): this is where the rules are pinned.
 * tests/host/paircmp_host.cpp, a stand-alone program around the host half of the library (microcket_amd/csrc/mkt_paircmp.h: the
   report, the grouping by id string that resolves colliding keys), gives the report to the byte and the definition's classes, however
   the ids are dealt to runs, also when built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import paircmp_inputs as pi
import paircmpdef as pd
import util

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "paircmp_host")
HOST_SAN = HOST + "_san"

_cache = {}


def golden():
    """[(case, text A, text B, the definition's result)], made once and left unchanged"""
    if "g" not in _cache:
        out = []
        for c in pi.cases():
            a, b = pi.make(c["gen"])
            out.append((c, a, b, pd.compare(a, b, int(c["dist"] or 0))))
        _cache["g"] = out
    return _cache["g"]


def sorted_lines(b):
    return b"".join(sorted(b.splitlines(keepends=True)))


def test_cases_cover_what_they_are_there_for():
    g = {c["name"]: (c, a, b, r) for c, a, b, r in golden()}
    assert [p["name"] for p in pi.CASE_PARAMS] == list(g)
    for c, a, b, r in g.values():
        assert c["gen"] == next(p for p in pi.CASE_PARAMS if p["name"] == c["name"])["gen"]
        assert r.info["lines"] == [c["lines_a"], c["lines_b"]] and max(r.info["lines"]) <= 21000
    for name in ("dist_1", "dist_200", "dist_500"):
        r = g[name][3]
        assert r.info["consistent"] >= 20 and r.info["discordant"] >= 20
    assert g["dist_0_is_200"][0]["stdout"] == g["dist_200"][0]["stdout"] and "Using Distance: 200\n" in g["dist_200"][0]["stdout"]
    assert g["dist_200_at_500"][3].info["consistent"] > g["dist_200"][3].info["consistent"]
    out = g["distribution"][0]["stdout"]
    for shown in ("\t0\n", "\t3e-06\n", "\t1.2e-05\n", "\t0.001234\n"):
        assert shown in out, shown
    r = g["repeats"][3]
    assert pd.SUPERSEDED in r.classes_a and r.info["distinct_a"] < r.info["data_lines"][0] == sum(r.info["dist"][0].values())
    r = g["hot"][3]
    assert r.classes_a.count(pd.SUPERSEDED) == 49 and r.info["b_only"] == 50 and r.info["consistent"] == 1
    assert g["both_empty"][3].info["lines"] == [0, 0] and g["only_a"][3].info["lines"][1] == 0 and g["only_b"][3].info["lines"][0] == 0
    c, a, b, r = g["ids"]
    for cross in (1, 2):
        at = a.rfind(b"\n", 0, cross * pi.CHUNK) + 1
        assert a[at:at + 1] == b"X" and a.index(b"\t", at) > cross * pi.CHUNK           # an id across the chunk boundary
    assert {len(x.split(b"\t")[0]) for x in a.split(b"\n") if x} >= {1, 63, 64, 65, 129, 300}
    c, a, b, r = g["lines"]
    assert not a.endswith(b"\n") and not b.endswith(b"\n") and b"\t007\t" in r.lines and str((1 << 31) - 1).encode() in r.lines
    assert r.classes_a.count(pd.COMMENT) == 4 and r.classes_b.count(pd.COMMENT) == 4
    assert g["mixed"][3].info["lines"][0] > 16384 and all(g["mixed"][3].info[k] > 40 for k in ("consistent", "discordant", "a_only", "b_only"))


@pytest.mark.parametrize("k", range(len(pi.CASE_PARAMS)))
def test_definition_gives_the_reference_bytes(k):
    c, a, b, r = golden()[k]
    assert pd.report(r, "{A}", "{B}").decode() == c["stdout"]
    assert r.lines_ib.decode() == c["inconsistent_ib"]
    assert sorted_lines(r.lines_a).decode() == c["inconsistent_a_sorted"]


def test_definition_refuses_lines_outside_the_domain():
    for bad, n in ((b"r1\tchr1\t5\tchr1\n", 1), (b"#c\nr1\tchr1\t5\tchr1\t6\nr2\tchr1\tx5\tchr1\t6\n", 3), (b"r\tc\t1\tc\t2147483648\n", 1), (b"\n", 1)):
        with pytest.raises(pd.BadLine) as e:
            pd.compare(b"ok\tc\t1\tc\t2\n", bad)
        assert (e.value.side, e.value.number) == ("B", n)


def _host(exe, tmp_path, c, a, b, bits):
    fa, fb = tmp_path / "a.pairs", tmp_path / "b.pairs"
    fa.write_bytes(a)
    fb.write_bytes(b)
    r = subprocess.run([exe, str(fa), str(fb), c["dist"] or "0", str(bits), "{A}", "{B}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (c["name"], r.returncode, r.stderr.decode()[-2000:])
    la, ca, lb, cb, rep = r.stdout.split(b"\n", 4)
    assert la == b"classes A %d" % len(ca) and lb == b"classes B %d" % len(cb)
    return bytes(x - 48 for x in ca), bytes(x - 48 for x in cb), rep


@pytest.mark.parametrize("bits", [0, 3, 12])
@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_half_gives_the_reference_report_and_the_classes(san, bits, tmp_path):
    util.ensure_built()
    exe = HOST_SAN if san else HOST
    assert os.path.exists(exe), exe
    for c, a, b, r in golden():
        ca, cb, rep = _host(exe, tmp_path, c, a, b, bits)
        assert rep.decode() == c["stdout"], c["name"]
        assert ca == r.classes_a and cb == r.classes_b, c["name"]


@pytest.mark.parametrize("bits", [0, 3])
def test_host_half_on_the_cases_without_golden(bits, tmp_path):
    """one id 5 000 times on each side: too much inconsistent text for the golden file, so the definition alone is the yardstick"""
    util.ensure_built()
    for c in pi.EXTRA_PARAMS:
        a, b = pi.make(c["gen"])
        r = pd.compare(a, b, int(c["dist"] or 0))
        assert r.classes_a.count(pd.SUPERSEDED) == 4999 and r.info["b_only"] == 5000 and r.info["consistent"] == 1
        ca, cb, rep = _host(HOST_SAN, tmp_path, c, a, b, bits)
        assert rep == pd.report(r, "{A}", "{B}") and ca == r.classes_a and cb == r.classes_b


def test_host_driver_refuses_a_short_line(tmp_path):
    util.ensure_built()
    (tmp_path / "a").write_bytes(b"r\tc\t1\tc\t2\n")
    (tmp_path / "b").write_bytes(b"#x\nr\tc\t1\tc\n")
    r = subprocess.run([HOST, str(tmp_path / "a"), str(tmp_path / "b"), "200", "0", "a", "b"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"file B line 2" in r.stderr
