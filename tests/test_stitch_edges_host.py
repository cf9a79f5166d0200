"""The stitcher's edge families without a GPU (tests/stitch_edge_cases.py): each family reaches the classes it was written for, worked
out from the definition's plain-loop scoring (stitchdef.candidates / choose); that scoring agrees with the vectorised one the
definition uses; the definition reproduces the program's hashes for every family and argument set
(tests/golden/stitch_edges_golden.json: FLASH v1.2.11 with one combiner thread + deal.flash.pl) and, where the program is present,
a live run of it; and the threshold table of mkt_stitch.h (through tests/host/stitch_thresholds.cpp) is the float32 comparison."""
import json
import os
import subprocess

import numpy as np
import pytest

import stitch_edge_cases as ec
import stitchdef as sd
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FLASH = "/root/reference/bin/flash"
GOLDEN = os.path.join(ROOT, "tests", "golden", "stitch_edges_golden.json")
_cache = {}


def golden():
    if "g" not in _cache:
        with open(GOLDEN) as f:
            _cache["g"] = json.load(f)
    return _cache["g"]


def golden_case(family, name):
    return next(c for c in golden()["families"][family] if c["name"] == name)


def check_hashes(r, g):
    """a result (stitchdef.stitch's, or the GPU's in the same form) against a golden entry: every stream and the stat line"""
    comb, unc = sd.by_kind(r["tab"])
    assert (sd.sha(comb), sd.sha(unc)) == (g["tab_combined_sha256"], g["tab_uncombined_sha256"]), g["name"]
    assert (sd.sha(r["ext"]), sd.sha(r["cut1"]), sd.sha(r["cut2"])) == (g["ext_sha256"], g["cut1_sha256"], g["cut2_sha256"]), g["name"]
    assert r["stat"].decode() == g["stat"] and r["total"] == g["pairs"], g["name"]


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_family_reaches_its_classes(family):
    facts = ec.COVER[family]()
    print(family, facts)
    n = [text.count(b"\n") // 8 for _c, text, _kw in ec.cases(family)]
    assert max(n) <= 400 and len({c for c, _t, _kw in ec.cases(family)}) == len(n)


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_candidates_agree_with_best_offsets(family):
    """the plain loops against the vectorised scan, every pair of every case; and against the lines the definition wrote"""
    for case, text, kw in ec.cases(family):
        m, M, x, phred = kw.get("m", 10), kw.get("M", 150), kw.get("x", 0.25), kw.get("phred", 33)
        rows = ec.scored(family)[case]
        off = sd._best_offsets([p for p, _c, _o in rows], m, M, x, phred)
        assert [int(o) for o in off] == [o for _p, _c, o in rows], case
        r = ec.definition(family)[case]
        assert r["combined"] == sum(o >= 0 for _p, _c, o in rows) and r["total"] == len(rows)
        for (p, cand, _o) in rows:
            n1, n2 = len(p[1]), len(p[3])
            assert [c[0] for c in cand] == list(range(max(0, n1 - n2), n1 - m + 1))
            assert all(0 <= mm <= eff <= n1 - i and mq <= 93 * mm for i, eff, mm, mq in cand)


def test_golden_names_every_case_once():
    assert os.path.getsize(GOLDEN) < 100_000
    assert set(golden()["families"]) == set(ec.FAMILIES)
    for family in ec.FAMILIES:
        assert [c["name"] for c in golden()["families"][family]] == [c for c, _t, _kw in ec.cases(family)]


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_definition_reproduces_every_hash(family):
    for case, text, kw in ec.cases(family):
        g = golden_case(family, case)
        assert sd.sha(text) == g["input_sha256"] and g["flash_args"] == ec.flash_args(kw), case      # the generator
        check_hashes(ec.definition(family)[case], g)


@pytest.mark.skipif(not os.path.exists(REF_FLASH), reason="the reference's bin/flash is not on this machine")
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_definition_equals_the_program(family):
    """every line of the program's output for every case, kind by kind in order (stitchdef.by_kind) and as a multiset"""
    for case, text, kw in ec.cases(family):
        p = subprocess.run([REF_FLASH, "-q", "--interleaved-input", *ec.flash_args(kw), "-t", "1", "-To", "-c", "-"], input=text, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert p.returncode == 0, (case, p.stderr)
        r = ec.definition(family)[case]
        assert sd.by_kind(p.stdout) == sd.by_kind(r["tab"]), case
        assert sorted(p.stdout.split(b"\n")) == sorted(r["tab"].split(b"\n")), case
        assert p.stdout.count(b"\n") == r["total"] == text.count(b"\n") // 8


def float32_thresholds(M, x):
    """thr[1 .. MAX_M] from float32 arithmetic: the largest mm, searched up to MAX_READ as the header does, for which
    float32(mm) / float32(sl) > float32(x) is false; 0 above M.  x arrives as a double and is cast, as in mkt_stitch_begin."""
    sl = np.arange(1, sd.MAX_M + 1, dtype=np.float32)[None, :]
    mm = np.arange(0, sd.MAX_READ + 1, dtype=np.float32)[:, None]
    ok = ~(mm / sl > np.float32(x))
    assert ok[0].all() and (ok[:-1] | ~ok[1:]).all()          # true at 0, and never true again once false
    thr = ok.sum(axis=0) - 1
    thr[M:] = 0
    return [int(t) for t in thr]


def threshold_densities():
    """x as doubles: 0, 1, the usual values, and for seeded (k, sl) the float32 quotient k / sl with its two float32 neighbours"""
    xs = [0.0, 1.0, 0.1, 0.2, 0.25, 0.3, 0.5, 1 / 3]
    R = np.random.RandomState(4601)
    for _ in range(60):
        sl = int(R.randint(1, sd.MAX_M + 1))
        k = int(R.randint(0, sl + 1))
        q = np.float32(k) / np.float32(sl)
        xs += [float(v) for v in (np.nextafter(q, np.float32(-1)), q, np.nextafter(q, np.float32(2))) if 0 <= float(v) <= 1]
    return xs


def test_threshold_table_is_the_float32_comparison():
    util.ensure_built()
    xs = threshold_densities()
    assert len(xs) > 150
    jobs = [(M, x) for M in (1, 2, 149, 150, 151, 254, 255) for x in xs]
    r = subprocess.run([util.STITCH_THRESHOLDS_EXE], input="".join("%d %r\n" % j for j in jobs).encode(), stdout=subprocess.PIPE, check=True)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(jobs)
    for (M, x), ln in zip(jobs, lines):
        assert [int(t) for t in ln.split()] == float32_thresholds(M, x), (M, x)
    # the same through the command line, and what the families rely on: stitchdef.threshold is that table
    r = subprocess.run([util.STITCH_THRESHOLDS_EXE, "150", "0.25", "255", "0.3333333"], stdout=subprocess.PIPE, check=True)
    a, b = ([int(t) for t in ln.split()] for ln in r.stdout.decode().splitlines())
    assert a == float32_thresholds(150, 0.25) and b == float32_thresholds(255, 0.3333333)
    assert (a[127], a[126], a[149], a[150]) == (32, 31, 37, 0)
    assert all(a[sl - 1] == sd.threshold(sl, 0.25) for sl in range(1, 151)) and all(b[sl - 1] == sd.threshold(sl, 0.3333333) for sl in range(1, 256))
    assert subprocess.run([util.STITCH_THRESHOLDS_EXE, "256", "0.25"], stdout=subprocess.PIPE, stderr=subprocess.PIPE).returncode == 2
