"""The pair-level concordance on the GPU at its word, run, key and line edges: the directed cases of tests/paircmp_edge_cases.py
(tests/test_paircmp_edges_host.py proves that they sit there) through microcket_amd.PairCompare at every width of each case and
through bin/pairscmp.  Counters, both class arrays, the report and the inconsistent text equal the definition's (tests/paircmpdef.py)
byte for byte -- host_runs alone may differ between widths -- and, for the cases inside the pinned domain, what the reference's script
printed (tests/golden/paircmp_edges_golden.json).

A handle has no call that drops its texts, so a handle that refused a text cannot be given another one; after every refusal the
handle refuses again in the same words, and the one handle that can be repaired -- its bad line is an unfinished last line -- is.

Not reachable: two different ids with one full 96-bit key cannot be made, so at hash_bits 0 the host resolution of a collision is
exercised only through the narrowed widths (host_runs > 0 there)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import pytest

import microcket_amd as m
import paircmp_edge_cases as ec
import paircmpdef as pd

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairscmp")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paircmp_edges_golden.json")
INFO_KEYS = ("lines", "data_lines", "distinct_a", "consistent", "discordant", "a_only", "b_only", "dist")
_cache = {}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def want(c):
    """the definition's result of an accepted case, made once and left unchanged"""
    if c["name"] not in _cache:
        _cache[c["name"]] = pd.compare(c["a"], c["b"], int(c["dist"] or 0))
    return _cache[c["name"]]


def golden():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = {g["name"]: g for g in json.load(f)["cases"]}
    return _cache["golden"]


def distinct_ids(c):
    if ("ids", c["name"]) not in _cache:
        _cache["ids", c["name"]] = len({r[0] for t in (c["a"], c["b"]) for r in pd.parse(t, "A") if r is not None})
    return _cache["ids", c["name"]]


def feed(pc, a, b, piece=None):
    for add, t in ((pc.add_a, a), (pc.add_b, b)):
        if piece is None:
            add(t)
        else:
            for k in range(0, len(t), piece):
                add(t[k:k + piece])


def check(pc, res, info, name=""):
    """everything but host_runs equals the definition's"""
    assert {k: info[k] for k in INFO_KEYS} == {k: res.info[k] for k in INFO_KEYS}, name
    assert pc.classes("a").tobytes() == res.classes_a and pc.classes("b").tobytes() == res.classes_b, name
    assert pc.report("{A}", "{B}") == pd.report(res, "{A}", "{B}"), name
    assert info["lines_bytes"] == len(res.lines) and pc.lines() == res.lines, name


def check_golden(c, report, lines):
    g = golden()[c["name"]]
    assert report.decode() == g["stdout"]
    rows = lines.splitlines(keepends=True)
    assert len(rows) == g["lines_ib"] + g["lines_a"]
    assert sha(b"".join(rows[:g["lines_ib"]])) == g["sha256_ib"] and sha(b"".join(sorted(rows[g["lines_ib"]:]))) == g["sha256_a_sorted"]


@pytest.mark.parametrize("name,hash_bits", [(c["name"], w) for c in ec.accepted() for w in c["hash_bits"]])
def test_every_accepted_case_at_each_of_its_widths(name, hash_bits):
    c = ec.by_name(name)
    res = want(c)
    with m.PairCompare(device=0) as pc:
        feed(pc, c["a"], c["b"])
        info = pc.run(max_dist=int(c["dist"] or 0), hash_bits=hash_bits)
        check(pc, res, info, name)
        if c["golden"]:
            check_golden(c, pc.report("{A}", "{B}"), pc.lines())
        if hash_bits and distinct_ids(c) > (1 << hash_bits):                           # more ids than keys: some run holds two of them
            assert info["host_runs"] > 0, (name, hash_bits)
        if c["family"] == "run_at_block_edge":                                         # one id never collides: the device join decides
            assert info["host_runs"] == 0, (name, hash_bits)


@pytest.mark.parametrize("name", [c["name"] for c in ec.refused()])
def test_refused_cases_name_the_file_and_the_line(name):
    c = ec.by_name(name)
    side, number = c["refused"]
    with m.PairCompare(device=0) as pc:
        feed(pc, c["a"], c["b"])
        said = []
        for bits in (0, 2, 0):
            with pytest.raises(m.MktError, match=rf"bad argument: file {side} line {number}:") as e:
                pc.run(hash_bits=bits)
            said.append(str(e.value))
            with pytest.raises(m.MktError):
                pc.classes("a")                                                        # nothing of an earlier run is handed out
        assert said[0] == said[1] == said[2]
    ok = ec.by_name("ids_words")                                                       # and the device is as it was
    with m.PairCompare(device=0) as pc:
        feed(pc, ok["a"], ok["b"])
        check(pc, want(ok), pc.run(hash_bits=2), name)


def test_a_refused_handle_runs_an_accepted_text_once_its_last_line_is_complete():
    ok = ec.by_name("ids_words")
    cut = ok["b"].rindex(b"\t", 0, ok["b"].rindex(b"\t"))                              # B ends inside its last line, behind the fourth field
    with m.PairCompare(device=0) as pc:
        feed(pc, ok["a"], ok["b"][:cut])
        n = ok["b"].count(b"\n")
        for bits in (0, 2):
            with pytest.raises(m.MktError, match=rf"bad argument: file B line {n}:"):
                pc.run(hash_bits=bits)
        pc.add_b(ok["b"][cut:])
        for bits in (0, 2, 1):
            check(pc, want(ok), pc.run(hash_bits=bits), bits)


def test_names_fed_in_pieces_of_one_byte():
    c = ec.by_name("names")
    with m.PairCompare(device=0) as pc:
        feed(pc, c["a"], c["b"], 1)
        check(pc, want(c), pc.run(), "one byte")
        check_golden(c, pc.report("{A}", "{B}"), pc.lines())


@pytest.mark.parametrize("name", ["edge_a_long_256", "edge_comments_512", "edge_b_long_257"])
def test_block_edge_from_device_memory_in_two_pieces_cut_inside_a_line(name):
    from microcket_amd import capi
    c = ec.by_name(name)
    hip = C.CDLL(capi.hip_runtimes()[0])
    ptrs = []
    try:
        with m.PairCompare(device=0) as pc:
            for side in ("a", "b"):
                t = c[side]
                d = C.c_void_p()
                assert hip.hipMalloc(C.byref(d), C.c_size_t(len(t))) == 0
                ptrs.append(d)
                assert hip.hipMemcpy(d, t, C.c_size_t(len(t)), 1) == 0                 # hipMemcpyHostToDevice
                half = t.index(b"\n", len(t) // 2) - 2                                # the cut lies inside a line
                assert half > 0 and b"\n" not in t[half - 1:half + 2]
                pc.add_device(side, d.value, half)
                pc.add_device(side, d.value + half, len(t) - half)
            info = pc.run(hash_bits=5)
            check(pc, want(c), info, name)
            assert info["host_runs"] == 0
    finally:
        for d in ptrs:
            hip.hipFree(d)


def _cli(args):
    return subprocess.run([EXE, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_cli_on_the_emit_lengths_and_on_a_refused_case(tmp_path):
    c = ec.by_name("emit_lengths")
    res, g = want(c), golden()["emit_lengths"]
    fa, fb, fo = tmp_path / "a.pairs", tmp_path / "b.pairs", tmp_path / "inconsistent.txt"
    fa.write_bytes(c["a"])
    fb.write_bytes(c["b"])
    said = g["stdout"].replace("{A}", str(fa)).replace("{B}", str(fb))
    r = _cli([str(fa), str(fb)])
    assert r.returncode == 0 and r.stdout.decode() == said, r.stderr.decode()
    r = _cli([str(fa), str(fb), "", str(fo)])
    assert r.returncode == 0 and r.stdout.decode() == said, r.stderr.decode()
    assert fo.read_bytes() == res.lines
    check_golden(c, r.stdout.replace(os.fsencode(str(fa)), b"{A}").replace(os.fsencode(str(fb)), b"{B}"), fo.read_bytes())
    c = ec.by_name("refused_a600_b3")
    fa.write_bytes(c["a"])
    fb.write_bytes(c["b"])
    out = tmp_path / "refused.txt"
    r = _cli([str(fa), str(fb), "200", str(out)])
    assert r.returncode not in (0, 2) and r.stdout == b"" and re.search(rb"file A line 600:", r.stderr), r.stderr
    assert not out.exists() or out.read_bytes() == b""
