"""The pair statistics without a GPU.
 * tests/pairstatdef.py, the definition of include/mkt.h in plain Python, on the directed families of tests/pairstat_cases.py against
   what each family states by hand.
 * The 74 edge constants committed in microcket_amd/csrc/mkt_pairstat.h equal the numpy derivation.
 * tests/host/pairstat_host.cpp, a stand-alone program around the host and shared half of the library (the parse and the classes of a
   line as the kernels apply them, the areas, P(s), the convergence rule, both texts), gives the definition's counters, float bit
   patterns and bytes, also when built with the address and undefined-behaviour sanitizers.
 * The reference pin: for the 36 cases of tests/golden/golden.json that carry their sorted .pairs text, the definition's trans /
   cis10K / cis1K / cis0 equal what the reference logged."""
import json
import os
import re
import struct
import subprocess

import pytest

import pairstat_cases as pc
import pairstatdef as pd
import util

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "pairstat_host")
HOST_SAN = HOST + "_san"
_cache = {}


def family(name):
    """(family, the definition's result), made once and left unchanged"""
    if not _cache:
        for f in pc.families():
            _cache[f["name"]] = (f, pd.stats(f["table"], f["text"], f["tol_permille"], f["min_count"]))
    return _cache[name]


NAMES = [f["name"] for f in pc.families()]


def golden_cases():
    """[(input name, case)] of golden.json with pairs_sorted"""
    with open(os.path.join(util.GOLDEN, "golden.json")) as f:
        g = json.load(f)
    return [(i["name"], c) for i in g["inputs"] for c in i["cases"] if "pairs_sorted" in c]


def golden_table(text: bytes) -> bytes:
    """every name of the text that a table can hold (some of the reference's inputs have names of more than 63 bytes), with the largest
    length the table takes"""
    names = sorted({f for ln in text.split(b"\n") if ln and not ln.startswith(b"#") for f in (ln.split(b"\t")[1], ln.split(b"\t")[3]) if len(f) <= 63} | {b"chr1"})
    return b"".join(n + b"\t4294967295\n" for n in names)


def test_committed_edges_equal_the_numpy_derivation():
    hdr = open(os.path.join(util.ROOT, "microcket_amd", "csrc", "mkt_pairstat.h")).read()
    body = hdr[hdr.index("#define MKT_PS_EDGES"):hdr.index("constexpr uint32_t kPsEdges")]
    got = [int(x) for x in re.findall(r"\b(\d+)u\b", body)]
    assert got == pd.EDGES and len(got) == 74 == pd.BINS
    assert got[:10] == [0, 1, 1, 2, 2, 3, 4, 6, 7, 10] and got[-3:] == [562341325, 749894209, 1000000000] and got[17] == 100 and got[18] == 133
    exact = [10.0 ** (k / 8.0) for k in range(73)]
    assert min(abs((x % 1.0) - 0.5) for x in exact) > 0.001                           # no edge near a rounding tie


@pytest.mark.parametrize("name", NAMES)
def test_definition_gives_what_the_family_states(name):
    f, r = family(name)
    want = dict(f["want"])
    bins, empty = want.pop("bins", {}), want.pop("empty_bins", ())
    rows, chrom = want.pop("dist_rows", None), want.pop("chrom", None)
    assert {k: r.info[k] for k in want} == want
    for d, k in bins.items():
        assert pd.bin_of(d) == k, d
    for k in empty:
        assert r.dist[k] == [0, 0, 0, 0] and r.area[k] == 0 and r.P[k] == 0.0
    if rows is not None:
        assert {k: r.dist[k] for k in range(pd.BINS) if any(r.dist[k])} == rows
    if chrom is not None:
        n = len(r.names)
        assert {(a, b): r.chrom[a][b] for a in range(n) for b in range(n) if r.chrom[a][b]} == chrom
    i = r.info
    assert i["counted"] == i["cis"] + i["trans"] == sum(map(sum, r.chrom)) and i["total"] == i["cis0"] + i["cis1K"] + i["cis10K"] + i["ref_trans"]
    if i["skipped"] == 0:                                                             # then the reference's classes are the table's
        assert (i["cis0"], i["cis1K"], i["cis10K"], i["ref_trans"]) == (i["cis"] - i["cis_1kb+"], i["cis_1kb+"] - i["cis_10kb+"], i["cis_10kb+"], i["trans"])
    assert sum(map(sum, r.dist)) <= i["cis"] and i["cis"] - sum(map(sum, r.dist)) <= i["no_strand"]


def test_definition_edges_family_in_detail():
    f, r = family("edges")
    ds = pc.edge_distances()
    assert all(e - 1 in ds and e in ds and e + 1 in ds for e in pd.EDGES if e) and len(ds) * 4 + 2 == f["text"].count(b"\n")
    for k in range(pd.BINS):                                                          # every distance once per orientation
        inside = sum(1 for d in ds if pd.EDGES[k] <= d < (pd.EDGES[k + 1] if k + 1 < pd.BINS else 1 << 62))
        assert r.dist[k] == [inside] * 4, k
    assert sum(1 for ln in f["text"].split(b"\n") if ln[:1] == b"e" and int(ln.split(b"\t")[2]) > int(ln.split(b"\t")[4])) >= len(ds)
    # areas by hand: bin 0 = [0, 1) holds d = 0, L position pairs per chromosome; bin 2 = [1, 2) holds d = 1
    Ls = [L for _, L in pc.ROWS]
    assert r.area[0] == sum(Ls) and r.area[2] == sum(L - 1 for L in Ls) and r.area[1] == r.area[3] == 0
    assert r.area[73] == sum((pc.BIG - d) for d in (10 ** 9, pc.BIG - 1)) * (pc.BIG - 10 ** 9) // 2        # only chr1 is that long
    assert sum(r.area) == sum(L * (L + 1) // 2 for L in Ls)                           # every (d, start) of every chromosome exactly once
    assert r.P[0] == 4.0 / float(sum(Ls)) and r.stat_text.count(b"\n") == 17 + 9 + 1 + 74 * 4
    assert b"dist_freq/1000000000+/--\t3\n" in r.stat_text and b"dist_freq/1-1/++\t0\n" in r.stat_text and b"chrom_freq/chr1/chr1\t%d\n" % (4 * len(ds)) in r.stat_text


def test_definition_area_can_pass_64_bits():
    table = pc.name_table(0) + b"".join(b"big%d\t4294967295\n" % k for k in range(8))
    r = pd.stats(table, b"")
    assert sum(r.area) > 1 << 64 and r.area[73] > 1 << 64 and isinstance(r.area_f[73], float)
    assert r.info["total"] == 0 and r.info["convergence_dist"] == -1 and all(p == 0.0 for p in r.P)


def test_definition_refuses_malformed_lines_and_tables():
    for text, number in pc.MALFORMED:
        with pytest.raises(pd.BadLine) as e:
            pd.stats(pc.TABLE, text)
        assert e.value.number == number
    assert len(pd.parse_table(pc.name_table(2048))) == 2048
    with pytest.raises(pd.TooManyNames):
        pd.parse_table(pc.name_table(2049))


def test_reference_pin_on_the_golden_pairs():
    cases = golden_cases()
    assert len(cases) == 36
    for name, c in cases:
        text = c["pairs_sorted"].encode()
        r = pd.stats(golden_table(text), text)
        log = dict(ln.split("\t") for ln in c["log"].splitlines())
        assert {k: str(v) for k, v in pd.reference_log(r).items()} == {k: log[k] for k in ("trans", "cis10K", "cis1K", "cis0")}, (name, c["mode"])
        assert r.info["total"] == c["pairs_lines"]


def _host(exe, tmp_path, table, text, tol, mc):
    ft, fp = tmp_path / "t.sizes", tmp_path / "in.pairs"
    ft.write_bytes(table)
    fp.write_bytes(text)
    return subprocess.run([exe, str(ft), str(fp), str(tol), str(mc), str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _check_host(r, out, want, tmp_path, name):
    assert out.returncode == 0, (name, out.returncode, out.stderr.decode()[-2000:])
    got = {ln.split(b" ")[0].decode(): ln.split(b" ")[1:] for ln in out.stdout.splitlines()}
    i = want.info
    for k in ("total", "skipped", "counted", "cis", "trans", "no_strand", "header_lines", "cis0", "cis1K", "cis10K", "ref_trans", "convergence_dist"):
        assert int(got[k][0]) == i[k], (name, k)
    assert [int(got["cis_ge%d" % k][0]) for k in range(6)] == [i[k] for k in pd.GE_KEYS], name
    assert [int(x) for x in got["dist"]] == [c for row in want.dist for c in row], name
    assert [x.decode() for x in got["area"]] == [struct.pack(">d", a).hex() for a in want.area_f], name
    assert [x.decode() for x in got["P"]] == [struct.pack(">d", p).hex() for p in want.P], name
    assert (tmp_path / "out.pairs.stat").read_bytes() == want.stat_text, name
    assert (tmp_path / "out.scaling.tsv").read_bytes() == want.scaling_text, name


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_half_gives_the_definitions_counters_floats_and_bytes(san, tmp_path):
    util.ensure_built()
    exe = HOST_SAN if san else HOST
    assert os.path.exists(exe), exe
    for name in NAMES:
        f, want = family(name)
        _check_host(f, _host(exe, tmp_path, f["table"], f["text"], f["tol_permille"], f["min_count"]), want, tmp_path, name)
    # areas past 2^64, an empty text
    table = b"".join(b"big%d\t4294967295\n" % k for k in range(8))
    _check_host(None, _host(exe, tmp_path, table, b"", 50, 1000), pd.stats(table, b""), tmp_path, "big")
    # the reference pin through the host half
    for name, c in golden_cases()[::6]:
        text = c["pairs_sorted"].encode()
        _check_host(None, _host(exe, tmp_path, golden_table(text), text, 50, 1000), pd.stats(golden_table(text), text), tmp_path, name)


def test_host_half_refuses_what_the_definition_refuses(tmp_path):
    util.ensure_built()
    for text, number in pc.MALFORMED:
        out = _host(HOST_SAN, tmp_path, pc.TABLE, text, 50, 1000)
        assert out.returncode == 3 and out.stderr == b"line %d\n" % number, (text[-40:], out.stderr)
    assert _host(HOST_SAN, tmp_path, pc.name_table(2048), pc.GOOD.replace(b"chr2", b"c7"), 50, 1000).returncode == 0
    assert _host(HOST_SAN, tmp_path, pc.name_table(2049), b"", 50, 1000).returncode == 5
    assert _host(HOST_SAN, tmp_path, b"chr1\n", b"", 50, 1000).returncode == 4
