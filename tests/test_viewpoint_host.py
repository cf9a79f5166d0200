"""The viewpoint contact profiles without a GPU.  tests/golden/viewpoint_golden.json holds what the reference's two Perl scripts
(util/analyze.EBV) wrote for seeded .pairs text; tests/viewpoint_inputs.py makes that text again.
 * tests/viewpointdef.py, the definition of include/mkt.h in plain Python, gives the three texts to the byte.
 * tests/host/viewpoint_host.cpp, a stand-alone program around the host half of the library (microcket_amd/csrc/mkt_viewpoint.h: the
   hotspot cut, the string order of the kept links, the three emitters), fed the link tables of the definition, gives them to the byte
   as well, also when built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import util
import viewpoint_inputs as vi
import viewpointdef as vd

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "viewpoint_host")
HOST_SAN = HOST + "_san"

_cache = {}


def golden():
    """[(case, text, names, the profile at the links' bins, the profile at the track's bins)], made once"""
    if "g" not in _cache:
        tt = vi.table_text()
        names, lens = vd.parse_table(tt)
        v = names.index(vi.VIEWPOINT)
        ps = vd.partner_set(names, v, vi.PARTNER_RE)
        out = []
        for c in vi.cases():
            text = vi.make(c["gen"])
            recs = vd.records(text, names, lens)
            a = vd.profile(recs, names, v, ps, vbin=c["vbin"], pbin=c["pbin"], second_side_only=1, hotspot_ratio=c["ratio"])
            b = vd.profile(recs, names, v, ps, vbin=c["vbin"], pbin=c["track_bin"], second_side_only=1, min_count=1, hotspot_ratio=c["ratio"])
            out.append((c, text, names, a, b))
        _cache["g"] = out
    return _cache["g"]


def test_cases_cover_what_they_are_there_for():
    g = {c["name"]: (c, text, a, b) for c, text, _, a, b in golden()}
    assert [p["name"] for p in vi.CASE_PARAMS] == list(g)
    for c, text, a, b in g.values():
        assert c["gen"] == next(p for p in vi.CASE_PARAMS if p["name"] == c["name"])["gen"] and text.count(b"\n") == c["lines"] <= 30000
        assert a.total >= 1 and c["bedgraph"] and c["links"]
    assert {c["ratio"] for c, _, _, _ in g.values()} >= {0.01, 0.5, 0.99}
    counts = {l[3] for name in ("pow2", "pow2_low") for l in g[name][2].links}
    assert counts >= {(1 << k) + d for k in range(13) for d in (-1, 0, 1)} - {0}
    shown = {int(ln.split("=")[1][:-1]) for name in ("pow2", "pow2_low") for ln in g[name][0]["links"].splitlines()}
    assert shown >= set(range(2, 13))
    c, _, a, _ = g["exact_cutoff"]
    assert a.total == 100 and int(a.total * c["ratio"]) == 30 + 20 and a.min_loop == 11                 # ">": with ">=" it would be 21
    c, _, a, _ = g["clipped"]
    assert a.min_loop == 50 == max(l[3] for l in a.links)
    assert {c["vbin"] for c, _, _, _ in g.values()} >= {200, 333, 170} and {c["pbin"] for c, _, _, _ in g.values()} >= {1000000, 7000}
    for name in ("edges", "edges_track"):
        c, text, a, _ = g[name]
        pos = {int(ln.split(b"\t")[4]) for ln in text.split(b"\n") if ln and not ln.startswith(b"#") and ln.split(b"\t")[3] == b"chrEBV"}
        assert {1, 20000, c["vbin"] - 1, c["vbin"], c["vbin"] + 1} <= pos
        firsts = [ln.split("\t")[1] for ln in c["links"].splitlines()]
        assert firsts != sorted(firsts, key=int) and max(l[0] for l in a.links) >= 10                   # string order, not numeric
    c, text, a, _ = g["defaults"]
    seen = {ln.split(b"\t")[1] for ln in text.split(b"\n") if ln and not ln.startswith(b"#")}
    assert {b"chrX", b"chrM", b"chr1_KI270706v1_random", b"xchr7", b"chrEBV"} <= seen
    assert any(ln.split(b"\t")[1] == ln.split(b"\t")[3] == b"chrEBV" for ln in text.split(b"\n") if ln and not ln.startswith(b"#"))
    assert "xhs7" in g["edges"][0]["links"] and "xchr7" in g["edges"][0]["partners"]
    for bad in ("hsX", "hsM", "random"):
        assert all(bad not in c[k] for c, _, _, _ in g.values() for k in ("links", "partners"))


@pytest.mark.parametrize("k", range(len(vi.CASE_PARAMS)))
def test_definition_gives_the_reference_texts(k):
    c, text, names, a, b = golden()[k]
    bg, ln, pt = vd.ebv_texts(text, vi.table_text(), vi.VIEWPOINT, vi.PARTNER_RE, c["vbin"], c["pbin"], c["ratio"], c["track_bin"], c["min_count"])
    assert bg.decode() == c["bedgraph"]
    assert ln.decode() == c["links"]
    assert pt.decode() == c["partners"]


def _host(exe, c, names, a, b):
    f = [len(names), *names, vi.VIEWPOINT, c["vbin"], c["pbin"], c["track_bin"], c["min_count"], a.total, repr(c["ratio"])]
    f += [len(a.links)] + [x for l in a.links for x in l]
    f += [len(a.track)] + a.track
    cells = list(reversed(b.partners))                                            # in another order: the program orders them
    f += [len(cells)] + [x for cell in cells for x in cell]
    r = subprocess.run([exe], input=" ".join(map(str, f)).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    out = r.stdout
    head, _, rest = out.partition(b"\n")
    texts = {}
    while rest:
        lab, _, rest = rest.partition(b"\n")
        _, name, n = lab.split()
        texts[name.decode()], rest = rest[:int(n)], rest[int(n):]
    return head.decode(), texts


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_functions_give_the_reference_texts(san):
    util.ensure_built()
    exe = HOST_SAN if san else HOST
    assert os.path.exists(exe), exe
    for c, text, names, a, b in golden():
        head, texts = _host(exe, c, names, a, b)
        assert head == f"min_loop {a.min_loop} kept {a.links_kept}", (c["name"], head)
        for k in ("bedgraph", "links", "partners"):
            assert texts[k].decode() == c[k], (c["name"], k)


def test_host_refuses_links_past_63_bits():
    util.ensure_built()
    f = [1, "chrV", "chrV", 1 << 50, 1, 1, 1, 0, "0.01", 0, 2, 0, 0, 0]                     # 2 bins of 2^50 bp, times 5000
    r = subprocess.run([HOST], input=" ".join(map(str, f)).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 3 and b"63 bits" in r.stderr
