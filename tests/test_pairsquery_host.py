"""Region queries through the .px2, host side (no GPU): tests/pairsquerydef.py against what the reference's pairix answered
(tests/golden/px2_golden.json, tests/golden/pairsquery_golden.json), and the stand-alone driver of csrc/mkt_px2query.h
(tests/host/pairsquery_host.cpp: region grammar, index, block plan, shared line filter), plain and under ASan/UBSan, against the
definition: the same answers and the same set of members to inflate."""
import functools
import json
import os
import subprocess

import pytest

import pairsquerydef as qd
import px2_inputs
import px2def

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "px2_golden.json")) as f:
    PX2 = json.load(f)
with open(os.path.join(HERE, "golden", "pairsquery_golden.json")) as f:
    GOLDEN = json.load(f)
CASES = [c["name"] for c in px2_inputs.accepted()]
CUTS = ["bgzip", "ff00"]


@functools.lru_cache(maxsize=None)
def files(name, cut, level):
    """(gz, px2) of a case: cut where the reference's bgzip cut it, or every 0xff00 bytes"""
    text = px2_inputs.case(name)["text"]
    gz = px2def.bgzf_compress(text, level, cuts=PX2[name]["bgzip_block_starts"][1:] if cut == "bgzip" else None)
    return gz, px2def.bgzf_compress(px2def.serialize(px2def.build_index(text, px2def.bgzf_blocks(gz, check=False), len(gz))))


def requests(name):
    """[(regions, autoflip, golden entry)] of a case: every recorded region singly, then the batch"""
    g = GOLDEN[name]
    out = [([q], False, {"lines": lines}) for q, lines in PX2[name]["queries"].items()]
    out += [([q], False, e) for q, e in g["single"].items()] + [([q], True, e) for q, e in g["autoflip"].items()]
    return out + [(g["batch"]["regions"], False, g["batch"]), (g["batch"]["regions"], False, g["L"])]


@pytest.mark.parametrize("cut,level", [("bgzip", 6), ("ff00", 1), ("ff00", 9)])
@pytest.mark.parametrize("name", CASES)
def test_definition_answers_every_golden_region(name, cut, level):
    f = qd.File(*files(name, cut, level))
    for regions, flip, entry in requests(name):
        assert qd.same_as_golden(entry, [ln for r in f.answer(regions, flip) for ln in r]), (regions, flip)
    assert [n.decode("latin-1") for n in f.ix["names"]] == GOLDEN[name]["l"]["lines"]
    # and px2def's own single-region query agrees wherever the second side has a range or nothing lies behind 2^30
    for q, lines in PX2[name]["queries"].items():
        assert [ln.decode("latin-1") for ln in f.answer([q])[0]] == lines == px2def.query(f.gz, files(name, cut, level)[1], q)


def test_block_cases_have_the_shapes_the_plan_is_about():
    for name in ("blocks_long_runs", "blocks_many_bins"):
        f = qd.File(*files(name, "ff00", 1))
        n = len(f.blocks) - 1                                       # without the EOF block
        assert n >= 4
        whole = f.plan(["chr1|chr1"])
        ends = [f.blocks[k][2] + f.blocks[k][3] for k in range(n)]
        assert any(z in ends for _, _, z in whole["spans"])         # a chunk that ends exactly at a member end
        assert any(a not in [b[2] for b in f.blocks] for _, a, _ in whole["spans"])     # a chunk that begins mid-member
        two = f.plan(["chr1:1-65536|chr1", "chr1|chr2"])
        assert two["runs"] == 2 and two["members"][0] == 0 and two["members"][-1] == n - 1


def drivers():
    d = os.path.join(HERE, "host", "_build")
    exes = [os.path.join(d, "pairsquery_host"), os.path.join(d, "pairsquery_host_san")]
    if not all(os.path.exists(e) for e in exes):
        from microcket_amd import build
        build.build_test_tools()
    return exes


def run_driver(exe, tmp_path, gz, px2, regions, flip=False):
    (tmp_path / "in.gz").write_bytes(gz)
    (tmp_path / "in.px2").write_bytes(px2)
    (tmp_path / "regions.txt").write_bytes("\n".join(regions).encode("latin-1"))
    r = subprocess.run([exe] + (["-a"] if flip else []) + [str(tmp_path / "in.gz"), str(tmp_path / "in.px2"), str(tmp_path / "regions.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def expected_stdout(f, regions, flip):
    info = {}
    ans = f.answer(regions, flip, info)
    p = f.plan(regions, flip)
    head = "members%s\nruns %d\ncandidates %d unparsed %d\n" % ("".join(" %d" % k for k in p["members"]), p["runs"], info["candidate_lines"], info["unparsed"])
    return head.encode() + b"".join(b"region %d %d\n" % (r, len(a)) + qd.printed(a) for r, a in enumerate(ans))


@pytest.mark.parametrize("name", CASES)
def test_driver_prints_the_definitions_answers_and_members(name, tmp_path):
    for cut, level in (("bgzip", 6), ("ff00", 1)):
        gz, px2 = files(name, cut, level)
        f = qd.File(gz, px2)
        for exe in drivers():
            for regions, flip, entry in requests(name)[:-1]:
                out = run_driver(exe, tmp_path, gz, px2, regions, flip)
                assert out == expected_stdout(f, regions, flip), (exe, regions, flip)


def test_driver_plans_two_runs_and_counts_unparsed(tmp_path):
    gz, px2 = files("blocks_long_runs", "ff00", 1)
    f = qd.File(gz, px2)
    regions = ["chr1:1-65536|chr1", "chr1|chr2", "chr1:1-65536|*", "*|chr2:1-5000"]
    for exe in drivers():
        assert run_driver(exe, tmp_path, gz, px2, regions) == expected_stdout(f, regions, False)
    # a pos2 that is no number, an empty line and a short line inside a scanned chunk: an index built by hand over such a text
    good = px2_inputs.HEADER + px2_inputs.rec(1, "chr1", 10, "chr1", 20) + px2_inputs.rec(2, "chr1", 11, "chr1", 21)
    bad = good + b"r3\tchr1\t12\tchr1\t2x\t+\t-\n" + b"\n" + b"r5\tchr1\t13\n" + px2_inputs.rec(6, "chr1", 14, "chr1", 99999999999) + px2_inputs.rec(7, "chr1", 15, "chr1", 25)
    gz = px2def.bgzf_compress(bad, 6)
    ix = px2def.build_index(good, px2def.bgzf_blocks(gz, check=False), len(gz))
    (x, _), = ix["bins"][0][4681]
    ix["bins"][0][4681] = [(x, len(gz) << 16)]
    px2 = px2def.bgzf_compress(px2def.serialize(ix))
    f = qd.File(gz, px2)
    info = {}
    assert [ln.split(b"\t")[0] for ln in f.answer(["chr1|chr1"], False, info)[0]] == [b"r1", b"r2", b"r7"] and info["unparsed"] == 4
    for exe in drivers():
        assert run_driver(exe, tmp_path, gz, px2, ["chr1|chr1"]) == expected_stdout(f, ["chr1|chr1"], False)


def test_refused_regions_name_their_index(tmp_path):
    gz, px2 = files("many_pairs", "bgzip", 6)
    names = qd.File(gz, px2).ix["names"]
    assert set(qd.REFUSED) == set(GOLDEN["_refused"])                 # what pairix did with them is recorded as data
    for bad in qd.REFUSED:
        batch = ["chr1|chr1", "chr1|chr2", bad, "chr2|chr2"]
        with pytest.raises(qd.RegionError) as e:
            for r, q in enumerate(batch):
                qd.expand(names, q, False, r)
        assert e.value.index == 2
        for exe in drivers():
            assert run_driver(exe, tmp_path, gz, px2, batch) == ("refused arg region 2: %s\n" % e.value.what).encode()


def test_index_of_another_file_is_refused(tmp_path):
    gz, _ = files("blocks_long_runs", "ff00", 1)
    _, other = files("blocks_many_bins", "bgzip", 6)
    with pytest.raises(ValueError, match="does not belong"):
        qd.File(gz, other).answer(["chr1|chr1"])
    for exe in drivers():
        assert run_driver(exe, tmp_path, gz, other, ["chr1|chr1"]) == b"refused format the index does not belong to this file\n"
