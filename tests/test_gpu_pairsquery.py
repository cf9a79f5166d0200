"""Region queries through the .px2 on the GPU (mkt_bgzf_query of include/mkt.h, microcket_amd.BgzfReader.query, bin/pairsquery).

Every region the reference's pairix answered (tests/golden/px2_golden.json, tests/golden/pairsquery_golden.json) is asked singly and as
one batch per case, without `run` (only the members of the plan are inflated) and after `run` (the resident text): the bytes are the
same by both routes and equal to the golden, and blocks_inflated is exactly the plan of tests/pairsquerydef.py.  The three-block
cases carry the edges of the compact buffer (a line across a member edge, a chunk from mid-member, a chunk that ends at a member end,
two runs of members)."""
import base64
import json
import os
import subprocess

import pytest

import inflate_cases
import matrixdef as md
import microcket_amd as m
import pairsquerydef as qd
import px2_inputs
import px2def
from test_pairsquery_host import CASES, GOLDEN, PX2, files, requests

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(m.lib_path()), "bin")


def reader(gz, px2, run=False):
    r = m.BgzfReader()
    r.add(gz)
    r.load_index(px2)
    if run:
        r.run()
    return r


def check(r, f, regions, flip, resident, entry=None):
    """one query against the definition (and the golden entry): the bytes per region, the counters, the plan"""
    info = {}
    want = f.answer(regions, flip, info)
    got = r.query(regions, autoflip=flip)
    assert got == [qd.printed(a) for a in want], (regions, flip, resident)
    if entry is not None:
        assert qd.same_as_golden(entry, b"".join(got).split(b"\n")[:-1]), (regions, flip)
    qi = r.query_info
    assert (qi.regions, qi.subqueries, qi.chunks, qi.candidate_lines, qi.lines, qi.unparsed) == \
           (len(regions), info["subqueries"], info["chunks"], info["candidate_lines"], info["lines"], info["unparsed"]), (regions, qi)
    assert (qi.blocks_inflated, qi.bytes_inflated) == ((0, 0) if resident else (info["blocks_inflated"], info["bytes_inflated"])), (regions, qi)
    assert qi.answer_bytes == sum(len(g) for g in got) and r.query_counts() == [len(a) for a in want]
    return got


@pytest.mark.parametrize("cut,level", [("bgzip", 6), ("ff00", 1)])
@pytest.mark.parametrize("name", CASES)
def test_every_golden_region_by_both_routes(name, cut, level):
    gz, px2 = files(name, cut, level)
    f = qd.File(gz, px2)
    with reader(gz, px2) as sel, reader(gz, px2, run=True) as res:
        for regions, flip, entry in requests(name):
            a = check(sel, f, regions, flip, False, entry)
            assert check(res, f, regions, flip, True, entry) == a
        assert [n.decode("latin-1") for n in sel.names()] == GOLDEN[name]["l"]["lines"]
        assert sel.count() == PX2[name]["n"]
        t = sel.query_timing_ms()
        assert set(t) == {"inflate_selected", "filter_gather"} and set(sel.timing_ms()) == {"table_upload", "inflate", "crc"}


@pytest.mark.parametrize("name", ["blocks_long_runs", "blocks_many_bins"])
def test_compact_buffer_edges_of_the_three_block_cases(name):
    gz, px2 = files(name, "ff00", 1)
    f = qd.File(gz, px2)
    text = px2_inputs.case(name)["text"]
    edge = 2 * px2_inputs.BLOCK                                   # a line straddles this member edge
    a = text.rfind(b"\n", 0, edge) + 1
    pos = int(text[a:text.find(b"\n", a)].split(b"\t")[2])
    with reader(gz, px2) as r:
        got = check(r, f, ["chr1:%d-%d|chr1" % (pos, pos)], False, False)
        assert text[a:text.find(b"\n", a) + 1] in got[0] and {1, 2} <= set(f.plan(["chr1:%d-%d|chr1" % (pos, pos)])["members"])
        # a chunk from mid-member that ends exactly at the end of member 0: member 1 stays out
        last0 = text.rfind(b"\n", 0, px2_inputs.BLOCK - 1) + 1
        p0 = int(text[last0:px2_inputs.BLOCK].split(b"\t")[2])
        q = "chr1:%d-%d|chr1" % (p0, p0)
        assert f.plan([q])["members"] == [0] and any(z == px2_inputs.BLOCK and x > 0 for _, x, z in f.plan([q])["spans"])
        assert check(r, f, [q], False, False)[0].endswith(text[last0:px2_inputs.BLOCK])
        # members 0 and 3: two runs in the compact buffer
        two = ["chr1:1-65536|chr1", "chr1|chr2", "chr1:1-65536|*"]
        assert f.plan(two)["runs"] == 2 and f.plan(two)["members"] == [0, 3]
        check(r, f, two, False, False)
        assert r.query_info.blocks_inflated == 2
        # everything at once, then the same object again on the resident text
        both = check(r, f, ["chr1|*", "*|chr2", "chr1|chr1"], False, False)
        r.run()
        assert check(r, f, ["chr1|*", "*|chr2", "chr1|chr1"], False, True) == both


def test_empty_batch_and_a_thousand_copies():
    gz, px2 = files("many_pairs", "bgzip", 6)
    f = qd.File(gz, px2)
    with reader(gz, px2) as r:
        assert r.query([]) == [] and r.query_info.answer_bytes == 0 and r.query_info.blocks_inflated == 0
        assert r.query_device()[1] == 0
        one = check(r, f, ["chr1:1-100000|chr2:1-100000"], False, False)
        many = check(r, f, ["chr1:1-100000|chr2:1-100000"] * 1000, False, False)
        assert many == one * 1000 and r.query_info.blocks_inflated == 1
        assert r.query(["chr1:1-100000|chr2:1-100000"] * 1000) == many                      # the same bytes on every call


def test_special_cases_of_the_definition():
    for name, region, tail in (("no_final_newline", "chr1:60000-80000|chr2:1-10", px2_inputs.case("no_final_newline")["text"].split(b"\n")[-1] + b"\n"), ("meta_in_middle", "a:1-100000|b:1-10", None),
                               ("large_positions", "chr1:1-1|chr1:1-10", None), ("large_positions", "chr1:1-1073741825|chr1", None), ("header_only", "chr1|chr1", None)):
        gz, px2 = files(name, "ff00", 1)
        with reader(gz, px2) as r:
            got = check(r, qd.File(gz, px2), [region], False, False)[0]
            assert b"#" not in got and (tail is None or got.endswith(tail))
    with reader(*files("header_only", "ff00", 1)) as r:
        assert r.names() == [] and r.query(["chr1|*"]) == [b""]


def test_refused_regions_name_their_index_and_leave_no_answer():
    gz, px2 = files("many_pairs", "bgzip", 6)
    with reader(gz, px2) as r:
        for bad in qd.REFUSED:
            with pytest.raises(m.MktError, match="region 2: ") as e:
                r.query(["chr1|chr1", "chr1|chr2", bad, "chr2|chr2"])
            with pytest.raises(qd.RegionError) as d:
                qd.parse_region(bad, 2)
            assert d.value.what in str(e.value) and r.query_info is None
            with pytest.raises(m.MktError):
                r.query_device()
        assert r.query(["chr1|chr2"], autoflip=True) == r.query(["chr2|chr1"], autoflip=True) != [b""]
        assert r.query(["chr2|chr1"]) == [b""]


@pytest.mark.parametrize("level", [0, 1, 2])
def test_files_of_pairsgz_with_their_own_index(level):
    for name in ("many_pairs", "blocks_many_bins", "no_final_newline"):
        with m.PairsGz() as g:
            g.add(px2_inputs.case(name)["text"])
            g.run(level=level)
            gz, px2 = g.gz_bytes(), g.px2_bytes()
        f = qd.File(gz, px2)
        with reader(gz, px2) as r:
            for regions, flip, entry in requests(name):
                check(r, f, regions, flip, False, entry)


def test_bytes_of_the_reference_bgzip_with_an_index_of_px2def():
    with open(os.path.join(HERE, "golden", "inflate_golden.json")) as fh:
        g = json.load(fh)
    for key in sorted(g):
        gz = base64.b64decode(g[key]["gz_base64"])
        name = g[key]["case"]
        px2 = px2def.bgzf_compress(px2def.serialize(px2def.build_index(px2_inputs.case(name)["text"], px2def.bgzf_blocks(gz, check=False), len(gz))))
        f = qd.File(gz, px2)
        with reader(gz, px2) as r:
            for regions, flip, entry in requests(name):
                check(r, f, regions, flip, False, entry)


def test_unparsed_records_are_counted_and_left_out():
    good = px2_inputs.HEADER + px2_inputs.rec(1, "chr1", 10, "chr1", 20) + px2_inputs.rec(2, "chr1", 11, "chr1", 21)
    bad = good + b"r3\tchr1\t12\tchr1\t2x\t+\t-\n" + b"\n" + b"r5\tchr1\t13\n" + px2_inputs.rec(6, "chr1", 14, "chr1", 99999999999) + px2_inputs.rec(7, "chr1", 15, "chr1", 25)
    gz = px2def.bgzf_compress(bad, 6)
    ix = px2def.build_index(good, px2def.bgzf_blocks(gz, check=False), len(gz))
    (x, _), = ix["bins"][0][4681]
    ix["bins"][0][4681] = [(x, len(gz) << 16)]
    px2 = px2def.bgzf_compress(px2def.serialize(ix))
    for run in (False, True):
        with reader(gz, px2, run=run) as r:
            got = check(r, qd.File(gz, px2), ["chr1|chr1"], False, run)[0]
            assert [ln.split(b"\t")[0] for ln in got.split(b"\n")[:-1]] == [b"r1", b"r2", b"r7"] and r.query_info.unparsed == 4


def test_index_and_file_errors():
    gz, px2 = files("blocks_long_runs", "ff00", 1)
    _, other = files("blocks_many_bins", "bgzip", 6)
    with m.BgzfReader() as r:
        with pytest.raises(m.MktError, match="call order violated"):
            r.query(["chr1|chr1"])                               # no file
        r.add(gz)
        with pytest.raises(m.MktError, match="call order violated"):
            r.query(["chr1|chr1"])                               # no index
        r.load_index(other)
        with pytest.raises(m.MktError, match="does not belong to this file"):
            r.query(["chr1|chr1"])
        r.load_index(px2)                                        # the file stays
        assert r.query(["chr1|chr2"])[0]
    with m.BgzfReader() as r:
        with pytest.raises(m.MktError, match="call order violated"):
            r.load_index(px2) or r.query(["chr1|chr1"])          # an index, no file
    # a member of the plan with a corrupted CRC: reason and offset; a region elsewhere is still answered by the same object
    f = qd.File(gz, px2)
    c = f.blocks[1][0]
    broken = bytearray(gz)
    broken[c + f.blocks[1][1] - 8] ^= 0x55
    with reader(bytes(broken), px2) as r:
        with pytest.raises(m.BgzfRefused) as e:
            r.query(["chr1|chr1"])
        assert (e.value.reason, e.value.offset) == ("crc", c) and "block at %d" % c in str(e.value) and r.query_info is None
        assert f.plan(["chr1|chr2"])["members"] == [3]
        assert r.query(["chr1|chr2"]) == [qd.printed(f.answer(["chr1|chr2"])[0])]


def test_device_answer_feeds_the_matrix():
    lines = [ln for ln in md.HAND_PAIRS.split(b"\n") if ln]
    recs = sorted((ln for ln in lines if ln[:1] != b"#"), key=lambda ln: (ln.split(b"\t")[1], ln.split(b"\t")[3], int(ln.split(b"\t")[2])))
    text = b"".join(ln + b"\n" for ln in [ln for ln in lines if ln[:1] == b"#"] + recs)          # the hand-made pairs, each pair contiguous
    gz = px2def.bgzf_compress(text, 6, cuts=[101, 300])
    px2 = px2def.bgzf_compress(px2def.serialize(px2def.build_index(text, px2def.bgzf_blocks(gz, check=False), len(gz))))
    f = qd.File(gz, px2)
    regions = [n.decode("latin-1") for n in f.ix["names"]]
    with m.Matrix(md.HAND_TABLE, [100, 1000]) as plain, m.Matrix(md.HAND_TABLE, [100, 1000]) as dev, reader(gz, px2) as r:
        ans = b"".join(r.query(regions))
        assert ans and ans == b"".join(qd.printed(a) for a in f.answer(regions))
        plain.add(ans)
        d, n = r.query_device()
        assert n == len(ans)
        dev.add_device(d, n)
        assert dev.run() == plain.run() and [dev.text(k) for k in range(2)] == [plain.text(k) for k in range(2)]


def test_pairsquery_executable(tmp_path):
    exe = os.path.join(BIN, "pairsquery")
    gz, px2 = files("many_pairs", "bgzip", 6)
    g = GOLDEN["many_pairs"]
    fa = tmp_path / "in.pairs.gz"
    fa.write_bytes(gz)
    (tmp_path / "in.pairs.gz.px2").write_bytes(px2)

    def run(*args):
        r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        return r.returncode, r.stdout, r.stderr.decode()

    def out(entry):
        return "".join(ln + "\n" for ln in entry["lines"]).encode("latin-1")

    asked = ["chr1:1-100000|*", "*|chr1:1-100000", "chr2|chr1"] + [q for q in g["single"] if "," in q]      # stars, an absent pair whose flip is present, commas
    assert len(asked) == 4
    for q in asked:
        assert run(str(fa), q)[:2] == (0, out(g["single"][q])), q
    flips = [q for q in g["autoflip"] if q in ("zz|chr1", "chr2|chr1") or q.startswith("chr2:1-200000|")]      # absent; flipped, whole and with ranges
    assert len(flips) == 3 and g["autoflip"]["chr2|chr1"]["lines"]
    for q in flips:
        assert run("-a", str(fa), q)[:2] == (0, out(g["autoflip"][q])), q
    assert run(str(fa), *g["batch"]["regions"])[:2] == (0, out(g["batch"]))
    (tmp_path / "regions.txt").write_text("".join(q + "\n" for q in g["batch"]["regions"]))
    assert run("-L", str(fa), str(tmp_path / "regions.txt"))[:2] == (0, out(g["L"]))
    assert run("-l", str(fa))[:2] == (0, out(g["l"]))
    assert run("-n", str(fa))[:2] == (0, b"%d\n" % PX2["many_pairs"]["n"])
    rc, so, se = run(str(fa), "chr1|chr1", "chr1:10-5|chr2")
    assert (rc, so) == (1, b"") and "region 1: " in se
    assert run()[0] == 1 and run("-x", str(fa))[0] == 1
    fa.write_bytes(inflate_cases.case("wrong_crc")["gz"])
    rc, so, se = run(str(fa), "chr1|chr1")
    assert (rc, so) == (3, b"") and "does not belong" in se
    _, other = files("blocks_long_runs", "ff00", 1)
    bad = bytearray(files("blocks_long_runs", "ff00", 1)[0])
    blocks = px2def.bgzf_blocks(bytes(bad), check=False)
    bad[blocks[0][0] + blocks[0][1] - 8] ^= 1
    fa.write_bytes(bytes(bad))
    (tmp_path / "in.pairs.gz.px2").write_bytes(other)
    rc, so, se = run(str(fa), "chr1:1-100|chr1")
    assert (rc, so) == (3, b"") and "[crc]" in se and "block at 0" in se
