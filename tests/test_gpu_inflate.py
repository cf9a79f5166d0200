"""BGZF read back on the GPU (mkt_bgzf_* of include/mkt.h, microcket_amd.BgzfReader, bin/pairsgunzip, pairs2matrix on .gz input).

Every directed case of tests/inflate_cases.py and every file the reference's bgzip wrote (tests/golden/inflate_golden.json) goes
through the reader: the text, the counters and the refusals with their reason and offset.  What this project's own writers make
(PairsGz at its three levels, sam2bam) inflates back to what went in; the device text feeds the pair comparison and the matrix
binning; the executables write the same bytes."""
import base64
import json
import os
import subprocess

import pytest

import bamio
import inflate_cases
import matrixdef as md
import microcket_amd as m
import px2_inputs
import px2def
from test_inflate_host import deflate_kinds

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(m.lib_path()), "bin")
with open(os.path.join(HERE, "golden", "inflate_golden.json")) as f:
    GOLDEN = json.load(f)
with open(os.path.join(HERE, "golden", "paircmp_golden.json")) as f:
    PAIRCMP = json.load(f)
with open(os.path.join(HERE, "golden", "px2_golden.json")) as f:
    PX2 = json.load(f)


def read(gz, piece=None):
    with m.BgzfReader() as r:
        for k in range(0, len(gz), piece or max(len(gz), 1)):
            r.add(gz[k:k + (piece or len(gz))])
        info = r.run()
        return r.text(), info


def check_file(gz, text, name):
    got, info = read(gz)
    assert got == text, name
    blocks = px2def.bgzf_blocks(gz, check=False)
    assert (info.blocks, info.gz_bytes, info.text_bytes) == (len(blocks), len(gz), len(text)), name
    assert [info.stored, info.fixed, info.dynamic] == deflate_kinds(gz), name
    assert info.has_eof == (1 if gz[-28:] == px2def.BGZF_EOF else 0), name


@pytest.mark.parametrize("name", [c["name"] for c in inflate_cases.accepted()])
def test_directed_cases_inflate(name):
    c = inflate_cases.case(name)
    check_file(c["gz"], c["text"], name)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_files_of_the_reference_bgzip_inflate(name):
    g = GOLDEN[name]
    check_file(base64.b64decode(g["gz_base64"]), px2_inputs.case(g["case"])["text"], name)


@pytest.mark.parametrize("name", [c["name"] for c in inflate_cases.refused()])
def test_refused_cases_name_reason_and_offset(name):
    c = inflate_cases.case(name)
    with m.BgzfReader() as r:
        r.add(c["gz"])
        with pytest.raises(m.BgzfRefused) as e:
            r.run()
        assert (e.value.reason, e.value.offset) == (c["refused"], inflate_cases.refused_offset(c))
        assert "block at %d" % e.value.offset in str(e.value)
        if c["refused"] == "plain_gzip":
            assert "not BGZF" in str(e.value)
        assert r.info is None
        with pytest.raises(m.MktError):
            r.text()
        with pytest.raises(m.MktError):
            r.device_text()
        # the same object reads a good file afterwards
        good = inflate_cases.case("dynamic_level6")
        r.close()
    check_file(good["gz"], good["text"], "after a refusal")


def test_any_chunking_and_a_second_run_give_the_same_text():
    c = inflate_cases.case("many_members_odd_offsets")
    for piece in (1000, 65537):
        assert read(c["gz"], piece)[0] == c["text"]
    with m.BgzfReader() as r:
        r.add(c["gz"])
        a = r.run()
        assert r.run() == a and r.text() == c["text"]
        t = r.timing_ms()
        assert set(t) == {"table_upload", "inflate", "crc"} and t["inflate"] > 0
        more = inflate_cases.case("isize_1")
        r.add(more["gz"])
        with pytest.raises(m.MktError):
            r.text()                                         # stale: the file has grown
        r.run()
        assert r.text() == c["text"] + more["text"]


@pytest.mark.parametrize("level", [0, 1, 2])
def test_round_trip_of_pairsgz(level):
    for c in px2_inputs.accepted():
        with m.PairsGz() as g:
            g.add(c["text"])
            g.run(level=level)
            gz, px2 = g.gz_bytes(), g.px2_bytes()
        with m.BgzfReader() as r:
            r.add(gz)
            info = r.run()
            assert r.text() == c["text"], c["name"]
            assert info.has_eof == 1 and info.blocks == len(px2def.bgzf_blocks(gz, check=False))
            assert (info.stored > 0, info.fixed > 0, info.dynamic > 0)[level] or not c["text"]
            r.load_index(px2)
            assert r.count() == PX2[c["name"]]["n"] == px2def.count_lines(px2)


def test_index_that_is_no_index_is_refused():
    c = px2_inputs.case("many_pairs")
    with m.BgzfReader() as r:
        with pytest.raises(m.MktError):
            r.count()
        with pytest.raises(m.MktError):
            r.load_index(px2def.bgzf_compress(c["text"], 1))          # BGZF, but a .pairs text
        good = px2def.bgzf_compress(px2def.serialize(px2def.build_index(c["text"], px2def.bgzf_blocks(px2def.bgzf_compress(c["text"])), len(px2def.bgzf_compress(c["text"])))))
        with pytest.raises(m.MktError):
            r.load_index(good[:-28] + px2def.bgzf_compress(b"x"))     # bytes behind the last linear index
        r.load_index(good)
        assert r.count() == PX2["many_pairs"]["n"]


def test_sam2bam_output_inflates_to_what_bamio_reads():
    body = "".join("r%03d\t0\tchr1\t%d\t30\t10M\t*\t0\t0\tACGTACGTAC\tFFFFFFFFFF\n" % (k, 100 + 37 * k) for k in range(300)).encode()
    hdr = b"@HD\tVN:1.5\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000\n"
    for level in (0, 2):
        bam = m.sam_to_bam(hdr + body, sorted=True, level=level)[0]
        want = b"".join(raw for _, _, raw in bamio.bgzf_blocks(bam))
        got, info = read(bam)
        assert got == want and got[:4] == b"BAM\1" and info.has_eof == 1
        assert len(bamio.Bam(bam).records) == 300


def test_device_text_feeds_the_pair_comparison_and_the_matrix():
    c = PAIRCMP["cases"][0]
    import paircmp_inputs as pi
    a, b = pi.make(c["gen"])
    with m.PairCompare() as plain, m.PairCompare() as dev, m.BgzfReader() as ra, m.BgzfReader() as rb:
        plain.add_a(a)
        plain.add_b(b)
        want = plain.run()
        ra.add(px2def.bgzf_compress(a, 6))
        rb.add(px2def.bgzf_compress(b, 1))
        ra.run()
        rb.run()
        dev.add_device("a", *ra.device_text())
        dev.add_device("b", *rb.device_text())
        assert dev.run() == want and dev.report("{A}", "{B}") == plain.report("{A}", "{B}") and dev.lines() == plain.lines()
    with m.Matrix(md.HAND_TABLE, [100, 1000]) as plain, m.Matrix(md.HAND_TABLE, [100, 1000]) as dev, m.BgzfReader() as r:
        plain.add(md.HAND_PAIRS)
        r.add(px2def.bgzf_compress(md.HAND_PAIRS, 6, cuts=[101, 300]))
        r.run()
        dev.add_device(*r.device_text())
        assert dev.run() == plain.run()
        assert [dev.text(k) for k in range(2)] == [plain.text(k) for k in range(2)] and dev.text(0) == md.HAND_COO


def test_pairsgunzip_to_a_file_to_stdout_and_into_pairscmp(tmp_path):
    exe = os.path.join(BIN, "pairsgunzip")
    c = PAIRCMP["cases"][2]
    import paircmp_inputs as pi
    a, b = pi.make(c["gen"])
    fa, fb, out = tmp_path / "a.pairs.gz", tmp_path / "b.pairs", tmp_path / "a.txt"
    fa.write_bytes(px2def.bgzf_compress(a, 6))
    fb.write_bytes(b)
    r = subprocess.run([exe, str(fa), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == a, r.stderr.decode()
    r = subprocess.run([exe, str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stdout == a, r.stderr.decode()
    with open(fa, "rb") as f:
        r = subprocess.run([exe, "-", "-"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and r.stdout == a
    # the pipe that stands in for the script's pigz: pairsgunzip a.gz | pairscmp - b
    args = [os.path.join(BIN, "pairscmp"), "-", str(fb)] + ([c["dist"]] if c["dist"] is not None else [])
    p1 = subprocess.Popen([exe, str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p2 = subprocess.run(args, stdin=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    p1.stdout.close()
    assert p1.wait(timeout=60) == 0 and p2.returncode == 0, p2.stderr.decode()
    assert p2.stdout.decode() == c["stdout"].replace("{A}", "-").replace("{B}", str(fb))
    # a refused file: the reason and the offset on stderr, nothing written
    bad = inflate_cases.case("wrong_crc")
    fa.write_bytes(bad["gz"])
    out.unlink()
    r = subprocess.run([exe, str(fa), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 3 and r.stdout == b"" and not out.exists()
    assert "[crc]" in r.stderr.decode() and "block at %d" % inflate_cases.refused_offset(bad) in r.stderr.decode()
    fa.write_bytes(inflate_cases.case("plain_gzip")["gz"])
    r = subprocess.run([exe, str(fa)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 3 and "not BGZF" in r.stderr.decode()


def test_pairs2matrix_reads_gz_by_its_magic(tmp_path):
    exe = os.path.join(BIN, "pairs2matrix")
    table = tmp_path / "genome.sizes"
    table.write_bytes(md.HAND_TABLE)
    other = md.HAND_PAIRS.replace(b"\t120\t", b"\t130\t")
    nonl = md.HAND_PAIRS.rstrip(b"\n")                         # a last line without its newline goes the way of plain text
    files = {"in.pairs": md.HAND_PAIRS, "in.bin": px2def.bgzf_compress(md.HAND_PAIRS, 6, cuts=[97]), "other.pairs": other, "other.pairs.gz": px2def.bgzf_compress(other, 1),
             "nonl.pairs": nonl, "nonl.gz": px2def.bgzf_compress(nonl, 6)}
    for k, v in files.items():
        (tmp_path / k).write_bytes(v)

    def run(tag, *args):
        pre = tmp_path / tag
        r = subprocess.run([exe, "-g", str(table), "-r", "100,1000", "-o", str(pre), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return {f[len(tag):]: (tmp_path / f).read_bytes() for f in sorted(os.listdir(tmp_path)) if f.startswith(tag + ".")}

    want = run("t", str(tmp_path / "in.pairs"))
    assert want[".100.coo"] == md.HAND_COO
    assert run("g", str(tmp_path / "in.bin")) == want
    assert run("n", str(tmp_path / "nonl.gz")) == run("m", str(tmp_path / "nonl.pairs")) == want
    both = run("c", str(tmp_path / "in.pairs"), "--compare", str(tmp_path / "other.pairs"))
    assert ".scc.stat" in both
    assert run("d", str(tmp_path / "in.bin"), "--compare", str(tmp_path / "other.pairs.gz")) == both
    (tmp_path / "bad.gz").write_bytes(inflate_cases.case("ll_oversubscribed")["gz"])
    r = subprocess.run([exe, "-g", str(table), "-r", "100", "-o", str(tmp_path / "x"), str(tmp_path / "bad.gz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 12 and "[ll_oversubscribed]" in r.stderr.decode()
