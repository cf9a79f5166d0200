"""BAM read back on the GPU (mkt_bamtext_* of include/mkt.h, microcket_amd.BamReader, bam_to_sam, bin/bam2sam): the text and the header
equal what the reference's samtools printed (tests/golden/bamtext_golden.json) for every golden file; sam2bam's output decodes back to
its sorted lines; `bam2sam | sam2pairs` writes what sam2pairs writes on the SAM text."""
import os
import struct
import subprocess

import pytest

import bamdef
import bamio
import bamtext_cases as bc
import bamtextdef as bd
import microcket_amd as m
import util

GOLDEN, unz, golden_raw = bc.golden(), bc.unz, bc.golden_raw

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(m.lib_path()), "bin")
EXE = os.path.join(BIN, "bam2sam")


def golden_bam(key):
    return unz(GOLDEN[key]["bam"]) if key.startswith("sam/") else bc.bgzf(bc.case(key[5:])["raw"])


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_text_and_header_equal_samtools(key):
    bam, g = golden_bam(key), GOLDEN[key]
    assert m.bam_to_sam(bam) == unz(g["view"])
    assert m.bam_to_sam(bam, header=True) == unz(g["view_h"])
    with m.BamReader() as r:
        r.add(golden_raw(key))
        info = r.run()
        r.finish()
        assert r.header() == unz(g["view_H"]) and r.text() == unz(g["view"])
        assert info.records == unz(g["view"]).count(b"\n") and info.carry_bytes == 0 and info.header_done == 1
        assert r.refs() == bd.header(golden_raw(key))[1]


@pytest.mark.parametrize("key", ["sam/edge_unc.sam", "case/floats", "case/text_without_newline", "case/no_records"])
def test_bam2sam_prints_what_samtools_prints(key, tmp_path):
    g, path = GOLDEN[key], tmp_path / "x.bam"
    path.write_bytes(golden_bam(key))
    env = dict(os.environ, MKT_BAM2SAM_BATCH="65536")      # (these files are one batch each; test_bam2sam_in_many_batches has the batch loop)
    for flags, k in (([], "view"), (["-h"], "view_h"), (["-H"], "view_H")):
        r = subprocess.run([EXE] + flags + [str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, env=env)
        assert r.returncode == 0 and r.stdout == unz(g[k]), (flags, r.stderr.decode())
        with open(path, "rb") as f:
            r = subprocess.run([EXE] + flags + ["-"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0 and r.stdout == unz(g[k]), (flags, r.stderr.decode())


BATCH = 65536


def batches_of(bam, batch=BATCH):
    """the inflated bytes of each batch bam2sam makes of the file: it fills its buffer to `batch` bytes and takes the whole members"""
    members, p = [], 0
    while p < len(bam):
        bsize = struct.unpack_from("<H", bam, p + 16)[0] + 1
        members.append((bsize, struct.unpack_from("<I", bam, p + bsize - 4)[0]))
        p += bsize
    out, k, left, pend = [], 0, len(bam), 0
    while left or pend:
        take = min(batch - pend, left)
        pend, left = pend + take, left - take
        inflated = 0
        while k < len(members) and members[k][0] <= pend:
            pend -= members[k][0]
            inflated += members[k][1]
            k += 1
        out.append(inflated)
    return out


def test_bam2sam_in_many_batches(tmp_path):
    """A file of 25 batches: whole members per batch, the record a batch ends in carried into the next, the reader cleared in between."""
    c = bc.big_case()
    assert len(c["bam"]) > 20 * BATCH and len(batches_of(c["bam"])) > 20
    want, path = b"".join(c["lines"]), tmp_path / "big.bam"
    path.write_bytes(c["bam"])
    env = dict(os.environ, MKT_BAM2SAM_BATCH=str(BATCH))
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout == want, r.stderr.decode()[-300:]
    assert ("%d records in %d batches" % (len(c["lines"]), len(batches_of(c["bam"])))) in r.stderr.decode()
    with open(path, "rb") as f:
        r = subprocess.run([EXE, "-h", "-"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout == bc.TEXT + want, r.stderr.decode()[-300:]
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)      # one batch: the same bytes
    assert r.returncode == 0 and r.stdout == want


def test_refusal_in_a_later_batch_leaves_the_earlier_ones_written(tmp_path):
    bad_at = 60000
    c, good = bc.big_case(bad_at), bc.big_case()
    path = tmp_path / "bad.bam"
    path.write_bytes(c["bam"])
    # the lines of the records that end inside the batches in front of the one that holds the refused record
    ends, fed, written = [], 0, 0
    off = bc.START
    for ln_rec in range(bad_at):
        off += 4 + struct.unpack_from("<I", c["raw"], off)[0]
        ends.append(off)
    assert off == c["bad_offset"]
    bad_end = off + 4 + struct.unpack_from("<I", c["raw"], off)[0]
    for inflated in batches_of(c["bam"]):
        if fed + inflated >= bad_end:                   # the run that holds the whole refused record writes nothing
            break
        fed += inflated
    written = sum(1 for e in ends if e <= fed)
    assert 0 < written < bad_at
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, MKT_BAM2SAM_BATCH=str(BATCH)))
    assert r.returncode == 3 and r.stdout == b"".join(good["lines"][:written]), r.stderr.decode()[-300:]
    assert "[tag_type]" in r.stderr.decode() and "record %d at %d" % (bad_at, c["bad_offset"]) in r.stderr.decode()
    # -H decodes no record: the header of the same file is printed
    r = subprocess.run([EXE, "-H", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout == bc.TEXT


def test_bgzf_clear_makes_the_reader_as_new():
    a, b = bc.bgzf(bc.case("lengths")["raw"]), bc.bgzf(bc.case("tags")["raw"], block=1000)
    with m.BgzfReader() as fresh:
        fresh.add(b)
        want_info, want = fresh.run(), fresh.text()
    with m.BgzfReader() as r:
        r.add(a)
        r.run()
        assert r.text() == bc.case("lengths")["raw"]
        r.clear()
        assert r.info is None
        with pytest.raises(m.MktError):
            r.text()
        with pytest.raises(m.MktError):
            r.device_text()
        r.add(b)
        assert r.run() == want_info and r.text() == want == bc.case("tags")["raw"]      # nothing of the first file is left
        r.clear()
        assert r.run().blocks == 0 and r.text() == b""
    import px2_inputs
    c = px2_inputs.case("many_pairs")
    with m.PairsGz() as g, m.BgzfReader() as r:
        g.add(c["text"])
        g.run(level=1)
        r.add(g.gz_bytes())
        r.load_index(g.px2_bytes())
        assert r.count() > 0
        r.clear()
        with pytest.raises(m.MktError):
            r.count()                                    # the index is forgotten too
        with pytest.raises(m.MktError):
            r.query(["chr1|chr1"])


def test_bam2sam_usage_and_refusal(tmp_path):
    r = subprocess.run([EXE], stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"Usage" in r.stderr and b"stay written" in r.stderr
    c = bc.case("tag_type")
    path = tmp_path / "bad.bam"
    path.write_bytes(bc.bgzf(c["raw"]))
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 3 and r.stdout == b""
    assert "[tag_type]" in r.stderr.decode() and "record %d at %d" % c["refused"][1:] in r.stderr.decode()
    path.write_bytes(bc.bgzf(bc.case("lengths")["raw"])[:-40])      # a BGZF member cut short: the inflate names it
    r = subprocess.run([EXE, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 3


def test_sam2bam_output_decodes_back_to_its_sorted_lines():
    sam = unz(GOLDEN["sam/edge_aba.sam"]["sam"])
    text, lines = bamdef.split_sam(sam)
    ids = bamdef.ref_ids_of(text)
    for sorted_ in (True, False):
        bam = m.sam_to_bam(sam, sorted=sorted_, level=2)[0]
        want = [bamio.normalise_sam_line(lines[i].decode()).encode() + b"\n" for i in bamdef.file_order(lines, ids, sorted_)]
        assert m.bam_to_sam(bam).split(b"\n")[:-1] == [w[:-1] for w in want]
        assert m.bam_to_sam(bam, header=True, piece=4099).startswith(bamdef.header_text_out(text, sorted_))


@pytest.mark.parametrize("name,mode", [("edge_unc.sam", "unc"), ("edge_flash.sam", "flash")])
def test_bam2sam_into_sam2pairs_equals_sam2pairs_on_the_text(name, mode, tmp_path):
    g = GOLDEN["sam/" + name]
    bam, sam = tmp_path / "x.bam", tmp_path / "x.sam"
    bam.write_bytes(unz(g["bam"]))
    sam.write_bytes(unz(g["view_h"]))
    rc, _, err = m.run_sam2pairs(str(sam), mode, str(tmp_path / "a"), threads=4)
    assert rc == 0, err
    p1 = subprocess.Popen([EXE, "-h", str(bam)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p2 = subprocess.run([m.exe_path(), "/dev/stdin", mode, str(tmp_path / "b"), "4", "0.5", "10", "yes"], stdin=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    p1.stdout.close()
    assert p1.wait(timeout=60) == 0 and p2.returncode == 0, p2.stderr.decode()
    for ext in (".pairs", ".sam", ".log"):
        a, b = tmp_path / ("a" + ext), tmp_path / ("b" + ext)
        assert a.exists() == b.exists()
        if a.exists():
            assert util.canon(a.read_bytes()) == util.canon(b.read_bytes()), ext
