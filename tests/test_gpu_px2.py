"""final.pairs.gz and its pairix index on the GPU (mkt_pairsgz_* of include/mkt.h, microcket_amd.PairsGz, bin/pairsbgz).

For every case of px2_inputs.py: the .gz inflates block by block to the text with every CRC-32 and ISIZE right and ends with the EOF
block; the .px2 parses with no byte unaccounted for, equals the reference's own index of the same text under the comparison by text
offsets (tests/golden/px2_golden.json), and equals px2def's builder on this .gz's block table byte for byte; px2def's region lookup
over the two files returns the lines pairix printed.  The bytes do not depend on how the text was fed, on the call or on the process.
Refused texts name the line and leave nothing behind."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import microcket_amd as m
import px2_inputs
import px2def

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairsbgz")
with open(os.path.join(HERE, "golden", "px2_golden.json")) as f:
    GOLDEN = json.load(f)
ACCEPTED = [c["name"] for c in px2_inputs.accepted()]
REFUSED = [c["name"] for c in px2_inputs.refused()]
CLI_CASES = ["blocks_long_runs", "blocks_many_bins", "many_pairs"]
_cache = {}


def gpu_files(name, level=1, piece=None):
    """(gz, px2, info) of a case, made once per (case, level) when fed in one piece"""
    key = (name, level)
    if piece is None and key in _cache:
        return _cache[key]
    text = px2_inputs.case(name)["text"]
    with m.PairsGz() as g:
        if piece is None:
            g.add(text)
        else:
            for k in range(0, len(text), piece):
                g.add(text[k:k + piece])
        info = g.run(level=level)
        out = (g.gz_bytes(), g.px2_bytes(), info)
    if piece is None:
        _cache[key] = out
    return out


def check_files(name, gz, px2, level_note=""):
    case = px2_inputs.case(name)
    text = case["text"]
    blocks = px2def.bgzf_blocks(gz)                         # inflates every block; CRC-32 and ISIZE compared
    assert px2def.bgzf_inflate(gz) == text, level_note
    assert gz[-28:] == px2def.BGZF_EOF and blocks[-1][3] == 0
    assert [b[3] for b in blocks[:-1]] == [min(px2def.BGZF_RAW, len(text) - k) for k in range(0, len(text), px2def.BGZF_RAW)]
    ix = px2def.parse_px2(px2)                               # every byte accounted for; BGZF with its EOF block
    assert px2def.to_text_offsets(ix, blocks, len(gz)) == GOLDEN[name]["index"], level_note
    assert px2def.bgzf_inflate(px2) == px2def.serialize(px2def.build_index(text, blocks, len(gz))), level_note
    return ix


@pytest.mark.parametrize("name", ACCEPTED)
def test_files_equal_definition_and_reference(name):
    gz, px2, info = gpu_files(name)
    ix = check_files(name, gz, px2)
    text = px2_inputs.case(name)["text"]
    assert px2def.count_lines(px2) == GOLDEN[name]["n"] == info.lines
    recs = [ln for ln in text.split(b"\n") if ln and ln[:1] != b"#"]
    assert info.records == len(recs) and info.names == len(ix["names"])
    assert info.bins == info.chunks == sum(len(b) for b in ix["bins"])
    assert info.gz_bytes == len(gz) and info.px2_bytes == len(px2) and info.blocks == len(px2def.bgzf_blocks(gz, check=False)) - 1
    for region, lines in GOLDEN[name]["queries"].items():
        assert px2def.query(gz, px2, region) == lines, region


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("name", ["many_pairs", "bin_edges", "blocks_many_bins", "no_final_newline", "header_only"])
def test_other_levels(name, level):
    gz, px2, _ = gpu_files(name, level)
    check_files(name, gz, px2, "level %d" % level)


@pytest.mark.parametrize("name", ACCEPTED)
def test_pieces_give_the_same_bytes(name):
    gz, px2, _ = gpu_files(name)
    pieces = [4097] + ([1] if len(px2_inputs.case(name)["text"]) < 4096 else [])
    for piece in pieces:
        g2, x2, _ = gpu_files(name, piece=piece)
        assert g2 == gz and x2 == px2, piece


def _digests():
    out = {}
    for name in CLI_CASES + ["bin_edges"]:
        for level in (0, 1, 2):
            gz, px2, _ = gpu_files(name, level, piece=1 << 20)         # piece: not from the cache
            out["%s/%d" % (name, level)] = hashlib.sha256(gz).hexdigest() + hashlib.sha256(px2).hexdigest()
    return out


def test_same_bytes_on_every_call_and_in_a_fresh_process():
    first = _digests()
    assert _digests() == first
    for key, d in first.items():
        name, level = key.split("/")
        gz, px2, _ = gpu_files(name, int(level))
        assert hashlib.sha256(gz).hexdigest() + hashlib.sha256(px2).hexdigest() == d
    code = "import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_px2 as t; print(json.dumps(t._digests()))" % (os.path.dirname(HERE), HERE)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert json.loads(r.stdout.decode().strip().split("\n")[-1]) == first


@pytest.mark.parametrize("name", REFUSED)
def test_refused_texts_name_the_line(name, tmp_path):
    case = px2_inputs.case(name)
    with m.PairsGz() as g:
        g.add(case["text"])
        with pytest.raises(m.MktError) as e:
            g.run()
        assert "line %d:" % case["refused"] in str(e.value)
        assert g.info is None
        for fetch in (g.gz_bytes, g.px2_bytes):
            with pytest.raises(m.MktError):
                fetch()
        with pytest.raises(m.MktError):
            g.write(str(tmp_path / "never.pairs.gz"))
    # the tool: exit status, the line in its message, no file
    src, dst = tmp_path / "in.pairs", tmp_path / "out.pairs.gz"
    src.write_bytes(case["text"])
    r = subprocess.run([EXE, str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 21 and ("line %d:" % case["refused"]) in r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["in.pairs"]


def test_refused_line_is_the_smallest(tmp_path):
    """Several faults in one text, in different workgroups of the per-line kernel: the first line wins, whatever its kind."""
    good = [px2_inputs.rec(i, "chr1", 10 + i, "chr1", 5) for i in range(1000)]
    reappears = good[:400] + [px2_inputs.rec(0, "chr2", 1, "chr2", 5)] + good[400:]            # chr1|chr1 comes back at line 402
    for text, line in ((b"".join(reappears + [b"bad\n"]), 402), (b"".join(good[:300] + [b"bad\n"] + reappears[300:]), 301),
                       (b"".join(good[:700] + [good[3]] + good[700:] + [b"bad\n"]), 701)):
        with m.PairsGz() as g:
            g.add(text)
            with pytest.raises(m.MktError) as e:
                g.run()
            assert "line %d:" % line in str(e.value)


def test_run_again_after_more_text():
    a = px2_inputs.case("one_record")["text"]
    b = px2_inputs.rec(9, "chr1", 70000, "chr2", 5)
    with m.PairsGz() as g:
        g.add(a)
        g.run()
        first = g.gz_bytes()
        g.add(b)
        with pytest.raises(m.MktError):
            g.gz_bytes()                                     # stale: the text has grown
        g.run(level=2)
        gz, px2 = g.gz_bytes(), g.px2_bytes()
    assert px2def.bgzf_inflate(first) == a and px2def.bgzf_inflate(gz) == a + b
    blocks = px2def.bgzf_blocks(gz)
    assert px2def.bgzf_inflate(px2) == px2def.serialize(px2def.build_index(a + b, blocks, len(gz)))


def test_bad_options():
    with m.PairsGz() as g:
        g.add(px2_inputs.case("one_record")["text"])
        for level in (-1, 3):
            with pytest.raises(m.MktError):
                g.run(level=level)


@pytest.mark.parametrize("name", CLI_CASES)
def test_tool_writes_the_same_files(name, tmp_path):
    gz, px2, _ = gpu_files(name, 2)
    src, dst = tmp_path / "final.pairs", tmp_path / "final.pairs.gz"
    src.write_bytes(px2_inputs.case(name)["text"])
    r = subprocess.run([EXE, "-l", "2", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    assert dst.read_bytes() == gz and (tmp_path / "final.pairs.gz.px2").read_bytes() == px2
    check_files(name, dst.read_bytes(), (tmp_path / "final.pairs.gz.px2").read_bytes())
    # an index that exists is kept unless -f is given; stdin works
    r = subprocess.run([EXE, "-l", "1", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 4 and dst.read_bytes() == gz
    with open(src, "rb") as f:
        r = subprocess.run([EXE, "-f", "-l", "1", "-", str(dst)], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    g1, x1, _ = gpu_files(name, 1)
    assert dst.read_bytes() == g1 and (tmp_path / "final.pairs.gz.px2").read_bytes() == x1


def test_tool_refuses_gz_input(tmp_path):
    r = subprocess.run([EXE, str(tmp_path / "x.pairs.gz"), str(tmp_path / "y.pairs.gz")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 3 and os.listdir(tmp_path) == []
