"""The shared half of the GPU BGZF reader (microcket_amd/csrc/mkt_inflate.h: the block table, the dynamic header, the Kraft checks, the
table build, the decode of one token with its refusals) through its stand-alone driver tests/host/inflate_host.cpp, plain and under
ASan/UBSan, without a GPU: over every directed case of tests/inflate_cases.py and the files the reference's bgzip wrote
(tests/golden/inflate_golden.json) the text equals zlib's byte for byte, and a refusal names the case's reason and the block's offset.
The kernel executes the same functions."""
import base64
import hashlib
import json
import os
import subprocess

import pytest

import inflate_cases
import inflatedef
import px2_inputs
import px2def

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "tests", "host", "_build", "inflate_host")          # made by build() (microcket_amd/build.py build_test_tools)
with open(os.path.join(HERE, "golden", "inflate_golden.json")) as f:
    GOLDEN = json.load(f)


def deflate_kinds(gz):
    """deflate blocks by type over all members, as inflatedef sees them"""
    kinds = [0, 0, 0]
    for c, b, _, _ in px2def.bgzf_blocks(gz, check=False):
        for blk in inflatedef.inflate(gz[c + 18:c + b - 8])[0]:
            kinds[blk.btype] += 1
    return kinds


def run_driver(exe, gz, tmp_path):
    src, dst = tmp_path / "in.gz", tmp_path / "out.txt"
    src.write_bytes(gz)
    if dst.exists():
        dst.unlink()
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    words = r.stdout.decode().split()
    return words, (dst.read_bytes() if dst.exists() else None)


def test_golden_is_what_the_maker_writes():
    assert sorted(GOLDEN) == sorted("%s/l%d" % (n, l) for n in ("blocks_many_bins", "many_pairs") for l in (1, 6, 9))
    assert os.path.getsize(os.path.join(HERE, "golden", "inflate_golden.json")) < (1 << 20)
    for g in GOLDEN.values():
        text = px2_inputs.case(g["case"])["text"]
        assert hashlib.sha256(text).hexdigest() == g["text_sha256"]
        assert px2def.bgzf_inflate(base64.b64decode(g["gz_base64"])) == text


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_driver_accepts_and_inflates(sanitize, tmp_path):
    exe = HOST + "_san" if sanitize else HOST
    files = [(c["name"], c["gz"], c["text"]) for c in inflate_cases.accepted()]
    files += [(k, base64.b64decode(g["gz_base64"]), px2_inputs.case(g["case"])["text"]) for k, g in sorted(GOLDEN.items())]
    for name, gz, text in files:
        words, out = run_driver(exe, gz, tmp_path)
        assert out == text == px2def.bgzf_inflate(gz), name
        blocks = px2def.bgzf_blocks(gz)
        assert words == ["ok", str(len(blocks)), str(len(text))] + [str(k) for k in deflate_kinds(gz)] + ["1" if gz[-28:] == px2def.BGZF_EOF else "0"], name


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_driver_refuses_with_reason_and_offset(sanitize, tmp_path):
    exe = HOST + "_san" if sanitize else HOST
    for c in inflate_cases.refused():
        words, out = run_driver(exe, c["gz"], tmp_path)
        assert words == ["refused", c["refused"], str(inflate_cases.refused_offset(c))], c["name"]
        assert out is None
