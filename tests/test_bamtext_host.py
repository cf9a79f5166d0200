"""BAM records to SAM text without a GPU: the definition (tests/bamtextdef.py) against what the reference's samtools printed
(tests/golden/bamtext_golden.json), against the independent encoder tests/bamdef.py, and the shared half of the GPU decoder
(microcket_amd/csrc/mkt_bamtext.h: header walk, plausibility test, chain walk, resolve step, validation, length and emit routines)
through its stand-alone driver tests/host/bamtext_host.cpp, plain and under ASan/UBSan, over every directed case of
tests/bamtext_cases.py.  The kernels execute the same functions."""
import hashlib
import os
import subprocess

import pytest

import bamdef
import bamtext_cases as bc
import bamtextdef as bd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "tests", "host", "_build", "bamtext_host")          # made by build() (microcket_amd/build.py build_test_tools)
GOLDEN = bc.golden()
SAMS = ("edge_aba.sam", "edge_flash.sam", "edge_unc.sam")
unz, golden_raw = bc.unz, bc.golden_raw


def test_golden_is_what_the_maker_writes():
    assert sorted(GOLDEN) == sorted(["sam/" + s for s in SAMS] + ["case/" + c["name"] for c in bc.accepted()])
    assert os.path.getsize(os.path.join(HERE, "golden", "bamtext_golden.json")) < 100000
    for c in bc.accepted():
        assert hashlib.sha256(c["raw"]).hexdigest() == GOLDEN["case/" + c["name"]]["raw_sha256"], c["name"]
    for s in SAMS:
        body = b"".join(ln + b"\n" for ln in open(os.path.join(HERE, "golden", s), "rb").read().split(b"\n") if ln and not ln.startswith(b"@"))
        assert unz(GOLDEN["sam/" + s]["sam"]).endswith(body)


@pytest.mark.parametrize("key", sorted(GOLDEN))
def test_definition_reproduces_samtools(key):
    raw = golden_raw(key)
    for mode, k in (("", "view"), ("h", "view_h"), ("H", "view_H")):
        assert bd.view(raw, mode) == unz(GOLDEN[key][k]), (key, k)


@pytest.mark.parametrize("name", SAMS)
def test_bamdef_encoded_sams_decode_back_to_their_lines(name):
    sam = unz(GOLDEN["sam/" + name]["sam"])
    text, lines = bamdef.split_sam(sam)
    raw = bamdef.stream_bytes(text, lines, False)
    h, refs, got = bd.decode(raw)
    assert got == [ln + b"\n" for ln in lines] and h == text
    assert refs == [(n, l) for n, l in bamdef.references(text)]


def test_definition_refuses_every_malformed_case():
    for c in bc.refused():
        with pytest.raises(bd.Refused) as e:
            bd.decode(c["raw"], **{k: v for k, v in c.get("opts", {}).items() if k == "max_record"})
        assert (e.value.reason, e.value.record, e.value.offset) == c["refused"], c["name"]


def run_driver(exe, raw, tmp_path, *args):
    src, dst = tmp_path / "in.raw", tmp_path / "out.sam"
    src.write_bytes(raw)
    for p in (dst, tmp_path / "out.sam.hdr"):
        if p.exists():
            p.unlink()
    r = subprocess.run([exe, str(src), str(dst)] + [str(a) for a in args], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().split(), (dst.read_bytes() if dst.exists() else None), ((tmp_path / "out.sam.hdr").read_bytes() if dst.exists() else None)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_driver_decodes_every_case_at_both_segment_sizes(sanitize, tmp_path):
    exe = HOST + "_san" if sanitize else HOST
    for key in sorted(GOLDEN):
        raw = golden_raw(key)
        want, hdr = unz(GOLDEN[key]["view"]), unz(GOLDEN[key]["view_H"])
        for seg in (bc.SEGMENT, 256 << 10):
            words, out, h = run_driver(exe, raw, tmp_path, seg)
            assert words[0] == "ok" and out == want == bd.view(raw) and h == hdr, (key, seg, words)
            n_rec, n_text, n_seg, repairs = (int(w) for w in words[1:5])
            start = bd.header(raw)[2]
            assert (n_rec, n_text, n_seg) == (want.count(b"\n"), len(want), -(-(len(raw) - start) // seg)), (key, seg)
            if key.startswith("case/seg_decoy") and seg == bc.SEGMENT:
                assert repairs > 0, key                  # the guess took the decoy; the text does not show it
            if seg > len(raw):
                assert repairs == 0, key


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_driver_refuses_with_reason_ordinal_and_offset(sanitize, tmp_path):
    exe = HOST + "_san" if sanitize else HOST
    for c in bc.refused():
        for seg in (bc.SEGMENT, 256 << 10):
            words, out, _ = run_driver(exe, c["raw"], tmp_path, seg, c.get("opts", {}).get("max_record", bd.MAX_RECORD))
            assert words == ["refused", c["refused"][0], str(c["refused"][1]), str(c["refused"][2])], (c["name"], seg)
            assert out is None
