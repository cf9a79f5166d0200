"""Read stitching on the GPU: mkt_stitch_* (through microcket_amd.Stitcher) and bin/stitch against the definition (tests/stitchdef.py)
and the golden vectors made by FLASH v1.2.11 + deal.flash.pl (tests/golden/stitch_golden.json), byte for byte, by every route."""
import os
import subprocess
import sys

import pytest

import microcket_amd as m
import stitchdef as sd
from test_stitch import case_input, case_kw, edge_set, golden

pytestmark = pytest.mark.gpu
STREAMS = ("tab", "ext", "cut1", "cut2")
EXE = os.path.join(os.path.dirname(m.exe_path()), "stitch")


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")


def _kw(kw):
    return dict(min_overlap=kw.get("m", 10), max_overlap=kw.get("M", 150), max_mismatch_density=kw.get("x", 0.25), cut_tail=kw.get("cut_tail", 10),
                min_size=kw.get("min_size", 36))


def gpu(text, pieces=None, segment_pairs=None, **kw):
    """-> dict like stitchdef.stitch's.  pieces: the cut points of the pushes (default: one piece)"""
    with m.Stitcher(segment_pairs=segment_pairs, **_kw(kw)) as s:
        cuts = [0] + list(pieces or []) + [len(text)]
        for a, b in zip(cuts, cuts[1:]):
            s.push(text[a:b])
        s.finish()
        st = s.stats()
        out = {k: s.stream(i) for i, k in enumerate(STREAMS)}
        out.update(stat=s.stat_line(), total=st.total, combined=st.combined, uncombined=st.uncombined, passed=st.passed, percent=sd.percent(st.combined, st.total))
    return out


def cli(text, tmp_path, tab=False, args=(), env=None):
    """bin/stitch on a pipe -> (rc, dict, stderr)"""
    pre = str(tmp_path / "o")
    p = subprocess.run([EXE, *args, *(("--tab",) if tab else ("-o", pre)), "-"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, **(env or {})))
    out = {}
    if p.returncode == 0:
        if tab:
            out["tab"] = p.stdout
        else:
            for k, e in (("ext", ".ext.fq"), ("cut1", ".cut.read1.fq"), ("cut2", ".cut.read2.fq"), ("stat", ".stitch.stat")):
                out[k] = open(pre + e, "rb").read()
    return p.returncode, out, p.stderr


def same(got, want, keys=STREAMS + ("stat",)):
    for k in keys:
        assert got[k] == want[k], k


def test_edge_set_matches_the_programs_lines(tmp_path):
    _need_gpu()
    text, want = edge_set()
    same(gpu(text), want)
    rc, out, err = cli(text, tmp_path)
    assert rc == 0, err
    same(out, want, ("ext", "cut1", "cut2", "stat"))
    rc, out, err = cli(text, tmp_path, tab=True)
    assert rc == 0 and out["tab"] == want["tab"], err


def test_mixed_case_by_every_route(tmp_path):
    """about 3 000 mixed pairs: one piece; single bytes across a record boundary; 256-pair segments (several and a partial last one);
    the default segment; twice; bin/stitch in both modes -- all the same bytes, equal to the definition and the golden hashes"""
    _need_gpu()
    c = next(c for c in golden()["cases"] if c["name"] == "mixed")
    text, want = case_input(c)
    one = gpu(text)
    same(one, want)
    comb, unc = sd.by_kind(one["tab"])
    assert (sd.sha(comb), sd.sha(unc)) == (c["tab_combined_sha256"], c["tab_uncombined_sha256"])
    assert (sd.sha(one["ext"]), sd.sha(one["cut1"]), sd.sha(one["cut2"])) == (c["ext_sha256"], c["cut1_sha256"], c["cut2_sha256"])
    assert one["stat"].decode() == c["stat"] and one["percent"] == c["percent"]
    assert one["total"] == c["pairs"] == one["combined"] + one["uncombined"]
    # single bytes across the boundary between two records (and so between two pairs), the rest in two pieces
    b = text.index(b"\n@p1501/1\n") + 1
    cuts = list(range(b - 3, b + 4))
    same(gpu(text, pieces=cuts), one)
    same(gpu(text, pieces=cuts, segment_pairs=256), one)
    same(gpu(text, pieces=list(range(100003, len(text), 100003)), segment_pairs=256), one)
    assert c["pairs"] % 256 and c["pairs"] > 4 * 256
    same(gpu(text), one)                                          # two calls
    rc, out, err = cli(text, tmp_path, env={"MKT_STITCH_SEGMENT_PAIRS": "256"})
    assert rc == 0, err
    same(out, one, ("ext", "cut1", "cut2", "stat"))
    assert ("Percent combined: %s%%" % c["percent"]).encode() in err
    rc, out, err = cli(text, tmp_path, tab=True)
    assert rc == 0 and out["tab"] == one["tab"], err
    assert ("Percent combined: %s%%" % c["percent"]).encode() in err


def test_other_arguments(tmp_path):
    _need_gpu()
    c = next(c for c in golden()["cases"] if c["name"] == "other_args")
    text, want = case_input(c)
    kw = case_kw(c)
    got = gpu(text, **kw)
    same(got, want)
    assert (sd.sha(got["ext"]), sd.sha(got["cut1"]), sd.sha(got["cut2"]), got["stat"].decode()) == (c["ext_sha256"], c["cut1_sha256"], c["cut2_sha256"], c["stat"])
    rc, out, err = cli(text, tmp_path, args=("-m", str(kw["m"]), "-M", str(kw["M"]), "-x", str(kw["x"]), "--cut-tail", str(kw["cut_tail"]), "--min-size", str(kw["min_size"])))
    assert rc == 0, err
    same(out, want, ("ext", "cut1", "cut2", "stat"))


def test_more_than_2_16_pairs_of_60_bases():
    _need_gpu()
    c = next(c for c in golden()["cases"] if c["name"] == "len60_over_2_16")
    assert c["pairs"] > 1 << 16
    text, want = case_input(c)
    got = gpu(text, segment_pairs=1 << 15)
    same(got, want)
    assert (sd.sha(got["ext"]), sd.sha(got["cut1"]), sd.sha(got["cut2"]), got["stat"].decode(), got["percent"]) == (
        c["ext_sha256"], c["cut1_sha256"], c["cut2_sha256"], c["stat"], c["percent"])


def test_zero_pairs_one_pair_and_a_missing_last_newline(tmp_path):
    _need_gpu()
    empty = gpu(b"")
    assert all(empty[k] == b"" for k in STREAMS) and empty["stat"] == b"Combined\t0\tUncombined\t0\tPass\t0\n" and empty["total"] == 0
    rc, out, err = cli(b"", tmp_path)
    assert rc == 0 and out["stat"] == empty["stat"] and out["ext"] == b"" and b"Percent combined: 0.00%" in err
    text = sd.synth(21, 40)
    first = text[:text.index(b"@p1/1\n")]
    same(gpu(first), sd.stitch(first))
    assert gpu(first)["total"] == 1
    want = sd.stitch(text)
    same(gpu(text[:-1]), want)
    same(gpu(text[:-1], pieces=[len(text) - 2], segment_pairs=7), want)


def test_bad_inputs_are_clean_errors(tmp_path):
    _need_gpu()
    text = sd.synth(22, 30)
    lines = text.split(b"\n")
    odd = b"\n".join(lines[:8 * 20 + 4]) + b"\n"                  # an odd number of records
    with pytest.raises(m.MktError, match="not whole read pairs"):
        gpu(odd)
    rc, out, err = cli(odd, tmp_path)
    assert rc == 21 and b"not whole read pairs" in err
    rec = lambda n1, q=b"I": b"@a/1\n%s\n+\n%s\n@a/2\n%s\n+\n%s\n" % (b"A" * n1, q * n1, b"C" * 30, b"I" * 30)
    assert gpu(rec(sd.MAX_READ))["total"] == 1
    for bad, what in ((rec(sd.MAX_READ + 1), "longer than"), (rec(0), "empty read"), (rec(30, b" "), "quality byte"),
                      (rec(30).replace(b"I" * 30 + b"\n@a/2", b"I" * 29 + b"\n@a/2"), "differ in length")):
        with pytest.raises(m.MktError, match="read pair 3.*" + what):
            gpu(text[:text.index(b"@p3/1\n")] + bad + text)
    with pytest.raises(m.MktError, match="max overlap"):
        m.Stitcher(max_overlap=sd.MAX_M + 1)


def test_two_processes_give_the_same_bytes():
    _need_gpu()
    c = next(c for c in golden()["cases"] if c["name"] == "len100")
    text, want = case_input(c)
    same(gpu(text, segment_pairs=500), want)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import stitchdef as sd, microcket_amd as m\n"
            "text = sd.synth(%d, %d, %d)\n"
            "with m.Stitcher() as s:\n"
            "    s.push(text); s.finish()\n"
            "    print(' '.join(sd.sha(s.stream(k)) for k in range(4)), s.stat_line().decode().strip())\n") % (
                os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__))), c["seed"], c["pairs"], c["read_len"])
    outs = [subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120) for _ in range(2)]
    assert all(p.returncode == 0 for p in outs), outs[0].stderr
    expect = " ".join(sd.sha(want[k]) for k in STREAMS) + " " + want["stat"].decode().strip()
    assert outs[0].stdout.decode().strip() == outs[1].stdout.decode().strip() == expect
