"""Read stitching on the GPU at its word, lane, tie and threshold edges: the families of tests/stitch_edge_cases.py through
microcket_amd.Stitcher and bin/stitch against the definition (tests/stitchdef.py) and the program's hashes
(tests/golden/stitch_edges_golden.json), all four streams and the stat line byte for byte, every pair; the bounds of a quality
byte for two offsets; which bad pair is reported.  What each family reaches is asserted without a GPU in
tests/test_stitch_edges_host.py."""
import numpy as np
import pytest

import microcket_amd as m
import stitch_edge_cases as ec
import stitchdef as sd
from test_gpu_stitch import STREAMS, _kw, _need_gpu, cli, same
from test_stitch_edges_host import check_hashes, golden_case

pytestmark = pytest.mark.gpu
_cache = {}


def gpu(text, pieces=None, segment_pairs=None, **kw):
    """test_gpu_stitch.gpu with the phred offset passed on (kw as stitchdef.stitch takes them)"""
    with m.Stitcher(segment_pairs=segment_pairs, phred_offset=kw.get("phred", 33), **_kw(kw)) as s:
        cuts = [0] + list(pieces or []) + [len(text)]
        for a, b in zip(cuts, cuts[1:]):
            s.push(text[a:b])
        s.finish()
        st = s.stats()
        out = {k: s.stream(i) for i, k in enumerate(STREAMS)}
        out.update(stat=s.stat_line(), total=st.total, combined=st.combined, uncombined=st.uncombined, passed=st.passed, percent=sd.percent(st.combined, st.total))
    return out


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_family_in_one_piece(family):
    _need_gpu()
    for case, text, kw in ec.cases(family):
        got = gpu(text, **kw)
        same(got, ec.definition(family)[case])
        check_hashes(got, golden_case(family, case))


def thinned(family, case, text, kw, n):
    """n pairs of a case spread over it evenly, with the definition's result for them (made once)"""
    key = (family, case, n)
    if key not in _cache:
        total = text.count(b"\n") // 8
        sub = ec.take_pairs(text, sorted({k * total // n for k in range(n)}))
        _cache[key] = (sub, sd.stitch(sub, **kw))
    return _cache[key]


@pytest.mark.parametrize("segment_pairs", (1, 2, 3, 5))
@pytest.mark.parametrize("family", ("length_grid", "quality_ties"))
def test_short_segments(family, segment_pairs):
    """Segments that fill one, two or three of a workgroup's four waves (the idle ones still pass both barriers), and five: a full
    workgroup and a quarter of one.  The pushes are cut at single bytes around one record boundary."""
    _need_gpu()
    per_case = 60 // len(ec.cases(family))
    for case, text, kw in ec.cases(family):
        want = ec.definition(family)[case]
        if segment_pairs == 1:
            text, want = thinned(family, case, text, kw, per_case)
        lines = text.split(b"\n")
        b = len(b"\n".join(lines[:8 * (len(lines) // 16)])) + 1      # where a pair in the middle begins
        assert text[b - 1:b + 1] == b"\n@"
        same(gpu(text, pieces=range(b - 3, b + 4), segment_pairs=segment_pairs, **kw), want)


CLI_CASES = ["p64_m%d_M%d_x%s" % (mM + (x,)) for mM, x in zip(ec.MIN_MAX + ec.MIN_MAX[1:4], ec.DENSITIES)] + ["p33_m1_M1_x0.25", "p33_m10_M255_x0.3333333"]


@pytest.mark.parametrize("case", CLI_CASES)
def test_parameters_through_the_executable(case, tmp_path):
    """-m -M -x -p as bin/stitch takes them, every x and every (m, M) once with -p 64: both modes"""
    _need_gpu()
    _c, text, kw = next(c for c in ec.cases("parameters") if c[0] == case)
    want, g = ec.definition("parameters")[case], golden_case("parameters", case)
    rc, out, err = cli(text, tmp_path, args=ec.flash_args(kw))
    assert rc == 0, err
    same(out, want, ("ext", "cut1", "cut2", "stat"))
    assert (sd.sha(out["ext"]), sd.sha(out["cut1"]), sd.sha(out["cut2"]), out["stat"].decode()) == (g["ext_sha256"], g["cut1_sha256"], g["cut2_sha256"], g["stat"])
    rc, out, err = cli(text, tmp_path, tab=True, args=ec.flash_args(kw))
    assert rc == 0 and out["tab"] == want["tab"], err


def test_the_executable_cases_cover_the_parameters():
    kws = [next(kw for c, _t, kw in ec.cases("parameters") if c == case) for case in CLI_CASES]
    assert {kw["x"] for kw in kws if kw["phred"] == 64} == set(ec.DENSITIES) and {(kw["m"], kw["M"]) for kw in kws if kw["phred"] == 64} == set(ec.MIN_MAX)


def _bounds_pair(name, q1, q2):
    """reads of 200 bases that overlap in 150"""
    f = ec.rnd_seq(np.random.RandomState(4701), 250)
    return ec.record(name + b"/1", f[:200], q1, ec.rc(f[50:]), q2, name + b"/2")


@pytest.mark.parametrize("phred", (33, 64))
def test_quality_bounds(phred):
    """phred_offset and phred_offset + 93 are the accepted ends (for offset 64 that is byte 157, which the program itself cannot
    take: the definition alone is the reference here); one outside either, at the first position, the last and position 64, in read 1
    or in read 2, is refused with the pair's number."""
    _need_gpu()
    lo, hi = bytes([phred]) * 200, bytes([phred + 93]) * 200
    good = _bounds_pair(b"lo", lo, lo) + _bounds_pair(b"hi", hi, hi) + _bounds_pair(b"lohi", lo, hi) + _bounds_pair(b"hilo", hi, lo)
    want = sd.stitch(good, phred=phred)
    assert want["combined"] == 4
    same(gpu(good, phred=phred), want)
    mid = bytes([phred + 30]) * 200
    for c in (phred - 1, phred + 94):
        for pos in (0, 64, 199):
            for read in (1, 2):
                q = mid[:pos] + bytes([c]) + mid[pos + 1:]
                bad = _bounds_pair(b"bad", q if read == 1 else mid, q if read == 2 else mid)
                with pytest.raises(ValueError):
                    sd.stitch(bad, phred=phred)
                with pytest.raises(m.MktError, match="read pair 3 .*quality byte"):
                    gpu(good[:good.index(b"@hilo/1\n")] + bad + good, phred=phred)


def test_the_first_bad_pair_is_reported():
    """Refusals of the arguments, in segments of 8 pairs: a bad pair in the third segment; two in one segment (the smaller number
    wins whichever wave is first); an empty read behind a quality byte."""
    _need_gpu()
    text = sd.synth(31, 24, 60)
    lines = text.split(b"\n")

    def with_bad(bad):
        ls = list(lines)
        for k, what in bad.items():
            if what == "quality":
                ls[8 * k + 7] = b" " + ls[8 * k + 7][1:]
            else:
                ls[8 * k + 1] = ls[8 * k + 3] = b""
        return b"\n".join(ls)

    same(gpu(text, segment_pairs=8), sd.stitch(text))
    for bad, msg in (({19: "quality"}, "read pair 19 .*quality byte"), ({14: "quality", 9: "quality"}, "read pair 9 .*quality byte"),
                     ({9: "empty", 14: "quality"}, "read pair 9 .*empty read"), ({12: "empty", 10: "quality"}, "read pair 10 .*quality byte")):
        with pytest.raises(m.MktError, match=msg):
            gpu(with_bad(bad), segment_pairs=8)
