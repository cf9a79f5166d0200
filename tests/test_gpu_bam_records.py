"""sam2bam's records, exactly (DESIGN.md "The records, exactly"): for every case list of tests/bam_record_cases.py, in input order and
sorted, the inflated blocks of mkt_bam_* joined are byte for byte the stream tests/bamdef.py encodes from the same text -- header,
every fixed field, name, CIGAR, SEQ nibbles, QUAL, every tag -- and a difference is reported as record and field.  The writer is
bam_record<WRITE> and its Sink in mkt_bam.hip (k_merge_gather on the out-of-core path).  The one tolerance: floats of domain B (more
than 9 digits or a power of ten beyond 10^+-22 that is no %.9g print of a float) may be one ulp off float32_exact; domains A and C are
compared like every other byte.  The conditions the inputs must meet (all 64 Sink alignment classes, colliding reference names, the
float domains) are asserted on the CPU in tests/test_bamdef_host.py."""
import functools
import struct

import pytest

import bam_record_cases as cases
import bamdef
import bamio

pytestmark = pytest.mark.gpu

CASES = cases.all_cases()


@functools.lru_cache(maxsize=None)
def _want(k, sorted_):
    return bamdef.stream_bytes(CASES[k].header, CASES[k].lines, sorted_)


def _inflated(bam_bytes):
    assert bam_bytes.endswith(bamio.EOF_BLOCK)
    return b"".join(raw for _, _, raw in bamio.bgzf_blocks(bam_bytes))


def _compare(k, sorted_, got):
    c = CASES[k]
    if not c.masked:
        if got != _want(k, sorted_):
            msg = bamdef.explain(got, c.header, c.lines, sorted_)
            raise AssertionError(f"{c.name}, sorted={sorted_}: {msg}")
        return
    # domain B: every byte but the float words, then the words against the one-ulp bound
    ranges = cases.float_word_ranges(c, sorted_)
    msg = bamdef.explain(got, c.header, c.lines, sorted_, ignore=[(a, b) for a, b, _ in ranges])
    assert msg == "", f"{c.name}, sorted={sorted_}: {msg}"
    off = []
    for a, b, text in ranges:
        bits = struct.unpack("<I", got[a:b])[0]
        exact = bamdef.float32_exact(text)
        d = bamdef.ulps_between(bits, exact)
        print(f"domain B {text!r}: got 0x{bits:08x}, exact 0x{exact:08x}, {d} ulp")
        if d > 1 or bamdef.f32_class(bits) != bamdef.f32_class(exact):
            off.append((text, hex(bits), hex(exact)))
    assert not off, off


@pytest.mark.parametrize("sorted_", [False, True], ids=["input order", "sorted"])
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_stream_is_the_definition(k, sorted_):
    import microcket_amd as m
    c = CASES[k]
    bam_b, bai_b, n = m.sam_to_bam(cases.sam_text(c), sorted=sorted_, level=0)
    assert n == len(c.lines)
    _compare(k, sorted_, _inflated(bam_b))


def test_sink_case_through_deflate_and_the_out_of_core_path(tmp_path):
    """levels 1 and 2 must inflate to the level-0 stream; with a run budget (>= 3 runs, sized as tests/test_gpu_bam_spill.py does) the
    records pass through k_merge_gather, which copies them with its own accesses: the same bytes"""
    import microcket_amd as m
    k = [c.name for c in CASES].index("sink")
    text = cases.sam_text(CASES[k])
    for sorted_ in (False, True):
        for level in (1, 2):
            _compare(k, sorted_, _inflated(m.sam_to_bam(text, sorted=sorted_, level=level)[0]))
    body = len(text) - len(CASES[k].header)
    for level in (0, 2):
        st = {}
        bam_b, bai_b, n = m.sam_to_bam(text, sorted=True, level=level, run_bytes=body // 4, tmp=tmp_path / "s", stats=st, piece=4096)
        assert st["runs"] >= 3 and st["tmp_bytes"] > 0 and n == len(CASES[k].lines), st
        _compare(k, True, _inflated(bam_b))
        assert (bam_b, bai_b) == m.sam_to_bam(text, sorted=True, level=level)[:2]


def test_rejected_shapes_raise():
    """one bad line after a good one, as test_errors_are_reported does; the accepted neighbours of every limit are in the `fields` and
    `tags` case lists above"""
    import microcket_amd as m
    good = cases.line(b"good")
    for header in {h for _, h, _ in cases.REJECTS}:
        assert m.sam_to_bam(header + good + b"\n")[2] == 1
    for what, header, bad in cases.REJECTS:
        with pytest.raises(m.MktError):
            m.sam_to_bam(header + good + b"\n" + bad + b"\n")
            pytest.fail(f"accepted: {what}")
        with pytest.raises(m.MktError):
            m.sam_to_bam(header + bad + b"\n", sorted=False)
            pytest.fail(f"accepted alone, input order: {what}")


@pytest.mark.parametrize("nref", cases.REF_SIZES)
def test_absent_reference_names_are_rejected(nref):
    """names that are not in the header but hit an occupied probe chain of the name table, are a prefix of a present name or extend
    one: as RNAME and as RNEXT (every present name is looked up both ways by test_stream_is_the_definition)"""
    import microcket_amd as m
    header, lines, names, absent = cases.ref_case(nref)
    assert m.sam_to_bam(header + lines[0] + b"\n")[2] == 1
    for kind, name in absent.items():
        for bad in (cases.line(b"bad", rname=name), cases.line(b"bad", rname=names[0], rnext=name)):
            with pytest.raises(m.MktError):
                m.sam_to_bam(header + lines[0] + b"\n" + bad + b"\n")
                pytest.fail(f"accepted: {kind}: {name!r}")
