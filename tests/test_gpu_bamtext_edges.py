"""The GPU BAM-to-SAM decoder at its edges: the directed families of tests/bamtext_cases.py (lengths, numbers, tags, segments at
segment_bytes = 256, pieces, refused), each against tests/bamtextdef.py and, where samtools' answer is recorded, against
tests/golden/bamtext_golden.json."""
import struct

import pytest

import bamtext_cases as bc
import bamtextdef as bd
import microcket_amd as m

GOLDEN, unz = bc.golden(), bc.unz

pytestmark = pytest.mark.gpu

ACCEPTED = [c["name"] for c in bc.accepted()]


def decode(raw, cuts=(), **opts):
    """the texts of the runs joined, the header, the infos: the stream fed in the pieces the cuts make"""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(raw))) + [len(raw)]
    texts, infos = [], []
    with m.BamReader() as r:
        for a, b in zip(edges, edges[1:]):
            r.add(raw[a:b])
            infos.append(r.run(**opts))
            texts.append(r.text())
        r.finish()
        return b"".join(texts), r.header(), infos


@pytest.mark.parametrize("name", ACCEPTED)
def test_family_at_small_and_default_segments(name):
    c = bc.case(name)
    want, hdr = bd.view(c["raw"]), bd.view(c["raw"], "H")
    assert want == unz(GOLDEN["case/" + name]["view"]) and hdr == unz(GOLDEN["case/" + name]["view_H"])
    start = bd.header(c["raw"])[2]
    for seg in (bc.SEGMENT, 0):
        text, h, (info,) = decode(c["raw"], segment_bytes=seg)
        assert text == want and h == hdr, (name, seg)
        assert info.records == want.count(b"\n") and info.text_bytes == len(want)
        assert info.segments == -(-(len(c["raw"]) - start) // (seg or 256 << 10))
        if seg == bc.SEGMENT and c.get("repairs"):
            assert info.repairs > 0                      # the guess took the decoy; the text does not show it
        if seg == 0:
            assert info.repairs == 0
    assert decode(c["raw"])[2][0].float_records == (3 if name == "floats" else 0)      # floats, Bf1, Bf300: an empty B:f array holds none


@pytest.mark.parametrize("name", ACCEPTED)
def test_pieces_give_the_text_of_the_whole(name):
    raw = bc.case(name)["raw"]
    want = bd.view(raw)
    start = bd.header(raw)[2]
    inner = [3, 4, 7, 8, 8 + len(bc.TEXT) - 1, start - 5, start - 1, start, start + 1, start + 3, start + 4, start + 35, start + 36, start + 37]
    cuts = list(range(997, len(raw), 997)) + inner
    for seg in (bc.SEGMENT, 0):
        text, h, infos = decode(raw, cuts, segment_bytes=seg)
        assert text == want and h == bd.view(raw, "H"), (name, seg)
        assert sum(i.records for i in infos) == want.count(b"\n") and infos[-1].carry_bytes == 0
    # without its end: every complete record is decoded, finish names the partial one
    if want:
        with m.BamReader() as r:
            r.add(raw[:-1])
            info = r.run(segment_bytes=bc.SEGMENT)
            assert r.text() == b"".join(bd.decode(raw)[2][:-1]) and info.carry_bytes > 0
            with pytest.raises(m.BamRefused) as e:
                r.finish()
            assert (e.value.reason, e.value.record, e.value.offset) == ("truncated", want.count(b"\n") - 1, _last_record_offset(raw, start))


def _last_record_offset(raw, start):
    p = last = start
    while p < len(raw):
        last = p
        p += 4 + struct.unpack_from("<I", raw, p)[0]
    return last


@pytest.mark.parametrize("name", [c["name"] for c in bc.refused()])
def test_refused_with_reason_ordinal_and_offset(name):
    c = bc.case(name)
    good = bc.case("numbers")["raw"]
    for cuts in ((), range(97, len(c["raw"]), 97)):
        with m.BamReader() as r:
            edges = [0] + list(cuts) + [len(c["raw"])]
            with pytest.raises(m.BamRefused) as e:
                for a, b in zip(edges, edges[1:]):
                    r.add(c["raw"][a:b])
                    r.run(segment_bytes=bc.SEGMENT, **c.get("opts", {}))
                r.finish()
            assert (e.value.reason, e.value.record, e.value.offset) == c["refused"], (name, bool(cuts))
            assert "[%s]" % c["refused"][0] in str(e.value)
            with pytest.raises(m.MktError):
                r.text()
            # the same reader decodes a good stream afterwards
            r.add(good)
            r.run()
            r.finish()
            assert r.text() == bd.view(good)


def test_many_segments_and_many_record_blocks():
    """70000 records: the one-workgroup scans take more than one turn (over 256 segments at any size here, over 256 blocks of 256
    records), whole and in pieces."""
    c = bc.big_case()
    want = b"".join(c["lines"])
    for seg, cuts in ((bc.SEGMENT, ()), (0, ()), (2048, range(1 << 20, len(c["raw"]), 1 << 20))):
        text, _, infos = decode(c["raw"], cuts, segment_bytes=seg)
        assert text == want, seg
        assert sum(i.records for i in infos) == len(c["lines"]) > 65536 and (seg == 0 or infos[0].segments > 256)


@pytest.mark.parametrize("bad_at", [300, 69000])
def test_first_refused_record_among_many_blocks(bad_at):
    """the refused record lies in the first and in the second turn of the scan over the blocks' sums"""
    c = bc.big_case(bad_at)
    raw = c["raw"]
    if bad_at == 300:                                     # a second refused record far behind the first: the first is named
        other = bc.big_case(69000)
        raw = raw[:other["bad_offset"]] + other["raw"][other["bad_offset"]:]
    with m.BamReader() as r:
        r.add(raw)
        with pytest.raises(m.BamRefused) as e:
            r.run()
        assert (e.value.reason, e.value.record, e.value.offset) == ("tag_type", bad_at, c["bad_offset"])


def test_options_are_checked_and_device_text_is_the_text():
    raw = bc.case("lengths")["raw"]
    with m.BamReader() as r, m.Context("unc", device=0) as ctx:
        r.add(raw)
        for bad in ({"segment_bytes": 128}, {"segment_bytes": 768}, {"max_record": 16}, {"max_record": (16 << 20) + 1}):
            with pytest.raises(m.MktError):
                r.run(**bad)
        r.run()
        d, n = r.device_text()
        assert n == len(bd.view(raw)) and ctx.copy_to_host(d, n + 64) == bd.view(raw) + bytes(64)
        t = r.timing_ms()
        assert set(t) == {"header", "index_guess", "resolve", "length", "scan", "emit"} and t["emit"] > 0
