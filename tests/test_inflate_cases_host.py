"""The directed BGZF files of tests/inflate_cases.py against the two independent checkers, without a GPU: every accepted case inflates
to its text by zlib and by inflatedef (RFC 1951), every refused case is refused by inflatedef, by the framing check (CRC-32, ISIZE) or by
the block-table walk of px2def.bgzf_blocks, for the reason the case names.  No case is skipped."""
import struct
import zlib

import pytest

import inflate_cases
import inflatedef
import px2def

# the reason of a case -> what the independent checker says
WALK = {"bad_magic": "no BGZF block", "plain_gzip": "no BGZF block", "xlen": "not the one BC subfield", "past_file": "runs past the file"}
INFLATE = {"block_type_3": "block type 3", "stored_nlen": "NLEN is not the complement", "stored_padding": "up to the byte boundary are not zero",
           "ll_oversubscribed": "literal/length code: over-subscribed", "ll_incomplete": "literal/length code: incomplete", "d_oversubscribed": "distance code: over-subscribed",
           "d_incomplete": "distance code: incomplete", "cl_oversubscribed": "code-length code: over-subscribed", "cl_incomplete": "code-length code: incomplete",
           "no_end_of_block": "no code for end of block", "repeat_first": "at the first length", "repeat_past_last": "runs past the last code length",
           "length_symbol": "length symbol 286", "distance_symbol": "distance symbol 30", "distance_before_start": "reaches before the start",
           "past_span": "the stream ends inside", "trailing_bytes": "trailing bytes after the final block"}
FRAME = ("output_long", "output_short", "crc")


def members(gz):
    return [(c, gz[c + 18:c + b - 8], struct.unpack_from("<II", gz, c + b - 8)) for c, b, _, _ in px2def.bgzf_blocks(gz, check=False)]


def test_families_are_all_there():
    fam = {c["family"] for c in inflate_cases.cases()}
    assert fam == {"block_kinds", "matches", "codes", "refused"}
    assert set(WALK) | set(INFLATE) | set(FRAME) == {c["refused"] for c in inflate_cases.refused()}
    assert inflate_cases.BATCH == 64
    assert all(len(c["gz"]) <= 48 * 0x10000 for c in inflate_cases.cases())


@pytest.mark.parametrize("name", [c["name"] for c in inflate_cases.accepted()])
def test_accepted_cases_inflate_to_their_text(name):
    c = inflate_cases.case(name)
    out_z, out_d = [], []
    for _, raw, (crc, isize) in members(c["gz"]):
        z = zlib.decompress(raw, -15)
        _, d = inflatedef.inflate(raw)
        assert len(z) == isize <= 65536 and zlib.crc32(z) == crc and d == z
        out_z.append(z)
        out_d.append(d)
    assert b"".join(out_z) == c["text"] == b"".join(out_d)


@pytest.mark.parametrize("name", [c["name"] for c in inflate_cases.refused()])
def test_refused_cases_are_refused_for_their_reason(name):
    c = inflate_cases.case(name)
    why = c["refused"]
    if why in WALK:
        with pytest.raises(ValueError) as e:
            px2def.bgzf_blocks(c["gz"], check=False)
        assert WALK[why] in str(e.value) and ("at %d" % inflate_cases.refused_offset(c)) in str(e.value)
        if why == "plain_gzip":
            assert c["gz"][:3] == b"\x1f\x8b\x08" and not c["gz"][3] & 4 and zlib.decompress(c["gz"], 31)       # a gzip file that gzip reads
        return
    bad = []
    for off, raw, (crc, isize) in members(c["gz"]):
        try:
            _, d = inflatedef.inflate(raw)
        except inflatedef.InflateError as e:
            bad.append((off, "inflate", str(e)))
            continue
        if len(d) > isize:
            bad.append((off, "output_long", ""))
        elif len(d) < isize:
            bad.append((off, "output_short", ""))
        elif zlib.crc32(d) != crc:
            bad.append((off, "crc", ""))
    assert len(bad) == 1 and bad[0][0] == inflate_cases.refused_offset(c) > 0
    if why in FRAME:
        assert bad[0][1] == why
    else:
        assert bad[0][1] == "inflate" and INFLATE[why] in bad[0][2], bad
