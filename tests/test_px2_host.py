"""The definition of final.pairs.gz.px2 (tests/px2def.py) against what the reference's bgzip | pairix wrote (tests/golden/px2_golden.json),
without a GPU; and the host half of the GPU path (microcket_amd/csrc/mkt_px2.h) through its stand-alone driver, plain and under
ASan/UBSan."""
import json
import os
import subprocess

import pytest

import px2_inputs
import px2def

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "px2_golden.json")) as f:
    GOLDEN = json.load(f)

ACCEPTED = [c["name"] for c in px2_inputs.accepted()]
REFUSED = [c["name"] for c in px2_inputs.refused()]
LEVELS = {"zlib1": 1, "zlib6": 6, "stored": 0}


def _own_files(case, level=6, cuts=None):
    gz = px2def.bgzf_compress(case["text"], level, cuts)
    blocks = px2def.bgzf_blocks(gz)
    ix = px2def.build_index(case["text"], blocks, len(gz))
    return gz, blocks, ix, px2def.bgzf_compress(px2def.serialize(ix), level)


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(c["name"] for c in px2_inputs.cases())
    assert os.path.getsize(os.path.join(HERE, "golden", "px2_golden.json")) < (1 << 20)


@pytest.mark.parametrize("name", ACCEPTED)
@pytest.mark.parametrize("level", sorted(LEVELS))
def test_builder_equals_reference_index(name, level):
    case = px2_inputs.case(name)
    gz, blocks, ix, px2 = _own_files(case, LEVELS[level])
    assert px2def.bgzf_inflate(gz) == case["text"]
    back = px2def.parse_px2(px2)                           # every byte accounted for
    assert px2def.to_text_offsets(back, blocks, len(gz)) == GOLDEN[name]["index"]
    assert all(order == sorted(order) for order in back["bin_order"])
    assert px2def.count_lines(px2) == GOLDEN[name]["n"]


@pytest.mark.parametrize("name", ["blocks_long_runs", "blocks_many_bins", "many_pairs"])
def test_builder_does_not_depend_on_the_cuts(name):
    """The reference's bgzip cuts at line ends; cutting this project's way (every 0xff00 bytes) or there gives the same index in text offsets."""
    case = px2_inputs.case(name)
    gz, blocks, ix, px2 = _own_files(case, 1, cuts=GOLDEN[name]["bgzip_block_starts"][1:-1])
    assert [b[2] for b in blocks] == GOLDEN[name]["bgzip_block_starts"]
    assert px2def.to_text_offsets(px2def.parse_px2(px2), blocks, len(gz)) == GOLDEN[name]["index"]


@pytest.mark.parametrize("name", ACCEPTED)
def test_region_lookup_returns_the_reference_lines(name):
    case = px2_inputs.case(name)
    gz, _, _, px2 = _own_files(case, 1)
    assert sorted(GOLDEN[name]["queries"]) == sorted(case["regions"])
    for region, lines in GOLDEN[name]["queries"].items():
        assert px2def.query(gz, px2, region) == lines, region


@pytest.mark.parametrize("name", REFUSED)
def test_refused_inputs_name_the_line(name):
    case = px2_inputs.case(name)
    gz = px2def.bgzf_compress(case["text"], 1)
    with pytest.raises(px2def.Px2Error) as e:
        px2def.build_index(case["text"], px2def.bgzf_blocks(gz), len(gz))
    assert e.value.line == case["refused"]
    assert "index" not in GOLDEN[name]


def test_block_cases_hit_the_block_edges():
    for name in ("blocks_long_runs", "blocks_many_bins"):
        case = px2_inputs.case(name)
        text = case["text"]
        starts = {a for a, _ in px2def.split_lines(text)}
        B = px2def.BGZF_RAW
        assert B in starts and 3 * B in starts and 2 * B not in starts and text[2 * B - 1:2 * B] != b"\n"
        gz, blocks, ix, _ = _own_files(case, 1)
        begs = {beg for bins in ix["bins"] for chunks in bins.values() for beg, _ in chunks}
        ends = {end for bins in ix["bins"] for chunks in bins.values() for _, end in chunks}
        assert blocks[1][0] << 16 in begs and blocks[1][0] << 16 in ends          # a chunk ends, the next begins, at offset 0 of block 1
        first_of_pair2 = min(beg for chunks in ix["bins"][1].values() for beg, _ in chunks)
        assert first_of_pair2 == blocks[3][0] << 16                              # the pair boundary on block 3
    many = px2_inputs.case("blocks_many_bins")["text"].count(b"\n") - 2
    assert sum(len(b) for b in px2def.build_index(*_blockargs("blocks_many_bins"))["bins"]) > 0.8 * many > 800      # a chunk for most of its lines
    assert sum(len(b) for b in px2def.build_index(*_blockargs("blocks_long_runs"))["bins"]) < 20


def _blockargs(name):
    text = px2_inputs.case(name)["text"]
    gz = px2def.bgzf_compress(text, 1)
    return text, px2def.bgzf_blocks(gz), len(gz)


# ---- the host half of the GPU path ---------------------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "tests", "host", "_build", "px2_host")              # made by build() (microcket_amd/build.py build_test_tools)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_half_driver(sanitize):
    """names -> table and reappearing-pair check, header serialiser: the driver's output equals px2def's for every case."""
    exe = HOST + "_san" if sanitize else HOST
    for case in px2_inputs.cases():
        heads = []                                         # (line, name) of the first record of every run, as the GPU hands them over
        prev = None
        bad = None
        for j, (a, b) in enumerate(px2def.split_lines(case["text"])):
            if case["text"][a:a + 1] == b"#":
                continue
            try:
                c1, _, c2 = px2def.parse_record(case["text"], a, b, j + 1)
            except px2def.Px2Error:
                break
            if (c1, c2) != prev:
                heads.append((j, c1 + b"|" + c2))
                prev = (c1, c2)
        seen = set()
        for j, nm in heads:
            if nm in seen and bad is None:
                bad = j + 1
            seen.add(nm)
        n_lines = len(px2def.split_lines(case["text"]))
        inp = "%d %d\n" % (n_lines, len(heads)) + "".join("%d %s\n" % (j, nm.decode()) for j, nm in heads)
        r = subprocess.run([exe], input=inp.encode(), capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        out = r.stdout.decode().split("\n")
        if bad is not None:
            assert out[0] == "reappears %d" % bad
            continue
        names = []
        for _, nm in heads:
            names.append(nm)
        want = px2def.serialize({"n_lines": n_lines, "names": names, "bins": [{}] * len(names), "linear": [[]] * len(names)})
        assert out[0] == "ok %d" % len(names)
        assert bytes.fromhex(out[1]) == want
