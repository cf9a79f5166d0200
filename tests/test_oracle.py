"""The oracle (oracle/sam2pairs_oracle.c, a CPU restatement) is pinned:
  * against the committed golden vectors, which hold outputs of the REFERENCE ITSELF
    (tests/golden/golden.json, made by tests/golden/make_golden.py from oracle/_ref);
  * against what oracle/_ref printed for further seeded inputs (tests/golden/ref_build_golden.json), and against
    oracle/_ref directly whenever that build is present."""
import os

import pytest

import util


def _input_bytes(ent):
    if ent["kind"] == "file":
        return open(os.path.join(util.GOLDEN, ent["name"]), "rb").read()
    return util.synth(ent["profile"], ent["seed"], ent["groups"], ent["read_len"], ent["genome"], ent["lanes"], 1)


def test_golden_inputs_reproducible(golden):
    """The seeded generator regenerates the exact inputs the golden vectors were made from."""
    for ent in golden["inputs"]:
        assert util.sha(_input_bytes(ent)) == ent["sha256"], ent["name"]


def test_oracle_matches_golden(golden):
    n = 0
    for ent in golden["inputs"]:
        text = _input_bytes(ent)
        for c in ent["cases"]:
            pairs, sam, log, st = util.oracle_run(text, c["mode"], c["threads"], c["ratio"], c["mapq"], c["sam"])
            cp, cs = util.canon(pairs), util.canon(sam)
            tag = (ent["name"], c["mode"], c["threads"], c["ratio"], c["mapq"], c["sam"])
            assert log.decode() == c["log"], tag
            assert cp.count(b"\n") == c["pairs_lines"], tag
            assert util.sha(cp) == c["pairs_sha256"], tag
            assert util.sha(cs) == c["sam_sha256"], tag
            if "pairs_sorted" in c:
                assert cp.decode() == c["pairs_sorted"], tag
            n += 1
    assert n >= 50


REF_BUILD_INPUTS = [("unc", 101, 4000, ("unc",)), ("flash", 102, 4000, ("flash",)), ("stress", 103, 9000, ("unc", "flash"))]
REF_BUILD_GRID = ((2, 0.5, 10, True), (4, 0.5, 10, True), (8, 0.5, 10, True), (4, 0.8, 30, False), (5, 0.5, 0, True))
Q2_THREADS = (2, 4, 8)


def ref_key(profile, seed, groups, mode, T, ratio, mapq, sam):
    return f"{profile}/{seed}/{groups}/{mode}/T{T}/r{ratio}/q{mapq}/sam{int(sam)}"


def _ref_build_golden():
    """What oracle/_ref printed for the inputs below (tests/golden/make_ref_build_golden.py): the checks hold without that build."""
    import json
    with open(os.path.join(util.GOLDEN, "ref_build_golden.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("profile,seed,groups,modes", REF_BUILD_INPUTS)
def test_oracle_matches_reference_build(profile, seed, groups, modes):
    text = util.synth(profile, seed, groups)
    rec = _ref_build_golden()["sam2pairs"]
    for mode in modes:
        for (T, ratio, mapq, sam) in REF_BUILD_GRID:
            op, osam, ol, st = util.oracle_run(text, mode, T, ratio, mapq, sam)
            want = rec[ref_key(profile, seed, groups, mode, T, ratio, mapq, sam)]
            assert util.sha(text) == want["input_sha256"], (profile, seed, groups)
            assert util.sha(util.canon(op)) == want["pairs_sha256"], (profile, mode, T, ratio, mapq)
            assert util.sha(util.canon(osam)) == want["sam_sha256"], (profile, mode, T, ratio, mapq)
            assert ol.decode() == want["log"], (profile, mode, T, ratio, mapq, want["log"], ol)
            if util.have_ref():
                rc, rp, rs, rl, err = util.ref_run(text, mode, T, ratio, mapq, sam)
                assert rc == 0
                assert util.canon(rp) == util.canon(op), (profile, mode, T, ratio, mapq)
                assert util.canon(rs) == util.canon(osam), (profile, mode, T, ratio, mapq)
                assert rl == ol, (profile, mode, T, ratio, mapq, rl, ol)


def q2_input():
    return util.synth("unc", 77, (1 << 18) + (1 << 17), read_len=50)


def test_quirk_q2_across_batches():
    """K just above 2^18 surviving groups with a LARGE remainder (keeps the reference clear of its
    own `loaded` race): the logged selfCircle depends on the thread count exactly as the closed form says."""
    text = q2_input()
    rec = _ref_build_golden()["quirk_q2"]
    for T in Q2_THREADS:
        op, osam, ol, st = util.oracle_run(text, "unc", T, 0.5, 0, False)
        assert st.groups % (1 << 18) >= (1 << 16)
        want = rec[str(T)]
        assert util.sha(text) == want["input_sha256"]
        assert ol.decode() == want["log"], (T, want["log"], ol)
        assert util.sha(util.canon(op)) == want["pairs_sha256"]
        if util.have_ref():
            rc, rp, rs, rl, err = util.ref_run(text, "unc", T, 0.5, 0, False)
            assert rc == 0
            assert rl == ol, (T, rl, ol)
            assert util.sha(util.canon(rp)) == util.sha(util.canon(op))


def test_oracle_cli_exit_codes(tmp_path):
    import subprocess
    exe = util.ORACLE_EXE
    sam = tmp_path / "x.sam"
    sam.write_bytes(util.synth("unc", 1, 10))
    assert subprocess.run([exe], stderr=subprocess.PIPE).returncode == 2
    assert subprocess.run([exe, str(sam), "unc", str(tmp_path / "o"), "1"], stderr=subprocess.PIPE).returncode == 5
    assert subprocess.run([exe, str(sam), "bad", str(tmp_path / "o"), "4"], stderr=subprocess.PIPE).returncode == 6
    assert subprocess.run([exe, str(tmp_path / "missing.sam"), "unc", str(tmp_path / "o"), "4"], stderr=subprocess.PIPE).returncode == 10
