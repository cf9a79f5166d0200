"""bin/pairs2matrix's front end without a GPU: every command line it refuses before it asks for a device (a usage error, an unreadable
file, a bad value, table, list, track or BEDPE) answers with the exit code and the bytes of stderr that
tests/golden/pairs2matrix_cli_golden.json holds.  The file was recorded once, by tests/golden/make_pairs2matrix_cli_golden.py, from the
binary of the commit it names, before the front end was rewritten around one option table: which error wins when a command line holds
two is part of what is pinned.  MKT_PAIRS2MATRIX names another binary to hold to the same file."""
import json
import os
import subprocess

import pytest

import util

EXE = os.environ.get("MKT_PAIRS2MATRIX") or os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
GOLDEN = json.load(open(os.path.join(util.ROOT, "tests", "golden", "pairs2matrix_cli_golden.json")))
GROUPS = sorted({c["group"] for c in GOLDEN["cases"]})


def _built():
    if "MKT_PAIRS2MATRIX" not in os.environ:
        from microcket_amd import build
        build.build_lib()
        build.build_pairs2matrix()
    return EXE


def test_the_recording_holds_what_it_is_there_for():
    cases = GOLDEN["cases"]
    assert GROUPS == sorted(["missing value", "unknown option", "needs its switch", "accepted", "bad value", "cross-option", "table", "track", "bedpe", "unreadable", "precedence"])
    assert 100 <= len(cases) <= 400 and {c["exit"] for c in cases} == {2, 10, 12}                  # nothing that reaches the device
    assert GOLDEN["usage"].startswith("Usage: {EXE} -g <chrom.sizes>") and len(GOLDEN["recorded_from"]) >= 7
    n = lambda g: sum(c["group"] == g for c in cases)
    assert n("precedence") >= 8 and n("unreadable") >= 5 and n("table") >= 4 and n("track") >= 4 and n("bedpe") >= 5
    for c in cases:
        assert c["exit"] != 2 or c["stderr"].endswith("{USAGE}"), c["name"]                         # every usage error prints the usage text
        assert c["exit"] == 2 or "{USAGE}" not in c["stderr"] and c["stderr"].startswith("Error: ") and c["stderr"].count("\n") == 1, c["name"]
    text = " ".join(a for c in cases for a in c["argv"])
    for opt in GOLDEN["usage"].replace("[", " ").replace("]", " ").split():                         # every option of the usage text is in some case
        if opt.startswith("-") and opt != "-":
            assert opt in text, opt


@pytest.mark.parametrize("group", GROUPS)
def test_exit_code_and_stderr_are_those_of_the_recording(group, tmp_path):
    exe = _built()
    wrong = []
    for k, c in enumerate(c for c in GOLDEN["cases"] if c["group"] == group):
        d = tmp_path / str(k)
        d.mkdir()
        for fn, text in c["files"].items():
            (d / fn).write_bytes(text.encode())
        r = subprocess.run([exe] + [a.replace("{TMP}", str(d)) for a in c["argv"]], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        want = c["stderr"].replace("{USAGE}", GOLDEN["usage"]).replace("{EXE}", exe).replace("{TMP}", str(d))
        if (r.returncode, r.stderr.decode(), r.stdout) != (c["exit"], want, b"") or sorted(os.listdir(d)) != sorted(c["files"]):
            wrong.append((c["name"], c["argv"], r.returncode, r.stderr.decode()[:300], c["exit"], want[:300]))
    assert not wrong, wrong[:5]
