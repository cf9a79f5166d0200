"""The host half of adapter and quality trimming without a GPU: mkt_trim_check through the library; microcket_amd/csrc/mkt_trim.h driven
by tests/host/trim_host.cpp (built with the address and undefined-behaviour sanitizers, run as its own process) over the directed
families; its limit table against the definition's float32 arithmetic; and the golden logs in bin/makestat's trim-log reader."""
import os
import subprocess

import pytest

import ktrim_cases as kc
import ktrimdef as kd
import util
from test_ktrim_def import golden

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "trim_host_san")
PLAIN = os.path.join(util.ROOT, "tests", "host", "_build", "trim_host")
MAKESTAT = os.path.join(util.ROOT, "microcket_amd", "bin", "makestat")


@pytest.fixture(scope="module", autouse=True)
def _built():
    util.ensure_built()
    from microcket_amd import build
    build.build_makestat()
    assert os.path.exists(HOST) and os.path.exists(PLAIN)


def host(args, stdin=b"", exe=None):
    p = subprocess.run([exe or HOST, *args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode()


def _args(opts):
    return [f"{k}={v}" for k, v in opts.items()]


def test_check_through_the_library():
    import microcket_amd as m
    assert m.trim_check() is None
    assert m.trim_check(kit="BGI", min_size=10, window=510, min_qual=93) is None
    assert m.trim_check(adapter1="ACGTACGT") is None and m.trim_check(adapter1="ACGTACGTAC", adapter2="ACGTACGTTTTT") is None
    for name, opts, _ in kc.REFUSED_OPTIONS:
        assert m.trim_check(**opts), name
    assert "CLIP" in m.trim_check(kit="clip") and "adapter size 7" in m.trim_check(adapter1="ACGTACG")
    assert m.trim_check(kit="illumina", adapter1="ACG") is None      # the kit wins: the adapters are not looked at


def test_adapter_table_and_refusals_in_the_host_program():
    for name, canon in kd.KIT_NAMES.items():
        a1, a2 = kd.KITS[canon]
        n = min(len(a1), len(a2))
        assert host(["check", f"kit={name}"]) == f"ok {a1[:n]} {a2[:n]}\n"
    assert host(["check"]) == "ok {0} {0}\n".format(kd.KITS["illumina"][0])
    assert host(["check", "adapter1=ACGTACGTAC", "adapter2=TTTTACGTACGTAC"]) == "ok ACGTACGTAC TTTTACGTAC\n"
    for name, opts, _ in kc.REFUSED_OPTIONS:
        assert host(["check", *_args(opts)]).startswith("refused: "), name


@pytest.mark.parametrize("mismatch", [0.0, 0.05, 0.1, 0.125, 0.2, 0.25, 0.3, 1 / 3, 0.5, 0.7, 0.999, 1.0])
def test_limit_table_is_the_float32_arithmetic(mismatch):
    got = [int(x) for x in host(["limits", repr(mismatch)]).split()]
    assert got == kd.limit_table(mismatch) and len(got) == kd.MAX_ADAPTER + 1
    assert got == [int(x) for x in host(["limits", repr(mismatch)], exe=PLAIN).split()]


def test_host_program_on_the_directed_families():
    """every pair of every batch: the kept length, the class and the dimer flag of the definition"""
    for name, opts, argv, records in kc.all_batches():
        P = kd.resolve(**opts)
        lines = "".join("\t".join((h1, s1, "+", q1, h2, s2, "+", q2)) + "\n" for h1, s1, q1, h2, s2, q2 in records if "\t" not in h1)
        want = []
        for h1, s1, q1, h2, s2, q2 in records:
            if "\t" in h1:
                continue
            k, cls, dim = kd.trim_pair(s1.encode(), q1.encode(), s2.encode(), q2.encode(), P)
            want.append(f"{k} {cls} {int(dim)}\n")
        assert host(["pairs", *_args(opts)], lines.encode()) == "".join(want), name


def test_host_program_record_check():
    good = ("@a", "ACGT" * 10, "+", "I" * 40)
    cases = [(("a",) + good[1:], 1), ((good[0], good[1], "-", good[3]), 2), (("@" + "h" * 126,) + good[1:], 3), ((good[0], "A" * 511, "+", "I" * 511), 4),
             ((good[0], good[1], "+", "I" * 39), 5), ((good[0], good[1], "+", "I" * 39 + " "), 6), ((good[0], good[1], "", good[3]), 2)]
    for rec, code in cases:
        for first in (True, False):
            f = (rec + good) if first else (good + rec)
            assert host(["pairs"], ("\t".join(f) + "\n").encode()) == f"bad {code}\n", (rec[0][:10], code, first)
    assert host(["pairs"], ("\t".join(("@" + "h" * 125, "A" * 510, "+", "I" * 510) * 2) + "\n").encode()).split()[1] == str(kd.PASS)


def test_golden_logs_parse_in_makestat(tmp_path):
    """bin/makestat reads PREFIX.trim.log: its Total line is the log's"""
    for c in golden()["cases"]:
        (tmp_path / "s.trim.log").write_text(c["log"])
        (tmp_path / "s.rmdup.log").write_text("Total\t%d\nUniq\t%d\n" % (c["pairs"], c["pairs"]))
        p = subprocess.run([MAKESTAT, "s", "no"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        lines = p.stdout.decode().splitlines()
        assert "Total\t{:,}\t100.0".format(c["pairs"]) in lines, (c["name"], p.stdout, p.stderr)
