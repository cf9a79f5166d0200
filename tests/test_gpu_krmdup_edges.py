"""mkt_rmdup_* at its batch, table, key and copy edges: every case of tests/krmdup_edge_cases.py through m.rmdup -- resident and in
streaming segments, two outputs and interleaved -- byte for byte against the oracle restatement (read 1, read 2, log) and against the
hashes of the reference build's own output (tests/golden/krmdup_edges_golden.json); the key-window argument sets through bin/krmdup
as well, which parses them itself.  A mismatch names the first differing record and the edge its pair was built for."""
import os

import pytest

import krmdup_edge_cases as ec
import microcket_amd as m
import util
from test_krmdup_edges_host import check_golden

pytestmark = pytest.mark.gpu


def same(case, how, mate, got, want):
    """got == want, or the first record that differs and what its pair is there for"""
    if got == want:
        return
    g, w = got.split(b"\n"), want.split(b"\n")
    k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
    per = 8 if mate == "interleaved" else 4
    order = ec.restated(case.name)["order"]
    rec = k // per
    edge = case.label(order[rec]) if rec < len(order) else "behind the last expected record"
    show = lambda L: L[k][:80] if k < len(L) else None
    pytest.fail("%s, %s, %s: %d bytes for %d; record %d differs in line %d: got %r, expected %r; expected there: %s"
                % (case.name, how, mate, len(got), len(want), rec, k % per, show(g), show(w), edge))


def run(case, how, want, **kw):
    o1, o2, ol = want
    r1, r2, st = m.rmdup(case.text, **ec.kwargs(case.args), **kw)
    assert util.krmdup_log(*st) == ol, (case.name, how, st, ol)
    if kw.get("interleaved"):
        assert r2 == b""
        same(case, how, "interleaved", r1, ec.interleave(o1, o2))
    else:
        same(case, how, "read 1", r1, o1)
        same(case, how, "read 2", r2, o2)
    return r1, r2


@pytest.mark.parametrize("name", ec.NAMES)
def test_rmdup_edge_case(name, monkeypatch):
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    case = ec.get(name)
    want = ec.oracle(name)
    r1, r2 = run(case, "resident", want)
    if case.golden:
        check_golden(name, r1, r2, want[2])
    if case.interleaved:
        inter, _ = run(case, "resident", want, interleaved=True)
        if case.golden:
            check_golden(name, r1, r2, want[2], inter)
    if case.segment_mb is not None:
        monkeypatch.setenv("MKT_RMDUP_SEGMENT_MB", str(case.segment_mb))
    for k, piece in enumerate(case.pieces):
        how = "streaming, %s" % ("one piece" if piece == 0 else "pieces of %d bytes" % piece)
        run(case, how, want, stream=True, piece=piece or len(case.text))
        if case.interleaved and k == 0:
            run(case, how, want, stream=True, piece=piece or len(case.text), interleaved=True)


@pytest.mark.parametrize("name", ec.GROUPS["key_window"])
def test_krmdup_executable_parses_the_window(name):
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    case = ec.get(name)
    o1, o2, ol = ec.oracle(name)
    exe = os.path.join(os.path.dirname(m.exe_path()), "krmdup")
    rc, r1, r2, log, err = util.krmdup_run_cli(exe, case.text, False, case.args)
    assert rc == 0, err
    assert log == ol, (name, log, ol)
    same(case, "bin/krmdup", "read 1", r1, o1)
    same(case, "bin/krmdup", "read 2", r2, o2)
