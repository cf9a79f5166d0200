"""The definition of adapter and quality trimming (tests/ktrimdef.py) against every golden made by Ktrim 1.6.0
(tests/golden/ktrim_golden.json): the seeded cases by hash, the directed batches of tests/ktrim_cases.py literally; and what the
directed families reach.  No GPU."""
import json
import os

import pytest

import ktrim_cases as kc
import ktrimdef as kd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ktrim_golden.json")
_cache = {}


def golden():
    if "g" not in _cache:
        with open(GOLDEN) as f:
            _cache["g"] = json.load(f)
    return _cache["g"]


def case_input(c):
    """the two streams of a seeded case (cached: the generator is the slow part)"""
    key = ("case", c["name"])
    if key not in _cache:
        t1, t2 = kd.synth(c["seed"], c["pairs"], c["read_len"], c.get("kit", "illumina"))
        assert (kd.sha(t1), kd.sha(t2)) == (c["input1_sha256"], c["input2_sha256"]), c["name"]
        _cache[key] = (t1, t2)
    return _cache[key]


def batch_input(b):
    if "batches" not in _cache:
        _cache["batches"] = {name: (opts, argv, kc.text_of(records)) for name, opts, argv, records in kc.all_batches()}
    opts, argv, (t1, t2) = _cache["batches"][b["name"]]
    assert (kd.sha(t1), kd.sha(t2)) == (b["input1_sha256"], b["input2_sha256"]) and opts == b["opts"] and argv == b["argv"], b["name"]
    return t1, t2


def batch_output(b):
    """the reference's stdout for a directed batch: the definition's interleaved stream, held against the golden's hash of the program's"""
    key = ("out", b["name"])
    if key not in _cache:
        il = kd.trim_stream(*batch_input(b), **b["opts"])[0]
        assert kd.sha(il) == b["stdout_sha256"], b["name"]
        _cache[key] = il
    return _cache[key]


def test_seeded_goldens():
    for c in golden()["cases"] + [golden()["pipe"]]:
        t1, t2 = case_input(c)
        il, r1, r2, st = kd.trim_stream(t1, t2, **c.get("opts", {}))
        assert kd.sha(il) == c["stdout_sha256"], c["name"]
        if "log" in c:
            assert kd.log_text(st) == c["log"] and (kd.sha(r1), kd.sha(r2)) == (c["read1_sha256"], c["read2_sha256"]), c["name"]
            assert (r1, r2) == kd.split_interleaved(il)


def test_directed_goldens():
    names = [b["name"] for b in golden()["batches"]]
    assert names == [n for n, _, _, _ in kc.all_batches()]
    for b in golden()["batches"]:
        t1, t2 = batch_input(b)
        il, r1, r2, st = kd.trim_stream(t1, t2, **b["opts"])
        assert kd.sha(il) == b["stdout_sha256"] and kd.log_text(st) == b["log"], b["name"]


def _log(b):
    return dict((k, int(v)) for k, v in (line.split("\t") for line in b["log"].splitlines()))


def test_families_reach_their_classes():
    g = {b["name"]: b for b in golden()["batches"]}
    for kit in ("illumina", "nextera", "transposase", "bgi"):
        lg = _log(g[f"adapter_position_{kit}"])
        # reads of 100: inserts 0 .. 97 by the adapter (0 .. 35 dropped, 0 and 1 dimers), 98 and 99 by the tail, 100 untouched;
        # reads of 150: 60 .. 68, 124 .. 132 and 147 by the adapter, 148 and 149 by the tail
        assert lg["Dimer"] == 2 and lg["Dropped"] == 36 and lg["TailHit"] == 2 + 2 and lg["Aadaptor"] == 98 + 19, (kit, lg)
    for name in ("mismatch_limit_m0.125", "mismatch_limit_m0.0", "mismatch_limit_m0.3"):
        lg = _log(g[name])
        assert 0 < lg["Aadaptor"] < lg["Total"], (name, lg)
    lg = _log(g["quality_default"])
    assert lg["Dropped"] >= 2 and lg["TailHit"] == 1


def test_observed_rules():
    P = kd.resolve()
    q = b"I" * 100
    s = kc.rnd(5, 100).encode()
    assert kd.trim_pair(s[:80], q[:80], s[:70], q[:70], P)[0] == 70
    for good, want in ((60, 60), (40, 40), (37, 37), (36, 36), (35, 0)):
        assert kd.trim_pair(s, b"I" * good + b"#" * (100 - good), s, q, P)[0] == want
    assert kd.limit_table(0.125)[:18] == [0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 3]
    assert kd.limit_table(0.0) == [0] * 65 and kd.limit_table(1.0) == list(range(65))


@pytest.mark.parametrize("name", [r[0] for r in kc.REFUSED_INPUT])
def test_refused_input(name):
    _, t1, t2, opts, what = next(r for r in kc.REFUSED_INPUT if r[0] == name)
    with pytest.raises(ValueError, match=what.replace("read pairs in stream", "records in stream")):
        kd.trim_stream(t1, t2, **opts)


def test_refused_options():
    for name, opts, _ in kc.REFUSED_OPTIONS:
        with pytest.raises(ValueError):
            kd.resolve(**opts)
