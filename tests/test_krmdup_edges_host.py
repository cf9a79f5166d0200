"""The duplicate remover's edge cases without a GPU (tests/krmdup_edge_cases.py): every case sits at the edge it was written for,
worked out from the numpy restatement of key, bucket and slot; the checker oracle/krmdup_oracle.c reproduces what the reference
build printed for every case (tests/golden/krmdup_edges_golden.json, made by oracle/_ref/krmdup.ref and krmdup.pipe.ref) and, where
that build is present, a live run of it; and, so that the checker does not go unchecked, an independent plain-Python restatement of
krmdup.cpp:88-227 and the numpy one agree with it."""
import json
import os

import numpy as np
import pytest

import krmdup_edge_cases as ec
import util

GOLDEN = os.path.join(util.GOLDEN, "krmdup_edges_golden.json")
_cache = {}


def golden():
    if "g" not in _cache:
        with open(GOLDEN) as f:
            _cache["g"] = {c["name"]: c for c in json.load(f)["cases"]}
    return _cache["g"]


def check_golden(name, r1, r2, log, inter=None):
    """outputs against a case's golden entry: both files, the log, the records of the interleaved form"""
    g = golden()[name]
    assert log.decode() == g["log"], name
    assert (util.sha(r1), util.sha(r2)) == (g["read1_sha256"], g["read2_sha256"]), name
    inter = ec.interleave(r1, r2) if inter is None else inter
    assert util.sha(b"\n".join(util.fastq_records(inter))) == g["pipe_records_sha256"], name


@pytest.mark.parametrize("name", ec.NAMES)
def test_case_sits_at_its_edge(name):
    print(name, ec.get(name).check())


def test_sizes_and_names():
    assert os.path.getsize(GOLDEN) < 100_000
    assert list(golden()) == [n for n in ec.NAMES if ec.get(n).golden]
    assert [n for n in ec.NAMES if not ec.get(n).golden] == ["rag_extra%d" % k for k in range(1, 8)]
    for n in ec.NAMES:
        c = ec.get(n)
        assert len(c.text) < 27 << 20 and util.sha(c.text) == golden().get(n, {"input_sha256": util.sha(c.text)})["input_sha256"], n      # the generator
        assert list(c.args) == golden().get(n, {"args": list(c.args)})["args"]


@pytest.mark.parametrize("name", ec.NAMES)
def test_oracle_reproduces_the_reference_build(name):
    c = ec.get(name)
    o1, o2, ol = ec.oracle(name)
    # the numpy restatement: the same counters, and the same pairs in the same order (their read-1 records cut from the input)
    r = ec.restated(name)
    assert ol == util.krmdup_log(*r["stats"]), name
    buf, st, en = ec.lines_of(c.text)
    L = lambda k: c.text[st[k]:en[k]]
    if len(r["order"]) <= 3000:
        assert o1 == b"".join(b"%s\n%s\n+\n%s\n" % (L(8 * o), L(8 * o + 1), L(8 * o + 3)) for o in r["order"]), name
    else:
        assert o1.count(b"\n") == 4 * len(r["order"])
        ids = np.frombuffer(o1, dtype=np.uint8).reshape(len(r["order"]), -1)[:, :7] if name != "carry" else None
        if ids is not None:                                   # fixed-shape records: the id columns of all of them
            want = np.frombuffer(c.text, dtype=np.uint8).reshape(r["stats"][0], -1)[r["order"], :7]
            assert (ids == want).all(), name
    if c.golden:
        check_golden(name, o1, o2, ol)
    else:                                                     # lines behind the last whole pair: ignored; the pairs before them unchanged
        assert (o1, o2, ol) == ec.oracle("rag_nonl")[:2] + (ol,) and ol == ec.oracle("rag_nonl")[2]
    if os.path.exists(util.KRMDUP_REF) and c.golden:
        rc, q1, q2, qlog, err = util.krmdup_run_cli(util.KRMDUP_REF, c.text, False, c.args)
        assert rc == 0, err
        assert (q1, q2, qlog) == (o1, o2, ol), name


@pytest.mark.parametrize("name", [n for g in ec.SMALL_GROUPS for n in ec.GROUPS[g]])
def test_plain_restatement_equals_the_oracle(name):
    c = ec.get(name)
    assert c.small
    assert ec.plain(c.text, c.args) == ec.oracle(name), name
