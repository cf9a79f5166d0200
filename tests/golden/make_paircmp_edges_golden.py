"""Generates tests/golden/paircmp_edges_golden.json: for every case of tests/paircmp_edge_cases.py that lies inside the pinned domain
(golden: true) what the reference's benchmarking/check.consistency.pl prints, run here with perl under LC_ALL=C and required to warn
about nothing: its stdout whole, with the two paths replaced by {A} and {B}, and of its "inconsistent" file the number of I/B lines
and of A lines, the SHA-256 of the I/B part (it comes in B's file order) and the SHA-256 of the sorted A part (the script walks a Perl
hash there).  The inputs are made again at test time, so none is stored.  Nothing of the script is copied, and
tests/golden/paircmp_golden.json is not touched.
    python tests/golden/make_paircmp_edges_golden.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import paircmp_edge_cases as ec                                                   # noqa: E402

SCRIPT = "/root/reference/benchmarking/check.consistency.pl"
OUT = os.path.join(HERE, "paircmp_edges_golden.json")
ENV = dict(os.environ, LC_ALL="C")
LIMIT = 1 << 20                                                                   # of a committed file


def sha(b):
    return hashlib.sha256(b).hexdigest()


def case(c):
    with tempfile.TemporaryDirectory() as d:
        fa, fb, fo = (os.path.join(d, n) for n in ("a.pairs", "b.pairs", "inconsistent.txt"))
        with open(fa, "wb") as f:
            f.write(c["a"])
        with open(fb, "wb") as f:
            f.write(c["b"])
        r = subprocess.run(["perl", SCRIPT, fa, fb, c["dist"] if c["dist"] is not None else "", fo], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        assert r.stderr == b"", (c["name"], r.stderr[:500])                       # a warning means a line outside the pinned domain
        with open(fo, "rb") as f:
            rows = f.read().splitlines(keepends=True)
        stdout = r.stdout.decode().replace(fa, "{A}").replace(fb, "{B}")
    n_ib = sum(1 for x in rows if x[:1] in (b"I", b"B"))
    assert all(x[:2] == b"A\t" for x in rows[n_ib:]) and all(x[:2] in (b"I\t", b"B\t") for x in rows[:n_ib]), c["name"]
    return dict(name=c["name"], dist=c["dist"], stdout=stdout, lines_ib=n_ib, lines_a=len(rows) - n_ib, sha256_ib=sha(b"".join(rows[:n_ib])),
                sha256_a_sorted=sha(b"".join(sorted(rows[n_ib:]))))


def main():
    cases = [case(c) for c in ec.cases() if c["golden"]]
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_paircmp_edges_golden.py", "cases": cases}, f, indent=1, sort_keys=True)
    size = os.path.getsize(OUT)
    assert size < LIMIT, size
    print("cases:", len(cases), "bytes:", size)


if __name__ == "__main__":
    main()
