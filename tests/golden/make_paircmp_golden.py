"""Generates tests/golden/paircmp_golden.json: for seeded pairs of .pairs texts (tests/paircmp_inputs.py makes them again at test time,
so only the parameters are stored) what the reference's benchmarking/check.consistency.pl prints, run here with perl under LC_ALL=C:
its stdout with the two paths replaced by {A} and {B}, and its "inconsistent" file, the I and B lines verbatim (they come in B's file
order) and the A lines sorted (the script walks a Perl hash there).  Nothing of the script is copied.
    python tests/golden/make_paircmp_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import paircmp_inputs as pi                                                       # noqa: E402

SCRIPT = "/root/reference/benchmarking/check.consistency.pl"
ENV = dict(os.environ, LC_ALL="C")


def case(p):
    a, b = pi.make(p["gen"])
    with tempfile.TemporaryDirectory() as d:
        fa, fb, fo = (os.path.join(d, n) for n in ("a.pairs", "b.pairs", "inconsistent.txt"))
        with open(fa, "wb") as f:
            f.write(a)
        with open(fb, "wb") as f:
            f.write(b)
        r = subprocess.run(["perl", SCRIPT, fa, fb, p["dist"] if p["dist"] is not None else "", fo], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        assert r.stderr == b"", (p["name"], r.stderr[:500])                       # a warning means a line outside the pinned domain
        with open(fo, "rb") as f:
            rows = f.read().decode().splitlines(keepends=True)
        stdout = r.stdout.decode().replace(fa, "{A}").replace(fb, "{B}")
    out = dict(p)
    out["lines_a"], out["lines_b"] = a.count(b"\n") + (a[-1:] not in (b"", b"\n")), b.count(b"\n") + (b[-1:] not in (b"", b"\n"))
    out["stdout"] = stdout
    n_ib = sum(1 for x in rows if x[0] in "IB")
    assert all(x[0] == "A" for x in rows[n_ib:]), p["name"]
    out["inconsistent_ib"] = "".join(rows[:n_ib])
    out["inconsistent_a_sorted"] = "".join(sorted(rows[n_ib:]))
    return out


def main():
    cases = [case(p) for p in pi.CASE_PARAMS]
    with open(pi.GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_paircmp_golden.py", "cases": cases}, f, indent=1, sort_keys=True)
    print("cases:", len(cases), "bytes:", os.path.getsize(pi.GOLDEN))


if __name__ == "__main__":
    main()
