"""Generates tests/golden/viewpoint_golden.json: for seeded .pairs text (tests/viewpoint_inputs.py makes it again at test time, so
only the parameters are stored) the three texts of the reference's viewpoint analysis, run here with perl under LC_ALL=C on
/root/reference/util/analyze.EBV/calc.inter.EBV.matrix.and.circos.pl (stdout: the viewpoint bedgraph, stderr: the Circos links) and
calc.loop2EBV.pl | sort -k1,1 -k2,2n (the partner bedgraph), as analyze.EBV.sh chains them.  Nothing of the scripts is copied.
    python tests/golden/make_viewpoint_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import viewpoint_inputs as vi                                                     # noqa: E402

DIR = "/root/reference/util/analyze.EBV"
ENV = dict(os.environ, LC_ALL="C")


def num(x):
    return repr(x) if isinstance(x, float) else str(x)


def case(p):
    text = vi.make(p["gen"])
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "in.pairs")
        with open(fn, "wb") as f:
            f.write(text)
        a = subprocess.run(["perl", os.path.join(DIR, "calc.inter.EBV.matrix.and.circos.pl"), fn, num(p["vbin"]), num(p["pbin"]), num(p["ratio"])],
                           env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
        b = subprocess.run(["perl", os.path.join(DIR, "calc.loop2EBV.pl"), fn, num(p["track_bin"]), num(p["min_count"])], env=ENV, stdout=subprocess.PIPE, check=True)
        s = subprocess.run(["sort", "-k1,1", "-k2,2n"], input=b.stdout, env=ENV, stdout=subprocess.PIPE, check=True)
    out = dict(p)
    out["lines"] = text.count(b"\n")
    out["bedgraph"], out["links"], out["partners"] = a.stdout.decode(), a.stderr.decode(), s.stdout.decode()
    assert out["bedgraph"] and out["links"] and "uninitialized" not in out["links"], p["name"]
    return out


def main():
    cases = [case(p) for p in vi.CASE_PARAMS]
    with open(vi.GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_viewpoint_golden.py", "viewpoint": vi.VIEWPOINT, "partners": vi.PARTNER_RE, "cases": cases}, f, indent=1, sort_keys=True)
    print("cases:", len(cases), "bytes:", os.path.getsize(vi.GOLDEN))


if __name__ == "__main__":
    main()
