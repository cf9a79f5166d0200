"""Makes tests/golden/pairsquery_golden.json from the reference's own binaries.  Run by hand where the reference lies:

    python tests/make_pairsquery_golden.py /path/to/reference

No test runs this or reads the reference.  Per accepted case of px2_inputs.py: `bgzip -c | pairix` indexes the text, then pairix answers
what pairsquerydef.requests asks: single regions (a star on either side, b = e, b = 0, commas, ends around 2^30, an absent pair), regions
with -a (a flipped pair, present and absent), one batch of overlapping and repeated regions on the command line and the same through -L,
and -l.  An answer of more than 40 lines is recorded as its line count and the SHA-256 of pairix's stdout.  Exit statuses are recorded as data.  "_refused" records what pairix did with the regions this project refuses."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairsquerydef  # noqa: E402
import px2_inputs  # noqa: E402


def main(ref):
    bgzip, pairix = os.path.join(ref, "bin", "bgzip"), os.path.join(ref, "bin", "pairix")

    def ask(*args):
        r = subprocess.run([pairix, *args], capture_output=True)
        lines = r.stdout.decode("latin-1").split("\n")[:-1]
        if len(lines) <= 40:
            return {"lines": lines, "status": r.returncode}
        return {"n": len(lines), "sha256": hashlib.sha256(r.stdout).hexdigest(), "status": r.returncode}      # a long answer: its hash

    out = {}
    with tempfile.TemporaryDirectory() as d:
        gzp, lst = os.path.join(d, "in.pairs.gz"), os.path.join(d, "regions.txt")
        for c in px2_inputs.accepted():
            plain = os.path.join(d, "in.pairs")
            with open(plain, "wb") as f:
                f.write(c["text"])
            with open(gzp, "wb") as f:
                f.write(subprocess.run([bgzip, "-c", plain], check=True, capture_output=True).stdout)
            subprocess.run([pairix, "-f", gzp], check=True, capture_output=True)
            rq = pairsquerydef.requests(c)
            with open(lst, "w") as f:
                f.write("".join(q + "\n" for q in rq["batch"]))
            g = {"single": {q: ask(gzp, q) for q in rq["single"]}, "autoflip": {q: ask("-a", gzp, q) for q in rq["autoflip"]},
                 "batch": dict(ask(gzp, *rq["batch"]), regions=rq["batch"]), "L": ask("-L", gzp, lst), "l": ask("-l", gzp)}
            if c["name"] == "many_pairs":
                out["_refused"] = {q: ask(gzp, q) for q in pairsquerydef.REFUSED}
            out[c["name"]] = g
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairsquery_golden.json")
    with open(path, "w") as f:
        f.write("{\n")                                  # a line per case and per field of a case, so that a change shows as a few lines
        for i, name in enumerate(sorted(out)):
            f.write(" %s: {\n" % json.dumps(name))
            f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(out[name][k], separators=(",", ":"), sort_keys=True)) for k in sorted(out[name])))
            f.write("\n }%s\n" % ("," if i + 1 < len(out) else ""))
        f.write("}\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
