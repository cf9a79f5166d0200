"""Generates tests/golden/krmdup_edges_golden.json by running THE REFERENCE's krmdup / krmdup.pipe (oracle/_ref, built unmodified by
oracle/Makefile) on the directed cases of tests/krmdup_edge_cases.py with each case's arguments.  Per case: SHA-256 of the input, of
<prefix>.read1.fq / .read2.fq, the log text and SHA-256 of the sorted 8-line records of krmdup.pipe's stdout, as in
krmdup_golden.json.  Hashes and logs only.  The cases with lines behind the last whole pair are left out: what the reference does
with those is not what is reproduced.  Runs only where the reference build is present.
    python tests/golden/make_krmdup_edges_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import krmdup_edge_cases as ec  # noqa: E402
import util  # noqa: E402


def main():
    assert os.path.exists(util.KRMDUP_REF) and os.path.exists(util.KRMDUP_PIPE_REF), "oracle/_ref/krmdup.ref missing: make -C oracle"
    out = {"generator": "tests/golden/make_krmdup_edges_golden.py", "cases": []}
    for name in ec.NAMES:
        c = ec.get(name)
        if not c.golden:
            continue
        rc, r1, r2, log, err = util.krmdup_run_cli(util.KRMDUP_REF, c.text, False, c.args)
        assert rc == 0, err
        rcp, so, _, logp, errp = util.krmdup_run_cli(util.KRMDUP_PIPE_REF, c.text, True, c.args)
        assert rcp == 0 and logp == log, errp
        out["cases"].append({"name": name, "args": list(c.args), "pairs": len(ec.lines_of(c.text)[1]) // 8, "input_sha256": util.sha(c.text), "log": log.decode(),
                             "read1_sha256": util.sha(r1), "read2_sha256": util.sha(r2), "pipe_records_sha256": util.sha(b"\n".join(util.fastq_records(so)))})
    with open(os.path.join(HERE, "krmdup_edges_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("cases:", len(out["cases"]))


if __name__ == "__main__":
    main()
