"""Generates tests/golden/ktrim_golden.json by running THE REFERENCE's bin/ktrim (Ktrim 1.6.0) with one thread and -c, as the driver
calls it (microcket:405), on seeded synthetic FASTQ (tests/ktrimdef.synth) and on the directed families of tests/ktrim_cases.py.  Per
seeded case: SHA-256 of the two inputs, of stdout and of the log.  Per directed batch: SHA-256 of the inputs (tests/ktrim_cases.py
rebuilds them) and of stdout, the log literally (the literal stdout of 1444 pairs would be half a megabyte; tests/ktrimdef.py, which
must reproduce it here, shows the lines where a hash differs).  One seeded case also goes through the reference's `ktrim | krmdup.pipe`, its
products hashed (krmdup.pipe's stdout as sorted records: its order depends on its schedule).  Before anything is written, tests/ktrimdef.py must reproduce every case: a definition that disagrees with the
program cannot make a golden.  Runs only where the reference is present.   python tests/golden/make_ktrim_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ktrim_cases as kc  # noqa: E402
import ktrimdef as kd  # noqa: E402
import util  # noqa: E402

REF = os.environ.get("MKT_REFERENCE", "/root/reference")
KTRIM = os.path.join(REF, "bin", "ktrim")
KRMDUP_PIPE = os.path.join(REF, "bin", "krmdup.pipe")

SEEDED = [  # (name, seed, pairs, read_len, kit of the generator, options, argv)
    ("mixed", 21, 3000, None, "illumina", {}, []),
    ("nextera_100", 22, 2000, 100, "nextera", dict(kit="nextera"), ["-k", "nextera"]),
    ("bgi_other_args", 23, 2000, None, "bgi", dict(kit="BGI", min_size=30, min_qual=25, window=3), ["-k", "BGI", "-s", "30", "-q", "25", "-w", "3"]),
    ("transposase_m02", 24, 2000, None, "transposase", dict(kit="Transposase", mismatch=0.2), ["-k", "Transposase", "-m", "0.2"]),
    ("len150_over_4096", 25, 4096 + 300, 150, "illumina", {}, []),
]
PIPE_CASE = ("pipe_2000", 26, 2000, 100)


def run_reference(t1, t2, argv):
    """-> (stdout, log text)"""
    with tempfile.TemporaryDirectory(prefix="ktg_") as d:
        a, b, pre = os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), os.path.join(d, "o")
        open(a, "wb").write(t1)
        open(b, "wb").write(t2)
        p = subprocess.run([KTRIM, "-t", "1", "-o", pre, "-1", a, "-2", b, "-c", *argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout, open(pre + ".trim.log").read()


def run_pipe(t1, t2):
    """the reference's `ktrim -c | krmdup.pipe -i /dev/stdin -o X`: -> (ktrim's stdout, {product name: bytes})"""
    with tempfile.TemporaryDirectory(prefix="ktg_") as d:
        a, b, pre = os.path.join(d, "a.fq"), os.path.join(d, "b.fq"), os.path.join(d, "o")
        open(a, "wb").write(t1)
        open(b, "wb").write(t2)
        k = subprocess.run([KTRIM, "-t", "1", "-o", pre, "-1", a, "-2", b, "-c"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert k.returncode == 0, k.stderr.decode()
        r = subprocess.run([KRMDUP_PIPE, "-i", "/dev/stdin", "-o", pre + ".rmdup"], input=k.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        # krmdup.pipe writes its buckets in an order that depends on its schedule: its stdout is kept in the canonical form of util.fastq_records
        prod = {"stdout_records": b"\n".join(util.fastq_records(r.stdout)), "trim.log": open(pre + ".trim.log", "rb").read()}
        for f in sorted(os.listdir(d)):
            if f.startswith("o.rmdup"):
                prod[f[2:]] = open(os.path.join(d, f), "rb").read()
        return k.stdout, prod


def main():
    assert os.path.exists(KTRIM), "the reference's bin/ktrim is needed"
    out = {"generator": "tests/golden/make_ktrim_golden.py", "cases": [], "batches": [], "pipe": None}
    for name, seed, pairs, rl, kit, opts, argv in SEEDED:
        t1, t2 = kd.synth(seed, pairs, rl, kit)
        so, log = run_reference(t1, t2, argv)
        il, r1, r2, st = kd.trim_stream(t1, t2, **opts)
        assert il == so and kd.log_text(st) == log, f"{name}: tests/ktrimdef.py disagrees with the reference"
        out["cases"].append({"name": name, "seed": seed, "pairs": pairs, "read_len": rl, "kit": kit, "opts": opts, "argv": argv, "input1_sha256": kd.sha(t1),
                             "input2_sha256": kd.sha(t2), "stdout_sha256": kd.sha(so), "read1_sha256": kd.sha(r1), "read2_sha256": kd.sha(r2), "log": log})
    for name, opts, argv, records in kc.all_batches():
        t1, t2 = kc.text_of(records)
        so, log = run_reference(t1, t2, argv)
        il, r1, r2, st = kd.trim_stream(t1, t2, **opts)
        assert il == so and kd.log_text(st) == log, f"{name}: tests/ktrimdef.py disagrees with the reference"
        out["batches"].append({"name": name, "opts": opts, "argv": argv, "pairs": len(records), "input1_sha256": kd.sha(t1), "input2_sha256": kd.sha(t2),
                               "stdout_sha256": kd.sha(so), "log": log})
    name, seed, pairs, rl = PIPE_CASE
    t1, t2 = kd.synth(seed, pairs, rl)
    so, prod = run_pipe(t1, t2)
    assert kd.trim_stream(t1, t2)[0] == so
    out["pipe"] = {"name": name, "seed": seed, "pairs": pairs, "read_len": rl, "input1_sha256": kd.sha(t1), "input2_sha256": kd.sha(t2), "stdout_sha256": kd.sha(so),
                   "products": {k: kd.sha(v) for k, v in prod.items()}}
    with open(os.path.join(HERE, "ktrim_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("cases:", len(out["cases"]), "batches:", len(out["batches"]), "pairs in batches:", sum(b["pairs"] for b in out["batches"]), "pipe products:", sorted(prod))


if __name__ == "__main__":
    main()
