"""Makes tests/golden/bamtext_golden.json from the reference's own samtools (1.17).  Run by hand where the reference lies:

    python tests/golden/make_bamtext_golden.py /path/to/reference

No test runs this or reads the reference.  Two kinds of entry, every byte string as base64 of its zlib compression:
  sam/<file>    the alignment lines of tests/golden/edge_*.sam under a small header in the shape of the reference's anno/hg38.sam.header
                (its @HD line and the @SQ lines of the chromosomes the file names): the BAM `samtools view -b --no-PG` wrote, and what
                `view`, `view -h` and `view -H` printed for that BAM
  case/<name>   the accepted streams of tests/bamtext_cases.py (records samtools itself would not write), BGZF-compressed by Python's
                zlib: what `samtools view`, `view -h` and `view -H` printed; the stream itself is rebuilt by the tests and pinned by its SHA-256"""
import base64
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bamtext_cases  # noqa: E402

SAMS = ("edge_aba.sam", "edge_flash.sam", "edge_unc.sam")


def z64(b):
    return base64.b64encode(zlib.compress(b, 9)).decode()


def small_header(ref, lines):
    hdr = open(os.path.join(ref, "anno", "hg38.sam.header"), "rb").read().split(b"\n")
    used = set()
    for ln in lines:
        f = ln.split(b"\t")
        used.update((f[2], f[6]))
    used -= {b"*", b"="}
    out = [h for h in hdr if h.startswith(b"@HD") or (h.startswith(b"@SQ") and h.split(b"\t")[1][3:] in used)]
    known = {h.split(b"\t")[1][3:] for h in out if h.startswith(b"@SQ")}
    out += [b"@SQ\tSN:" + n + b"\tLN:1000000" for n in sorted(used - known)]      # a name the reference's header lacks
    return b"".join(h + b"\n" for h in out)


def views(samtools, path):
    out = {}
    for key, flag in (("view", []), ("view_h", ["-h"]), ("view_H", ["-H"])):
        r = subprocess.run([samtools, "view", "--no-PG"] + flag + [path], capture_output=True)
        assert r.returncode == 0, (path, r.stderr)
        out[key] = z64(r.stdout)
    return out


def main(ref):
    samtools = os.path.join(ref, "bin", "samtools")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in SAMS:
            lines = [ln for ln in open(os.path.join(HERE, name), "rb").read().split(b"\n") if ln and not ln.startswith(b"@")]
            sam = small_header(ref, lines) + b"".join(ln + b"\n" for ln in lines)
            bam = subprocess.run([samtools, "view", "-b", "--no-PG", "-"], input=sam, check=True, capture_output=True).stdout
            path = os.path.join(tmp, "x.bam")
            open(path, "wb").write(bam)
            out["sam/" + name] = dict(views(samtools, path), sam=z64(sam), bam=z64(bam))
        for c in bamtext_cases.accepted():
            path = os.path.join(tmp, "c.bam")
            open(path, "wb").write(bamtext_cases.bgzf(c["raw"]))
            out["case/" + c["name"]] = dict(views(samtools, path), raw_sha256=hashlib.sha256(c["raw"]).hexdigest())
    path = os.path.join(HERE, "bamtext_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
