"""Makes tests/golden/px2_golden.json from the reference's own binaries.  Run by hand where the reference lies:

    python tests/make_px2_golden.py /path/to/reference

No test runs this or reads the reference.  Per case of px2_inputs.py: `bgzip -c | pairix` indexes the text; the index is parsed with
px2def.parse_px2 and every virtual offset replaced by the offset in the text it points to (px2def.to_text_offsets, through the block table
of bgzip's file); `pairix file.gz REGION` answers the case's regions (a pair that
the file does not hold: exit status 1, no lines), `pairix -n` counts the lines.  For the inputs this project
refuses, what the reference did (exit status, first line of stderr, whether it left an index)."""
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import px2_inputs  # noqa: E402
import px2def  # noqa: E402


def main(ref):
    bgzip, pairix = os.path.join(ref, "bin", "bgzip"), os.path.join(ref, "bin", "pairix")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for c in px2_inputs.cases():
            plain, gzp = os.path.join(d, "in.pairs"), os.path.join(d, "in.pairs.gz")
            with open(plain, "wb") as f:
                f.write(c["text"])
            gz = subprocess.run([bgzip, "-c", plain], check=True, capture_output=True).stdout
            with open(gzp, "wb") as f:
                f.write(gz)
            if os.path.exists(gzp + ".px2"):
                os.remove(gzp + ".px2")
            r = subprocess.run([pairix, "-f", gzp], capture_output=True)
            g = {"reference_status": r.returncode, "reference_stderr": r.stderr.decode("latin-1").split("\n")[0], "reference_wrote_index": os.path.exists(gzp + ".px2")}
            if c["refused"] is None:
                assert r.returncode == 0 and g["reference_wrote_index"], (c["name"], r.stderr)
                assert px2def.bgzf_inflate(gz) == c["text"]
                blocks = px2def.bgzf_blocks(gz)
                with open(gzp + ".px2", "rb") as f:
                    ix = px2def.parse_px2(f.read())
                g["index"] = px2def.to_text_offsets(ix, blocks, len(gz))
                g["bgzip_block_starts"] = [b[2] for b in blocks]
                g["queries"] = {q: subprocess.run([pairix, gzp, q], capture_output=True).stdout.decode("latin-1").split("\n")[:-1] for q in c["regions"]}
                g["n"] = int(subprocess.run([pairix, "-n", gzp], check=True, capture_output=True).stdout)
            out[c["name"]] = g
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "px2_golden.json")
    with open(path, "w") as f:
        f.write("{\n")                                  # a line per case and per field of a case, so that a change shows as a few lines
        for i, name in enumerate(sorted(out)):
            f.write(" %s: {\n" % json.dumps(name))
            f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(out[name][k], separators=(",", ":"), sort_keys=True)) for k in sorted(out[name])))
            f.write("\n }%s\n" % ("," if i + 1 < len(out) else ""))
        f.write("}\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
