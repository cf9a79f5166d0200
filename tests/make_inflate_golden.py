"""Makes tests/golden/inflate_golden.json from the reference's own bgzip.  Run by hand where the reference lies:

    python tests/make_inflate_golden.py /path/to/reference

No test runs this or reads the reference.  For the px2_inputs cases `blocks_many_bins` and `many_pairs`: what `bgzip -l 1`, `-l 6`
and `-l 9` wrote, as base64 (a foreign writer's block cuts, code choices and EOF block), with the SHA-256 of the text it stands for."""
import base64
import hashlib
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import px2_inputs  # noqa: E402
import px2def  # noqa: E402

CASES = ("blocks_many_bins", "many_pairs")
LEVELS = (1, 6, 9)


def main(ref):
    bgzip = os.path.join(ref, "bin", "bgzip")
    out = {}
    for name in CASES:
        text = px2_inputs.case(name)["text"]
        for level in LEVELS:
            gz = subprocess.run([bgzip, "-l", str(level), "-c"], input=text, check=True, capture_output=True).stdout
            assert px2def.bgzf_inflate(gz) == text and px2def.bgzf_blocks(gz)
            out["%s/l%d" % (name, level)] = {"case": name, "level": level, "text_sha256": hashlib.sha256(text).hexdigest(), "gz_base64": base64.b64encode(gz).decode()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inflate_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(out), "files")


if __name__ == "__main__":
    main(sys.argv[1])
