"""Records tests/golden/matrix_bits.json: the sha256 digests that tests/test_gpu_matrix_bits.py compares against.

    python tests/golden/make_matrix_bits.py [output file]

Needs a GPU and the built library.  Run it on the commit whose bits are to be kept (the parent of a change that must not move them),
with the inputs and the digest code of the test itself; the test then asserts the same digests on the changed tree."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_matrix_bits as t  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    got = {case: t.digests(case) for case in t.CASES}
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", out, {k: len(v) for k, v in got.items()})
