"""Generates tests/golden/stitch_edges_golden.json by running THE REFERENCE's read stitching -- bin/flash (FLASH v1.2.11) with one
combiner thread and bin/deal.flash.pl, as make_stitch_golden.py does -- on the directed families of tests/stitch_edge_cases.py.  Per
family and argument set: SHA-256 of the input, of the program's tab lines kind by kind (stitchdef.by_kind), of deal.flash.pl's three
FASTQ files, and the stat line.  Hashes only.  Runs only where the reference is present.
    python tests/golden/make_stitch_edges_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_stitch_golden as base  # noqa: E402
import stitch_edge_cases as ec  # noqa: E402
import stitchdef as sd  # noqa: E402


def main():
    assert os.path.exists(base.FLASH) and os.path.exists(base.DEAL), "the reference's bin/flash and bin/deal.flash.pl are needed"
    out = {"generator": "tests/golden/make_stitch_edges_golden.py", "families": {}}
    for fam in ec.FAMILIES:
        rows = out["families"][fam] = []
        for name, text, kw in ec.cases(fam):
            tab, ext, c1, c2, stat, _pct = base.run_reference(text, ec.flash_args(kw), ())
            comb, unc = sd.by_kind(tab)
            rows.append({"name": name, "flash_args": ec.flash_args(kw), "pairs": text.count(b"\n") // 8, "input_sha256": sd.sha(text),
                         "tab_combined_sha256": sd.sha(comb), "tab_uncombined_sha256": sd.sha(unc), "ext_sha256": sd.sha(ext),
                         "cut1_sha256": sd.sha(c1), "cut2_sha256": sd.sha(c2), "stat": stat.decode()})
    with open(os.path.join(HERE, "stitch_edges_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print({fam: len(rows) for fam, rows in out["families"].items()})


if __name__ == "__main__":
    main()
