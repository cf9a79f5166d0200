"""Generates tests/golden/ref_build_golden.json by running THE REFERENCE's builds (oracle/_ref/sam2pairs.ref, oracle/_ref/krmdup.ref,
compiled unmodified by oracle/Makefile) on the exact inputs of tests/test_oracle.py::test_oracle_matches_reference_build,
::test_quirk_q2_across_batches and tests/test_krmdup.py::test_krmdup_oracle_matches_reference_build, so that those tests pin the
restatement against the reference's results also where the reference build is absent.  Per sam2pairs case: the .log verbatim and
SHA-256 of the canonical (LANG=C sorted) .pairs / .sam; per krmdup case: the log and SHA-256 of <prefix>.read1.fq / .read2.fq.
    python tests/golden/make_ref_build_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import util  # noqa: E402
import test_krmdup  # noqa: E402
import test_oracle  # noqa: E402


def main():
    assert util.have_ref() and os.path.exists(util.KRMDUP_REF), "oracle/_ref missing: make -C oracle ref"
    out = {"generator": "tests/golden/make_ref_build_golden.py", "sam2pairs": {}, "quirk_q2": {}, "krmdup": {}}
    for profile, seed, groups, modes in test_oracle.REF_BUILD_INPUTS:
        text = util.synth(profile, seed, groups)
        for mode in modes:
            for (T, ratio, mapq, sam) in test_oracle.REF_BUILD_GRID:
                rc, rp, rs, rl, err = util.ref_run(text, mode, T, ratio, mapq, sam)
                assert rc == 0, err
                out["sam2pairs"][test_oracle.ref_key(profile, seed, groups, mode, T, ratio, mapq, sam)] = {
                    "input_sha256": util.sha(text), "log": rl.decode(),
                    "pairs_sha256": util.sha(util.canon(rp)), "sam_sha256": util.sha(util.canon(rs))}
    text = test_oracle.q2_input()
    for T in test_oracle.Q2_THREADS:
        rc, rp, rs, rl, err = util.ref_run(text, "unc", T, 0.5, 0, False)
        assert rc == 0, err
        out["quirk_q2"][str(T)] = {"input_sha256": util.sha(text), "log": rl.decode(), "pairs_sha256": util.sha(util.canon(rp))}
    for seed, pairs, rl, args in test_krmdup.REF_BUILD_CASES:
        text = util.synth_fastq(seed, pairs, rl)
        rc, r1, r2, log, err = util.krmdup_run_cli(util.KRMDUP_REF, text, False, args)
        assert rc == 0, err
        out["krmdup"][str(seed)] = {"input_sha256": util.sha(text), "log": log.decode(), "read1_sha256": util.sha(r1), "read2_sha256": util.sha(r2)}
    with open(os.path.join(HERE, "ref_build_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("cases:", len(out["sam2pairs"]), len(out["quirk_q2"]), len(out["krmdup"]))


if __name__ == "__main__":
    main()
