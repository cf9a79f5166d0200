"""Generates tests/golden/stitch_golden.json by running THE REFERENCE's read stitching -- bin/flash (FLASH v1.2.11) with one combiner
thread and bin/deal.flash.pl, as the driver chains them (microcket:405-408) -- on seeded synthetic FASTQ (tests/stitchdef.synth) and
on a hand-written edge set.  Per seeded case: SHA-256 of the input, of the program's tab lines kind by kind (combined, uncombined: see stitchdef.by_kind), of deal.flash.pl's
three FASTQ files, the stat line and the program's "Percent combined".  The edge set is stored literally: input records and the
program's output lines.  Runs only where the reference is present.   python tests/golden/make_stitch_golden.py"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import stitchdef as sd  # noqa: E402

REF = os.environ.get("MKT_REFERENCE", "/root/reference")
FLASH = os.path.join(REF, "bin", "flash")
DEAL = os.path.join(REF, "bin", "deal.flash.pl")

CASES = [  # (name, seed, pairs, read_len, flash args, deal.flash.pl args)
    ("mixed", 11, 3000, None, ("-m", "10", "-M", "150"), ()),
    ("len60_over_2_16", 12, 65536 + 300, 60, ("-m", "10", "-M", "150"), ()),
    ("len100", 13, 2000, 100, ("-m", "10", "-M", "150"), ()),
    ("other_args", 14, 2000, None, ("-m", "15", "-M", "80", "-x", "0.1"), ("5", "30")),
]


def run_reference(text, fargs, dargs):
    """-> (tab bytes, ext, cut1, cut2, stat, percent string)"""
    p = subprocess.run([FLASH, "-q", "--interleaved-input", *fargs, "-t", "1", "-To", "-c", "-"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    q = subprocess.run([FLASH, "--interleaved-input", *fargs, "-t", "1", "-To", "-c", "-"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    pct = re.search(rb"Percent combined:\s*([0-9.]+)%", q.stderr + q.stdout).group(1).decode()
    assert q.stdout.endswith(p.stdout)
    with tempfile.TemporaryDirectory(prefix="stg_") as d:
        pre = os.path.join(d, "o")
        r = subprocess.run(["perl", DEAL, "-", pre, *dargs], input=p.stdout, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        files = [open(pre + e, "rb").read() for e in (".ext.fq", ".cut.read1.fq", ".cut.read2.fq", ".stitch.stat")]
    return (p.stdout, *files, pct)


def rc(s):
    return s.encode().translate(sd._COMP)[::-1].decode()


def rnd(seed, n):
    import random
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(n))


def mutate(s, positions, to=None):
    s = list(s)
    for p in positions:
        s[p] = to or {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[s[p]]
    return "".join(s)


def edge_records():
    """[(name, header 1, seq 1, qual 1, header 2, seq 2, qual 2)]"""
    E = []

    def add(name, s1, s2, q1=None, q2=None, h1=None, h2=None):
        E.append((name, h1 or f"{name}/1", s1, q1 or "I" * len(s1), h2 or f"{name}/2", s2, q2 or "I" * len(s2)))

    f = rnd(1, 400)
    s30 = f[:30]
    # tag forms
    add("tag_slash_unc", s30, "T" * 20, h1="a/1", h2="a/2")
    add("tag_slash_words", s30, rc(s30), h1="d/1 x y", h2="d/2 x y")
    add("tag_space", s30, rc(s30), h1="b 1:N:0:ACGT", h2="b 2:N:0:ACGT")
    add("tag_underscore", s30, rc(s30), h1="e_1", h2="e_2")
    add("tag_two_slashes", s30, rc(s30), h1="x/y/1", h2="x/y/2")
    # the two kinds form the tag differently: a '/' inside the header cuts a combined pair's tag only; an uncombined pair's loses
    # nothing but a closing "/1" or "/2"; white space at the header's end goes in both
    for h in ("x/y z", "a/2", "a/3", "q/1/", "/1", "a/1 ", "a b \t", "x/y/1"):
        k = len(E)
        add(f"tag_kind_comb_{k}", s30, rc(s30), h1=h, h2=h)
        add(f"tag_kind_unc_{k}", f[300:350], "T" * 30, h1=h, h2=h)
    add("lower_dot_combined", s30.lower(), rc(s30)[:10] + "." + rc(s30)[11:].lower())
    add("lower_dot_uncombined", f[40:70].lower(), "acgt.nACGTRYacgtac", q2="5" * 18)
    # the shortest reads
    add("len9", f[:9], rc(f[:9]))
    add("len10_overlap10", f[:10], rc(f[:10]))
    add("len10_overlap10_in_longer", f[100:140], rc(f[130:170]))
    add("overlap9_in_longer", f[100:140], rc(f[131:171]))
    # unequal lengths, containment
    add("n1_gt_n2", f[:50], rc(f[30:60]))
    add("n2_gt_n1", f[:30], rc(f[10:60]))
    add("r2_inside_r1", f[:60], rc(f[20:45]))
    add("r2_suffix_of_r1", f[:60], rc(f[35:60]))
    add("r1_inside_r2", f[20:45], rc(f[:60]))
    # eff below m only because of N
    add("n_eff_9", f[200:230], rc(mutate(f[218:248], (1, 5, 9), "N")))
    add("n_eff_10", f[200:230], rc(mutate(f[218:248], (1, 5), "N")))
    add("n_in_read1", mutate(f[200:230], (20, 25), "N"), rc(f[216:246]))
    # full overlaps at and over the cap M = 150
    for n in (150, 151, 160):
        s = f[:n]
        for k in (37, 38, 39, 40):
            add(f"full_{n}_mm{k}", s, rc(mutate(s, range(0, 3 * k, 3))), q1="I" * n, q2="5" * n)
    # ties: homopolymer, dinucleotide repeat
    add("homopolymer", "A" * 40, "T" * 40)
    add("homopolymer_quals", "A" * 40, "T" * 35, q1="".join(chr(35 + k) for k in range(40)), q2="".join(chr(70 - k) for k in range(35)))
    add("dinucleotide", "AC" * 25, "GT" * 20)
    add("dinucleotide_one_mismatch", mutate("AC" * 25, (44,)), "GT" * 20, q2="5" * 40)
    add("trinucleotide", "ACG" * 15, rc("ACG" * 12))
    # a mismatch with equal qualities, with and without N on read 2's side; quality differences 0 and 1
    s = f[250:290]
    add("mismatch_equal_q", s, rc(mutate(s, (12,))))
    add("mismatch_equal_q_n_read2", s, rc(mutate(s, (12,), "N")))
    add("mismatch_equal_q_n_read1", mutate(s, (12,), "N"), rc(s))
    add("both_n", mutate(s, (12,), "N"), rc(mutate(s, (12,), "N")), q1="I" * 40, q2="5" * 40)
    add("qdiff_1_r1_higher", s, rc(mutate(s, (12,))), q1="I" * 40, q2="H" * 40)
    add("qdiff_1_r2_higher", s, rc(mutate(s, (12,))), q1="H" * 40, q2="I" * 40)
    add("qdiff_3", s, rc(mutate(s, (12,))), q1="I" * 40, q2="F" * 40)
    add("n_higher_quality", mutate(s, (12,), "N"), rc(s), q1="I" * 40, q2="5" * 40)
    add("low_quals", s, rc(mutate(s, (3, 30))), q1="#" * 40, q2="!" * 40)
    # deal.flash.pl's min_size + cut_tail edge (46 by default), read 2 shorter; read 2 shorter than cut_tail
    for n in (45, 46, 47):
        add(f"unc_{n}", f[300:300 + n], "T" * 30)
    add("unc_read2_len12", f[300:350], "T" * 12, q2="ABCDEFGHIJKL")
    add("unc_read2_len10", f[300:350], "T" * 10, q2="ABCDEFGHIJ")
    add("unc_read2_len8", f[300:350], "TTTTGGGG", q2="ABCDEFGH")
    add("unc_read2_len4", f[300:350], "TTGG", q2="ABCD")
    return E


def main():
    assert os.path.exists(FLASH) and os.path.exists(DEAL), "the reference's bin/flash and bin/deal.flash.pl are needed"
    out = {"generator": "tests/golden/make_stitch_golden.py", "cases": [], "edges": []}
    for name, seed, pairs, rl, fargs, dargs in CASES:
        text = sd.synth(seed, pairs, rl)
        tab, ext, c1, c2, stat, pct = run_reference(text, fargs, dargs)
        out["cases"].append({"name": name, "seed": seed, "pairs": pairs, "read_len": rl, "flash_args": list(fargs), "deal_args": list(dargs),
                             "input_sha256": sd.sha(text), "tab_combined_sha256": sd.sha(sd.by_kind(tab)[0]), "tab_uncombined_sha256": sd.sha(sd.by_kind(tab)[1]), "ext_sha256": sd.sha(ext), "cut1_sha256": sd.sha(c1),
                             "cut2_sha256": sd.sha(c2), "stat": stat.decode(), "percent": pct})
    for name, h1, s1, q1, h2, s2, q2 in edge_records():      # one pair per run: its own lines, no question of order
        text = f"@{h1}\n{s1}\n+\n{q1}\n@{h2}\n{s2}\n+\n{q2}\n".encode()
        tab, ext, c1, c2, stat, pct = run_reference(text, ("-m", "10", "-M", "150"), ())
        out["edges"].append({"name": name, "input": [h1, s1, q1, h2, s2, q2], "tab": tab.decode(), "ext": ext.decode(), "cut1": c1.decode(),
                             "cut2": c2.decode(), "stat": stat.decode()})
    with open(os.path.join(HERE, "stitch_golden.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("cases:", len(out["cases"]), "edges:", len(out["edges"]))


if __name__ == "__main__":
    main()
