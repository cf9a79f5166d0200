"""Generates tests/golden/pairs2matrix_cli_golden.json: what bin/pairs2matrix answers to command lines it refuses before it asks for a
GPU (exit 2 usage, 10 unreadable file, 12 bad value / table / list / track / BEDPE), recorded from the binary of ONE commit so that a
rewrite of the front end can be held to it: per case the argv, the small input files, the exit code and stderr, with the program's
path, the temporary directory and the usage text replaced by {EXE}, {TMP} and {USAGE}.  tests/test_pairs2matrix_cli_host.py replays it.
    python tests/golden/make_pairs2matrix_cli_golden.py <pairs2matrix built from the commit> <that commit's id>
A case that would reach the device (exit 20 without a GPU, 0 with one) does not belong here: the generator refuses it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "pairs2matrix_cli_golden.json")

TABLE = "chr1\t100000\nchr2\t50000\nchrEBV\t5000\n"
PAIRS = "r\tchr1\t10\tchr2\t20\t+\t-\n"
BASE = ["-g", "{TMP}/g.sizes", "-r", "1000", "-o", "{TMP}/o"]
GONE = "{TMP}/missing.pairs"                     # the last thing looked at before the device: a case that passes every check ends here, exit 10

# group, the switches that turn it on, then per option of the group in the order main() looks at them: name, values it accepts
# (None: takes no value), values it refuses (one per distinct message and boundary)
NUM_BAD = ["x", "+1", "nan", "0x1p3", "1e999", "-1", "inf", "1e", " 1", ""]
INT_BAD = ["x", "12345678901", "3000000000", "1.5", "-1", ""]
GROUPS = [
    ("hic", [["--hic"]], [
        ("--hic-level", ["0", "2", "7"], ["x", "-1", "", "99999999999", "1x"]),
        ("--hic-block-bins", ["1", "32767"], ["x"]),
        ("--hic-genome", ["hg38", ""], []),
        ("--hic-norm-label", ["KR"], [])]),
    ("balance", [["--balance"]], [
        ("--ignore-diags", ["0", "2147483647"], INT_BAD),
        ("--min-nnz", ["0", "10"], ["x"]),
        ("--min-count", ["0", ".5", "1e3", "2E+1"], NUM_BAD),
        ("--mad-max", ["0", "5."], ["x"]),
        ("--tol", ["1e-5"], ["x"]),
        ("--max-iters", ["1", "200"], ["0", "x"])]),
    ("loops", [["--loops"]], [
        ("--loop-peak", ["1"], ["x"]),
        ("--loop-window", ["3"], ["x"]),
        ("--loop-window-max", ["20"], ["x"]),
        ("--loop-min-ll-count", ["0"], ["x"]),
        ("--loop-min-dist", ["0"], ["x"]),
        ("--loop-max-dist", ["0"], ["x"]),
        ("--loop-fdr", ["0.5", "1e-9"], ["0", "1", "x"]),
        ("--loop-cluster-radius", ["0"], ["x"])]),
    ("eigs", [["--eigs"]], [
        ("--eigs-n", ["1", "4"], ["0", "5", "x"]),
        ("--eigs-ignore-diags", ["0"], ["x"]),
        ("--eigs-min-good", ["0"], ["x"]),
        ("--eigs-max-iters", ["0"], ["x"]),
        ("--eigs-tol", ["0.5"], ["0", "1", "x"]),
        ("--eigs-clip", ["0"], ["x"]),
        ("--eigs-track", [], [])]),
    ("insulation", [["--insulation", "5000"]], [
        ("--ins-ignore-diags", ["0"], ["x"]),
        ("--ins-min-frac-valid", ["0", "1"], ["1.5", "x"]),
        ("--ins-min-strength", ["0"], ["x"])]),
    ("pileup", [["--apa"], ["--pileup", "{TMP}/f.bedpe"]], [
        ("--pile-flank", ["1", "32"], ["0", "33", "x"]),
        ("--pile-corner", ["1"], ["0", "x"]),
        ("--pile-kind", ["balanced", "oe", "oe-smooth"], ["x"]),
        ("--pile-edges", None, [])]),
    ("saddle", [["--saddle"]], [
        ("--saddle-groups", ["2", "64"], ["1", "65", "x"]),
        ("--saddle-trim", ["0,0", "5000,4999"], ["5000,5000", "5", "x,1", "1,x", "1,2,3"]),
        ("--saddle-contact", ["cis", "trans"], ["x"]),
        ("--saddle-kind", ["oe", "oe-smooth"], ["balanced"]),
        ("--saddle-min-dist", ["0", "2000"], ["x"]),
        ("--saddle-max-dist", ["0", "3000"], ["x"]),
        ("--saddle-corner", ["1"], ["0", "x"])]),
    ("scc", [["--compare", "{TMP}/missing2.pairs"]], [
        ("--scc-h", ["0", "16"], ["17", "x"]),
        ("--scc-min-dist", ["0", "1000"], ["x"]),
        ("--scc-max-dist", ["0", "4000"], ["x"]),
        ("--scc-weighting", ["n", "var"], ["x"])]),
    ("viewpoint", [["--viewpoint", "chr1"], ["--ebv"]], [
        ("--vp-bin", ["1"], ["0", "x"]),
        ("--vp-partner-bin", ["1"], ["0"]),
        ("--vp-track-bin", ["1"], ["0"]),
        ("--vp-min-count", ["1"], ["0"]),
        ("--vp-hotspot", ["0", "0.99"], ["1", "x"]),
        ("--vp-partners", ["chr2"], [""]),
        ("--vp-second-side", None, [])]),
]
SWITCH_WITH_VALUE = ["-g", "-r", "-o", "--insulation", "--pileup", "--compare", "--viewpoint"]

CASES = []


def case(group, name, args, files=None, base=BASE, inputs=(GONE,)):
    CASES.append({"group": group, "name": name, "argv": list(base) + list(args) + list(inputs), "files": dict({"g.sizes": TABLE}, **(files or {}))})


def option_cases():
    for _, _, opts in GROUPS:
        for opt, good, _ in opts:
            if good is not None:
                case("missing value", opt + " last", [opt], inputs=())
    for opt in SWITCH_WITH_VALUE:
        case("missing value", opt + " last", [opt], inputs=())
    case("missing value", "after an error of an earlier group", ["--hic-level", "1", "--tol"], inputs=())
    case("unknown option", "-x", ["-x"])
    case("unknown option", "--hic-levels", ["--hic", "--hic-levels", "1"])
    case("unknown option", "a lone - is a file name", ["--compare", "{TMP}/missing2.pairs"], inputs=("-",))
    case("unknown option", "no -g", [], base=BASE[2:])
    case("unknown option", "no -r", [], base=BASE[:2] + BASE[4:])
    case("unknown option", "no -o", [], base=BASE[:4])
    case("unknown option", "nothing", [], base=[], inputs=())
    case("unknown option", "an option's value may look like an option", ["--viewpoint", "--ebv"])
    for g, switches, opts in GROUPS:
        val = lambda opt, good: [opt] if good is None else [opt, good[0] if good else "{TMP}/t.bed"]
        for opt, good, _ in opts:
            case("needs its switch", opt, val(opt, good))
        for (a, ga, _), (b, gb, _) in zip(opts, opts[1:]):                  # the earlier one of the group is named, wherever it stands
            case("needs its switch", f"{b} {a}", val(b, gb) + val(a, ga))
        for sw in switches:                                                 # every accepted value at once, the last given wins
            args = list(sw)
            for opt, good, bad in opts:
                if good is None:
                    args += [opt]
                for v in (bad[:1] if bad else []) + (good or []):
                    args += [opt, v]
            case("accepted", f"{g} via {sw[0]}", args, files={"f.bedpe": ""})
        with_bad = [(opt, bad) for opt, _, bad in opts if bad]
        for opt, bad in with_bad:
            for v in bad:
                case("bad value", f"{opt} {v!r}", switches[0] + [opt, v])
        for (a, ba), (b, bb) in zip(with_bad, with_bad[1:]):
            case("bad value", f"{b} and {a}: the earlier one of the group", switches[-1] + [b, bb[-1], a, ba[0]])
    case("bad value", "--pile-flank 0 with --pileup", ["--pileup", "{TMP}/f.bedpe", "--pile-flank", "0"])
    case("bad value", "--vp-bin 0 with --ebv", ["--ebv", "--vp-bin", "0"])
    case("needs its switch", "--pile-edges beside --expected", ["--expected", "--loops", "--pile-edges"])
    case("needs its switch", "--vp-bin beside --hic", ["--hic", "--vp-bin", "5"])


def cross_cases():
    c = lambda name, args, **kw: case("cross-option", name, args, **kw)
    c("--loop-window equal to --loop-peak", ["--loops", "--loop-window", "2", "--loop-peak", "2"])
    c("--loop-window below the default peak, with --apa", ["--apa", "--loop-window", "1"])
    c("--loop-window-max 21", ["--loops", "--loop-window-max", "21"])
    c("--loop-window-max below --loop-window", ["--loops", "--loop-window-max", "4", "--loop-window", "6"])
    c("--loop-window-max equal to --loop-window is fine", ["--loops", "--loop-window-max", "6", "--loop-window", "6"])
    c("--pile-corner above --pile-flank", ["--apa", "--pile-corner", "5", "--pile-flank", "4"])
    c("--pile-corner above the default flank", ["--pileup", "{TMP}/f.bedpe", "--pile-corner", "11"], files={"f.bedpe": ""})
    c("the default corner inside a small --pile-flank is fine", ["--pileup", "{TMP}/f.bedpe", "--pile-flank", "3"], files={"f.bedpe": ""})
    c("--saddle-corner above half the default groups", ["--saddle", "--saddle-corner", "26"])
    c("--saddle-corner half the default groups is fine", ["--saddle", "--saddle-corner", "25"])
    c("--saddle-corner above half of --saddle-groups", ["--saddle", "--saddle-groups", "5", "--saddle-corner", "3"])
    c("the default --saddle-corner above half of --saddle-groups 2", ["--saddle", "--saddle-groups", "2"])
    c("--saddle-max-dist below --saddle-min-dist", ["--saddle", "--saddle-min-dist", "5000", "--saddle-max-dist", "1000"])
    c("--saddle-max-dist 0 below --saddle-min-dist is fine", ["--saddle", "--saddle-min-dist", "5000", "--saddle-max-dist", "0"])
    c("--scc-max-dist below --scc-min-dist", ["--compare", "{TMP}/in2.pairs", "--scc-min-dist", "5000", "--scc-max-dist", "1000"], files={"in2.pairs": PAIRS})
    for lst, what in (("1000,2000,3000,4000,5000", "five windows"), ("2000,1000", "not ascending"), ("1000,1000", "twice"), ("0", "zero"), ("x", "no number"), ("", "empty"),
                      ("1000,", "trailing comma")):
        c("--insulation list: " + what, ["--insulation", lst])
    c("--insulation window no multiple of the second -r", ["--insulation", "2000"], base=BASE[:3] + ["1000,300"] + BASE[4:])
    c("--insulation window of more than 1024 bins", ["--insulation", "1025000"])
    c("--insulation window of 1024 bins is fine", ["--insulation", "1024000"])
    two = BASE[:3] + ["1000,300"] + BASE[4:]
    c("--saddle-min-dist no multiple of the second -r", ["--saddle", "--saddle-min-dist", "2000"], base=two)
    c("--saddle-max-dist no multiple of the second -r", ["--saddle", "--saddle-max-dist", "2000"], base=two)
    c("--scc-min-dist no multiple of the second -r", ["--compare", "{TMP}/in2.pairs", "--scc-min-dist", "2000"], base=two, files={"in2.pairs": PAIRS})
    c("--scc-max-dist no multiple of the second -r", ["--compare", "{TMP}/in2.pairs", "--scc-max-dist", "2000"], base=two, files={"in2.pairs": PAIRS})
    c("--eigs-track with two resolutions", ["--eigs", "--eigs-track", "{TMP}/t.bed"], base=two, files={"t.bed": ""})
    c("--viewpoint with a name that is not in the table", ["--viewpoint", "chrZ"])
    c("--ebv without chrEBV", ["--ebv"], files={"g.sizes": "chr1\t100000\nchr2\t50000\n"})
    c("--vp-partners that keeps nothing", ["--viewpoint", "chr1", "--vp-partners", "nomatch"])
    c("--vp-partners that keeps only the viewpoint", ["--viewpoint", "chr1", "--vp-partners", "chr1"])
    c("--ebv with a table of chrEBV and names the preset leaves out", ["--ebv"], files={"g.sizes": "chrX\t100\nchrEBV\t5000\n"})
    c("an invalid regular expression", ["--viewpoint", "chr1", "--vp-partners", "("])
    c("a resolution giving 2^32 bins", [], base=BASE[:3] + ["1"] + BASE[4:], files={"g.sizes": "a\t4294967295\nb\t4294967295\n"})
    for rl in ("0", "5000,abc", "5000,,100", "", "100,100", ",".join(str(k + 1) for k in range(17)), "4294967296", "12345678901"):
        c(f"-r {rl!r}", [], base=BASE[:3] + [rl] + BASE[4:])


def file_cases():
    t = lambda name, text: case("table", name, [], files={"g.sizes": text})
    t("a line without a length", "chr1\t1000\nchr2\nchr3\t10\n")
    t("a duplicate name", "chr1\t1000\nchr2\t10\nchr1\t5\n")
    t("an empty table", "")
    t("only comments and empty lines", "#chr1\t5\n\n")
    t("a name of 64 bytes", "x" * 64 + "\t100\n")
    t("a name of 63 bytes is fine", "x" * 63 + "\t100\n")
    t("an empty name", "\t100\n")
    t("a length of 2^32", "chr1\t4294967296\n")
    t("a length with a letter", "chr1\t10x\n")
    t("CR LF lines and a third column are fine", "chr1\t1000\textra\r\nchr2\t10\r\n")
    k = lambda name, text: case("track", name, ["--eigs", "--eigs-track", "{TMP}/t.bed"], files={"g.sizes": "chrA\t2500\nchrB\t1000\n", "t.bed": text})
    rows = ["chrA\t0\t1000\t1", "chrA\t1000\t2000\t-0.5", "chrA\t2000\t2500\tnan", "chrB\t0\t1000\t1e-3"]
    k("a matching track is fine", "\n".join(rows) + "\n")
    k("CR LF and no final newline are fine", "\r\n".join(rows))
    k("too few rows", "\n".join(rows[:3]) + "\n")
    k("too many rows", "\n".join(rows + rows[:1]) + "\n")
    k("a wrong bin", "\n".join(rows[:2] + ["chrA\t2000\t3000\t1"] + rows[3:]) + "\n")
    k("a value that is not a number", "\n".join(rows[:1] + ["chrA\t1000\t2000\tup"] + rows[2:]) + "\n")
    k("an empty value", "\n".join(rows[:3] + ["chrB\t0\t1000\t"]) + "\n")
    k("an empty file", "")
    b = lambda name, text: case("bedpe", name, ["--pileup", "{TMP}/f.bedpe"], files={"f.bedpe": text})
    b("five columns", "chr1\t10\t20\tchr2\t30\n")
    b("a bad position", "chr1\t10\t2x\tchr2\t30\t40\n")
    b("an empty position", "chr1\t\t20\tchr2\t30\t40\n")
    b("a position of 19 digits", "chr1\t1\t1000000000000000000\tchr2\t30\t40\n")
    b("an end before its start", "#c\n\nchr1\t10\t20\tchr2\t40\t30\n")
    b("an unknown chromosome", "chr1\t10\t20\tchr9\t30\t40\n")
    b("a midpoint past the end", "chr1\t10\t20\tchr2\t50000\t50000\n")
    b("comments, empty lines, CR LF and more columns are fine", "#c\n\nchr1\t10\t20\tchr2\t49999\t50000\tx\ty\r\nchr2\t1\t1\tchr1\t5\t6")
    u = lambda name, args, **kw: case("unreadable", name, args, **kw)
    u("table", [], base=["-g", "{TMP}/missing.sizes"] + BASE[2:])
    u("track", ["--eigs", "--eigs-track", "{TMP}/missing.bed"])
    u("pileup", ["--pileup", "{TMP}/missing.bedpe"])
    u("input", [], inputs=("{TMP}/in.pairs", GONE), files={"in.pairs": PAIRS})
    u("compare", ["--compare", "{TMP}/missing2.pairs"], inputs=("{TMP}/in.pairs",), files={"in.pairs": PAIRS})
    u("a directory as the table", [], base=["-g", "{TMP}"] + BASE[2:])


def precedence_cases():
    """two errors of different groups in one command line, the later one first where the order of the arguments allows it"""
    p = lambda name, args, **kw: case("precedence", name, args, **kw)
    badres = BASE[:3] + ["x"] + BASE[4:]
    two = BASE[:3] + ["1000,300"] + BASE[4:]
    p("hic before balance", ["--balance", "--tol", "x", "--hic-level", "1"])
    p("balance before loops", ["--loop-peak", "1", "--balance", "--tol", "x"])
    p("loops before eigs", ["--eigs-n", "1", "--loops", "--loop-fdr", "2"])
    p("the loop windows before eigs", ["--eigs", "--eigs-n", "9", "--loops", "--loop-window", "1"])
    p("eigs before the insulation sub-options", ["--ins-ignore-diags", "1", "--eigs", "--eigs-tol", "2"])
    p("the insulation sub-options before pileup", ["--apa", "--pile-flank", "99", "--ins-min-strength", "1"])
    p("pileup before saddle", ["--saddle", "--saddle-kind", "x", "--pile-edges"])
    p("the pileup corner before saddle", ["--saddle", "--saddle-groups", "1", "--apa", "--pile-corner", "11"])
    p("saddle before scc", ["--scc-h", "1", "--saddle", "--saddle-contact", "x"])
    p("the saddle distances before scc", ["--compare", "{TMP}/missing2.pairs", "--scc-h", "99", "--saddle", "--saddle-min-dist", "9", "--saddle-max-dist", "3"])
    p("scc before viewpoint", ["--vp-bin", "5", "--compare", "{TMP}/missing2.pairs", "--scc-weighting", "x"])
    p("the scc distances before viewpoint", ["--ebv", "--vp-hotspot", "2", "--compare", "{TMP}/missing2.pairs", "--scc-min-dist", "9", "--scc-max-dist", "3"])
    p("viewpoint before the insulation list", ["--insulation", "x", "--ebv", "--vp-partners", ""])
    p("the insulation list before the table", ["--insulation", "2,1"], base=["-g", "{TMP}/missing.sizes"] + BASE[2:])
    p("the table before the viewpoint name", ["--viewpoint", "chrZ"], files={"g.sizes": "chr1\n"})
    p("the viewpoint name before -r", ["--viewpoint", "chrZ"], base=badres)
    p("the regular expression before -r", ["--viewpoint", "chr1", "--vp-partners", "("], base=badres)
    p("a bad table before a bad -r", [], base=badres, files={"g.sizes": "chr1\n"})
    p("-r before --eigs-track's single resolution", ["--eigs", "--eigs-track", "{TMP}/missing.bed"], base=BASE[:3] + ["1000,1000"] + BASE[4:])
    p("the insulation multiple before the saddle multiple", ["--saddle", "--saddle-min-dist", "2000", "--insulation", "2000"], base=two)
    p("the saddle multiple before the scc multiple", ["--compare", "{TMP}/missing2.pairs", "--scc-min-dist", "2000", "--saddle", "--saddle-max-dist", "2000"], base=two)
    p("the multiples a resolution at a time, not an option at a time", ["--saddle", "--saddle-min-dist", "1000", "--saddle-max-dist", "1200"], base=BASE[:3] + ["500,300"] + BASE[4:])
    p("the scc multiple before --eigs-track's single resolution", ["--eigs", "--eigs-track", "{TMP}/missing.bed", "--compare", "{TMP}/missing2.pairs", "--scc-max-dist", "2000"], base=two)
    p("the track file before the bin limit", ["--eigs", "--eigs-track", "{TMP}/missing.bed"], base=BASE[:3] + ["1"] + BASE[4:], files={"g.sizes": "a\t4294967295\nb\t4294967295\n"})
    p("the bin limit before the pileup file", ["--pileup", "{TMP}/missing.bedpe"], base=BASE[:3] + ["1"] + BASE[4:], files={"g.sizes": "a\t4294967295\nb\t4294967295\n"})
    p("a bad BEDPE before a missing input file", ["--pileup", "{TMP}/f.bedpe"], files={"f.bedpe": "chr1\t1\n"})
    p("a missing input file before a missing compare file", ["--compare", "{TMP}/missing2.pairs"])
    p("a missing value before everything", ["--hic-level", "1", "--balance", "--tol", "x", "--eigs-n"], inputs=())
    p("an unknown option before everything", ["--hic-level", "1", "-x"])
    p("no prefix before a sub-option without its switch", ["--hic-level", "1"], base=BASE[:4])


def record(exe, c):
    with tempfile.TemporaryDirectory() as d:
        for fn, text in c["files"].items():
            with open(os.path.join(d, fn), "wb") as f:
                f.write(text.encode())
        r = subprocess.run([exe] + [a.replace("{TMP}", d) for a in c["argv"]], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        left = sorted(set(os.listdir(d)) - set(c["files"]))
    assert r.returncode in (2, 10, 12), (c["name"], r.returncode, r.stderr)      # anything else reached the device, or crashed
    assert r.stdout == b"" and not left, (c["name"], r.stdout, left)
    return r.returncode, r.stderr.decode().replace(exe, "{EXE}").replace(d, "{TMP}")


def main():
    exe, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    usage = subprocess.run([exe], stdin=subprocess.DEVNULL, stderr=subprocess.PIPE).stderr.decode().replace(exe, "{EXE}")
    assert usage.startswith("Usage: {EXE} ") and usage.count("\n") == 14
    option_cases(); cross_cases(); file_cases(); precedence_cases()
    assert len({(c["group"], c["name"]) for c in CASES}) == len(CASES)
    for c in CASES:
        c["exit"], err = record(exe, c)
        c["stderr"] = err.replace(usage, "{USAGE}")
    with open(GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_pairs2matrix_cli_golden.py", "recorded_from": commit, "usage": usage, "cases": CASES}, f, indent=1, sort_keys=True)
    by = {}
    for c in CASES:
        by[c["exit"]] = by.get(c["exit"], 0) + 1
    print("cases:", len(CASES), "by exit code:", by, "bytes:", os.path.getsize(GOLDEN))


if __name__ == "__main__":
    main()
