"""Cost of the pair-level concordance (mkt_paircmp_*) on synthetic A and B of 1 M and 10 M lines each (a seeded block of
tests/paircmp_inputs' mixed family, repeated with other read names): the four phase times the library measures with HIP events, the
whole Python call, the wall time of bin/pairscmp on the two files and, with --script, of the reference's Perl script on the same host
and files (its stdout must equal pairscmp's).

    python tools/paircmp_bench.py [--lines 1000000,10000000] [--script /path/to/check.consistency.pl] [--out profiles/paircmp_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import paircmp_inputs as pi  # noqa: E402

BLOCK = 100000


def make_input(lines):
    a, b = pi.make(dict(kind="mixed", seed=99, n=BLOCK))
    a, b = a[a.index(b"\n") + 1:], b.replace(b"#a comment in the middle\n", b"")
    reps = max(1, lines // BLOCK)
    return (b"".join(t.replace(b"K84:", b"K%05d:" % r) for r in range(reps)) for t in (a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", default="1000000,10000000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--script", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import microcket_amd as m
    exe = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairscmp")
    out = []
    for n in (int(x) for x in a.lines.split(",")):
        ta, tb = make_input(n)
        la, lb = ta.count(b"\n"), tb.count(b"\n")
        res = []
        for run in range(a.runs + 1):                    # run 0 warms up
            with m.PairCompare() as pc:
                t0 = time.perf_counter()
                pc.add_a(ta)
                pc.add_b(tb)
                t1 = time.perf_counter()
                info = pc.run()
                dt = time.perf_counter() - t0
                tm = pc.timing_ms()
            if run:
                res.append((dt, t1 - t0, tm))
        dt, tadd, tm = min(res, key=lambda r: r[0])
        dev = sum(tm.values())
        out.append(f"A {la} lines {len(ta) / 1e6:.0f} MB, B {lb} lines {len(tb) / 1e6:.0f} MB: consistent {info['consistent']} discordant {info['discordant']} "
                   f"a_only {info['a_only']} b_only {info['b_only']} host_runs {info['host_runs']} text {info['lines_bytes'] / 1e6:.1f} MB")
        out.append(f"  library, best of {a.runs}: whole call {dt * 1e3:.1f} ms (copying both texts in {tadd * 1e3:.1f} ms); on the device {dev:.1f} ms = "
                   f"{(la + lb) / dev / 1e3:.1f} M lines/s: line index + parse {tm['parse']:.1f}, radix passes {tm['sort']:.1f}, join + counts {tm['join']:.1f}, text {tm['emit']:.1f} ms")
        with tempfile.TemporaryDirectory(prefix="paircmp_") as d:
            fa, fb = os.path.join(d, "a.pairs"), os.path.join(d, "b.pairs")
            for fn, t in ((fa, ta), (fb, tb)):
                with open(fn, "wb") as f:
                    f.write(t)
            best, ours = None, None
            for _ in range(a.runs):
                t0 = time.perf_counter()
                p = subprocess.run([exe, fa, fb, "200", os.path.join(d, "ours.txt")], stdout=subprocess.PIPE)
                w = time.perf_counter() - t0
                assert p.returncode == 0
                best, ours = (w if best is None else min(best, w)), p.stdout
            out.append(f"  bin/pairscmp a.pairs b.pairs 200 inconsistent.txt (files in the page cache), best of {a.runs}: {best:.2f} s wall")
            if a.script:
                t0 = time.perf_counter()
                p = subprocess.run(["perl", a.script, fa, fb, "200", os.path.join(d, "ref.txt")], stdout=subprocess.PIPE, env=dict(os.environ, LC_ALL="C"))
                w = time.perf_counter() - t0
                assert p.returncode == 0 and p.stdout == ours, "the reference's stdout differs"
                out.append(f"  perl check.consistency.pl on the same host and files, one run: {w:.2f} s wall (stdout equal to pairscmp's) = {w / best:.1f} x pairscmp")
            else:
                out.append("  the reference's Perl script was not run (no --script)")
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
