"""Cost of adapter and quality trimming (mkt_trim_*, bin/ktrim) at 150 bp: about ten million synthetic pairs (a seeded
block of tests/ktrimdef.synth pairs, repeated), one warm-up run, then timed runs: the ms per phase that the library measures with HIP
events around its kernels, the whole library call (host copies included), and the wall clock of `bin/ktrim -c > /dev/null` on the
same two files.

    python tools/trim_bench.py [--pairs 10000000] [--out profiles/trim_bench.txt]
    python tools/trim_bench.py --ktrim /path/to/ktrim [--threads 8]     # the CPU program on the same files instead (no GPU used)
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
import ktrimdef as kd  # noqa: E402

BLOCK = 20000
READ_LEN = 150


def make_input(pairs):
    b1, b2 = kd.synth(3000 + READ_LEN, BLOCK, READ_LEN)
    reps = max(1, pairs // BLOCK)
    return b1 * reps, b2 * reps, BLOCK * reps


def wall(cmd, runs):
    best = None
    for _ in range(runs):
        t0 = time.perf_counter()
        p = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t0
        assert p.returncode == 0, (cmd, p.returncode, p.stderr[-300:])
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ktrim", default=None)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    t1, t2, pairs = make_input(a.pairs)
    mb = (len(t1) + len(t2)) / 1e6
    lines = []
    with tempfile.TemporaryDirectory(prefix="trb_") as d:
        f1, f2, pre = os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq"), os.path.join(d, "o")
        with open(f1, "wb") as f:
            f.write(t1)
        with open(f2, "wb") as f:
            f.write(t2)
        if a.ktrim:
            best = wall([a.ktrim, "-t", str(a.threads), "-o", pre, "-1", f1, "-2", f2, "-c"], a.runs)
            lines.append(f"ktrim -t {a.threads} -c  {READ_LEN} bp  {pairs} pairs  {mb:.0f} MB in  best of {a.runs}: {best:.3f} s  {pairs / best / 1e6:.2f} M pairs/s "
                         f"(wall clock of the process, inputs from files, output discarded)")
        else:
            import microcket_amd as m
            res = []
            with m.Trimmer() as t:
                for run in range(a.runs + 1):                    # run 0 warms up
                    t0 = time.perf_counter()
                    t.begin().push(t1, t2, final=True)
                    dt = time.perf_counter() - t0
                    st, tm = t.stats(), t.timing_ms()
                    out_mb = len(t.interleaved()) / 1e6
                    assert st.total == pairs
                    if run:
                        res.append((dt, tm))
            dt, tm = min(res)
            kern = sum(tm)
            lines.append(f"trim  {READ_LEN} bp  {pairs} pairs  {mb:.0f} MB in  {out_mb:.0f} MB interleaved out  adapter {100.0 * st.adapter / st.total:.2f}%  dropped "
                         f"{100.0 * st.dropped / st.total:.2f}%  best of {a.runs}: whole call {dt * 1e3:.1f} ms = {pairs / dt / 1e6:.2f} M pairs/s (host copies in and out "
                         f"included); on the device {kern:.1f} ms = {pairs / kern / 1e3:.2f} M pairs/s: line indexes {tm[0]:.1f}, decisions {tm[1]:.1f}, sizes + scans "
                         f"{tm[2]:.1f}, writing {tm[3]:.1f} ms; host share of the call {100.0 * (1 - kern / (dt * 1e3)):.1f}%")
            exe = os.path.join(os.path.dirname(m.exe_path()), "ktrim")
            best = wall([exe, "-t", str(a.threads), "-o", pre, "-1", f1, "-2", f2, "-c"], a.runs)
            lines.append(f"bin/ktrim -c  {READ_LEN} bp  {pairs} pairs  {mb:.0f} MB in  best of {a.runs}: {best:.3f} s  {pairs / best / 1e6:.2f} M pairs/s "
                         f"(wall clock of the process, inputs from files, output discarded)")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
