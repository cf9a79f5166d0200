"""Cost of the resident read stitching (mkt_stitch_*) at 100 and 150 bp: a few million synthetic pairs (a seeded block
of tests/stitchdef.synth pairs, repeated), one warm-up run, then timed runs; pairs/s over the whole call (host copies included) and
the ms per phase that the library measures with HIP events around its kernels.

    python tools/stitch_bench.py [--pairs 2000000] [--out profiles/stitch_bench.txt]
    python tools/stitch_bench.py --flash /path/to/flash [--threads 16]     # the CPU program on the same input instead (no GPU used)
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stitchdef as sd  # noqa: E402

BLOCK = 20000


def make_input(read_len, pairs):
    block = sd.synth(1000 + read_len, BLOCK, read_len)
    reps = max(1, pairs // BLOCK)
    return block * reps, BLOCK * reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--flash", default=None)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    lines = []
    for rl in (100, 150):
        text, pairs = make_input(rl, a.pairs)
        if a.flash:
            best = None
            for _ in range(a.runs):
                t0 = time.perf_counter()
                p = subprocess.run([a.flash, "-q", "--interleaved-input", "-m", "10", "-M", "150", "-t", str(a.threads), "-To", "-c", "-"], input=text,
                                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                dt = time.perf_counter() - t0
                assert p.returncode == 0
                best = dt if best is None else min(best, dt)
            lines.append(f"flash -t {a.threads}  {rl} bp  {pairs} pairs  {len(text) / 1e6:.0f} MB in  best of {a.runs}: {best:.3f} s  {pairs / best / 1e6:.2f} M pairs/s "
                         f"(wall clock of the process, input on a pipe, output discarded)")
            continue
        import microcket_amd as m
        res = []
        for run in range(a.runs + 1):                    # run 0 warms up
            with m.Stitcher() as s:
                t0 = time.perf_counter()
                s.push(text)
                s.finish()
                dt = time.perf_counter() - t0
                st, tm = s.stats(), s.timing()
            assert st.total == pairs
            if run:
                res.append((dt, tm))
        dt, tm = min(res)
        kern = sum(tm)
        lines.append(f"stitch  {rl} bp  {pairs} pairs  {len(text) / 1e6:.0f} MB in  combined {100.0 * st.combined / st.total:.2f}%  best of {a.runs}: "
                     f"whole call {dt * 1e3:.1f} ms = {pairs / dt / 1e6:.2f} M pairs/s (host copies in and out included); on the device {kern:.1f} ms = "
                     f"{pairs / kern / 1e3:.2f} M pairs/s: line index {tm[0]:.1f}, scoring {tm[1]:.1f}, sizes + scans {tm[2]:.1f}, writing {tm[3]:.1f} ms")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
