"""Cost of the pair statistics on the GPU (mkt_pairstat_*) on the synthetic sorted final.pairs of tools/pairsgz_bench.py
(10 M lines): the line-index and kernel times the library measures with HIP events, the whole Python call, and the kernel's share of
the achievable HBM rate (6.3 TB/s on an MI355X) counting the text and its 8-byte line starts once.  For comparison the wall time of
Matrix.add on the same text: copy, line index and k_mx_parse, the closest existing one-lane-per-line parse (its kernel time alone is
not exposed by the library).

    python tools/pairstat_bench.py [--lines 10000000] [--runs 3] [--out profiles/pairstat_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pairsgz_bench
    import microcket_amd as m
    text = pairsgz_bench.make_input(a.lines)
    table = b"".join(b"chr%d\t250000000\n" % k for k in range(1, 24))
    nl = text.count(10)
    out = [f"final.pairs: {nl} lines, {len(text) / 1e6:.0f} MB, sorted, {max(1, a.lines // pairsgz_bench.BLOCK)} chromosome pairs (the file of profiles/pairsgz_bench.txt)"]
    res = []
    for run in range(a.runs + 1):                        # run 0 warms up
        with m.PairStats(table) as ps:
            t0 = time.perf_counter()
            ps.add(text)
            info = ps.run()
            dt = time.perf_counter() - t0
            tm = ps.timing_ms()
        if run:
            res.append((dt, tm))
    dt, tm = min(res, key=lambda r: r[0])
    moved = len(text) + 8 * nl
    share = moved / (tm["kernel"] * 1e-3) / (HBM_TBS * 1e12) if tm["kernel"] > 0 else 0.0
    out.append(f"  PairStats on one MI355X, best of {a.runs}: whole call {dt * 1e3:.1f} ms; on the device: line index {tm['index']:.2f} ms, k_ps_text {tm['kernel']:.2f} ms, "
               f"copy + index + kernel {tm['total']:.1f} ms; the kernel reads {moved / 1e6:.0f} MB = {100 * share:.1f} % of {HBM_TBS} TB/s")
    out.append(f"  counters: total {info['total']}, cis {info['cis']}, trans {info['trans']}, skipped {info['skipped']}, convergence_dist {info['convergence_dist']}")
    best = None
    for run in range(a.runs + 1):
        with m.Matrix(table, [1000000]) as mx:
            t0 = time.perf_counter()
            mx.add(text)
            w = time.perf_counter() - t0
        if run:
            best = w if best is None else min(best, w)
    out.append(f"  for comparison Matrix.add of the same text (copy, line index, k_mx_parse; unchanged by this module), best of {a.runs}: {best * 1e3:.1f} ms wall")
    s = "\n".join(out) + "\n"
    sys.stdout.write(s)
    if a.out:
        with open(a.out, "a") as f:
            f.write(s)


if __name__ == "__main__":
    main()
