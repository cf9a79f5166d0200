"""Cost of loop calling (mkt_matrix_loops) on one MI355X -> stdout (kept as profiles/matrix_loops.txt).

    python tools/loops_bench.py [--pairs N] [--reps 3] [--cpu-candidates 300000] > profiles/matrix_loops.txt

The data set and the nine resolutions of tools/matrix_bench.py (what profiles/matrix_expected.txt was measured on): the key list of the
bench's workload -> Matrix.add_keys -> run -> balance(k) -> expected(k) -> loops(k) with the default options.  Per resolution: device
ms between HIP events of the neighbourhood pass (both launches and the look at the grown count between them), the histogram and the
flagging (mkt_matrix_loops_timing), the median of --reps calls after one warm-up call; the share of candidates whose window grew; the
bytes the pass must READ (12 per cell: bin1, bin2, count; 4 per bin: the row pointers; 8 per bin: the weights) as a fraction of the
achievable HBM rate -- the neighbour reads and E are meant to hit in cache and are not counted -- and next to it the same with the 150 bytes
per cell the pass WRITES (its per-cell results) added.  CPU yardstick: tests/loopsdef.py cells_pass on one core
on the cells, weights and expected table fetched from the GPU, for the resolutions with at most --cpu-candidates candidates (it keeps a
dense matrix per chromosome, so fine resolutions are out of its reach)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from matrix_bench import HG38, RES, TABLE, cpu_model  # noqa: E402

HBM_ACHIEVABLE = 6.29e12           # bytes/s, a float4 copy on this part (the figure the kernel notes of this project use)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-candidates", type=int, default=300_000)
    args = ap.parse_args()
    import numpy as np
    import loopsdef as ld
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("loops_bench: no HIP device; nothing is measured without one")
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    table = [(nm.encode(), l) for nm, l in HG38]
    with m.Matrix(TABLE, RES, device=0) as mx:
        mx.add_keys(ctx, True)
        ds.close(); ctx.close()
        mx.run()
        print(f"# loop calling (default options, use_weights 1 after the default balance), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator, resolutions {','.join(map(str, RES))}", flush=True)
        print(f"# pass / hist / flag: ms between HIP events, median of {args.reps} calls.  pass is NOT pure kernel time: between its two launches the host reads the number")
        print("# of grown cells (a 4-byte copy and a stream synchronise), which the events include.  hist and flag are one kernel each.")
        print("# read GB/s: the bytes the pass must read (12 per cell + 12 per bin) over pass ms, with its share of the achievable 6.29 TB/s; +written: the same with")
        print(f"# the 150 bytes per cell of results the pass writes.  cpu: tests/loopsdef.py cells_pass on one core ({cpu_model()})")
        print("    resolution        cells  candidates     tested  grew %  at_max  enriched  loops   pass ms  hist ms  flag ms  read GB/s (share)   +written GB/s (share)   cpu s    cpu / pass")
        for k, r in enumerate(RES):
            mx.balance(k)
            e = mx.expected(k)
            res = mx.loops(k)
            t = [[], [], []]
            for _ in range(args.reps):
                res = mx.loops(k)
                for a, v in zip(t, mx.loops_timing_ms(k)):
                    a.append(v)
            p_ms, h_ms, f_ms = (statistics.median(a) for a in t)
            i = res.info
            nbins = mx.info(k)[0]
            rd = (12.0 * i.cells + 12.0 * nbins) / (p_ms * 1e-3) if p_ms > 0 else 0.0
            rate = rd + 150.0 * i.cells / (p_ms * 1e-3) if p_ms > 0 else 0.0
            cpu = "-"
            ratio = "-"
            if 0 < i.candidates <= args.cpu_candidates:
                b1, b2, c = mx.cells(k)
                off, _, nb = md.bin_layout(table, r)
                w = mx.weights(k)
                t0 = time.perf_counter()
                ld.cells_pass(b1, b2, c, nb, off, e.genome.expected_smooth, weights=w)
                dt = time.perf_counter() - t0
                cpu, ratio = f"{dt:.2f}", f"{dt * 1e3 / p_ms:.0f}x"
            print(f"{r:14d} {i.cells:12d} {i.candidates:11d} {i.tested:10d} {100.0 * i.grew / max(i.candidates, 1):7.1f} {i.at_max:7d} {i.enriched:9d} {len(res.loops):6d} "
                  f"{p_ms:9.3f} {h_ms:8.3f} {f_ms:8.3f}  {rd / 1e9:8.1f} ({100.0 * rd / HBM_ACHIEVABLE:5.2f} %)    {rate / 1e9:8.1f} ({100.0 * rate / HBM_ACHIEVABLE:5.2f} %) {cpu:>8} {ratio:>10}", flush=True)


if __name__ == "__main__":
    main()
