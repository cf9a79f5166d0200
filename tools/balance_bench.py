"""Cost of matrix balancing (mkt_matrix_balance) on one MI355X -> profiles/matrix_balance.txt.

    python tools/balance_bench.py [--pairs N] [--reps 3] [--cpu-cells 60000000] [--out profiles/matrix_balance.txt]
                                  [--note 'text' ...] [--bench-line 'this commit=<json>' ...]

The data set and the nine resolutions of tools/matrix_bench.py: the key list of the bench's workload (C2: synthetic 150 bp pairs, hg38,
unc mode) -> Matrix.add_keys -> run -> balance(k) with the default options.  Per resolution: the one-time setup and the iteration loop
(device time between HIP events, mkt_matrix_balance_timing; the host looks at the device's state once per 4 iterations, so the loop
holds up to 3 iterations of empty launches and the looks; other batch sizes through $MKT_BALANCE_BATCH are measured next to it), the host clock
around the whole call (which adds the filters on the host), iterations, masked bins, and the bytes one sweep has to move: 8 per cell
from each of the two copies (bin2, count / bin1, count) plus 8 per bin for the bias read, the marginal written and read twice and the
bias rewritten -- the gathers of bias[] are meant to hit in cache and are not counted.
CPU yardstick: tests/balancedef.py on the cells fetched from the GPU, one core (resolutions with at most --cpu-cells cells), which also
gives the largest relative deviation of the weights next to the derived bound iterations x longest row x 2^-52.
--kernel-only: one balance of every resolution and nothing written (for rocprofv3 --kernel-trace --stats)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from matrix_bench import HG38, RES, TABLE, cpu_model  # noqa: E402

HBM_ACHIEVABLE = 6.29e12           # bytes/s, a float4 copy on this part (the figure the kernel notes of this project use)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-cells", type=int, default=60_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_balance.txt"))
    ap.add_argument("--note", action="append", default=[])
    ap.add_argument("--bench-line", action="append", default=[])
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import balancedef as bd
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("balance_bench: no HIP device; nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

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
        if args.kernel_only:
            for k in range(len(RES)):
                mx.balance(k)
            return
        say(f"# matrix balancing (ICE, default options), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator (tools/matrix_bench.py), resolutions {','.join(map(str, RES))}")
        say("# setup / loop: device ms between HIP events; call: host clock around mkt_matrix_balance (adds the host-side filters); sweep bytes: 16 per cell + 40 per bin")
        say("# loop = the whole batched loop: one look at the state per 4 iterations, so it holds up to 3 iterations of empty launches behind the last one;"
            " ms/iter = loop / iterations and the GB/s derived from it are therefore lower bounds of the sweep's own rate")
        say("    resolution      nbins        cells lanes long bins  iters conv   masked  setup ms   loop ms  ms/iter  call ms   GB/s of sweep bytes (share of 6.29 TB/s)")
        stats = []
        for k, r in enumerate(RES):
            nbins, nnz, _tb = mx.info(k)
            avg = 2 * nnz // nbins
            lanes = 64 if avg >= 48 else 32 if avg >= 24 else 16 if avg >= 12 else 8   # the rule of mkt_balance.hip
            b1, b2, _c = mx.cells(k)
            nlong = int(((np.bincount(b1, minlength=nbins) + np.bincount(b2, minlength=nbins)) > 1024).sum())
            del b1, b2, _c
            st = mx.balance(k)                                               # the first call pays the setup
            setup = mx.balance_timing_ms(k)[0]
            loops, calls = [], []
            for _ in range(max(args.reps, 1)):
                t0 = time.perf_counter()
                st = mx.balance(k)
                calls.append((time.perf_counter() - t0) * 1e3)
                loops.append(mx.balance_timing_ms(k)[1])
            loop = statistics.median(loops)
            per = loop / max(st.iterations, 1)
            rate = (16.0 * nnz + 40.0 * nbins) / (per * 1e-3)
            say(f"    {r:>10} {nbins:>10} {nnz:>12} {lanes:>5} {nlong:>9} {st.iterations:>6} {int(st.converged):>4} {st.masked:>8} {setup:>9.3f} {loop:>9.3f} {per:>8.4f} {statistics.median(calls):>8.2f}"
                f"   {rate / 1e9:8.1f} ({100.0 * rate / HBM_ACHIEVABLE:.1f} %)")
            stats.append((st, per))
        say("# iterations per look at the state ($MKT_BALANCE_BATCH): loop ms, median of the same number of calls; 4 is what the library does")
        say("    resolution   batch 1   batch 2   batch 4   batch 8  batch 16")
        for k, r in enumerate(RES):
            row = []
            for batch in (1, 2, 4, 8, 16):
                os.environ["MKT_BALANCE_BATCH"] = str(batch)
                loops = []
                for _ in range(max(args.reps, 1)):
                    mx.balance(k)
                    loops.append(mx.balance_timing_ms(k)[1])
                row.append(statistics.median(loops))
            os.environ.pop("MKT_BALANCE_BATCH", None)
            say(f"    {r:>10} " + " ".join(f"{x:>9.3f}" for x in row))
        for bl in args.bench_line:
            say(f"    bench.py, same GPU call: {bl}")
        say(f"# CPU yardstick: tests/balancedef.py (numpy, np.bincount marginals) on the GPU's cells, one core of {cpu_model()}; bound = iterations x longest row x 2^-52")
        say("    resolution   CPU s  CPU ms/iter  GPU ms/iter    ratio  iters masked (definition)   max rel dev of weights      bound")
        for k, r in enumerate(RES):
            nbins, nnz, _tb = mx.info(k)
            if nnz > args.cpu_cells:
                say(f"    {r:>10}   skipped: {nnz} cells > --cpu-cells")
                continue
            b1, b2, c = mx.cells(k)
            off = md.bin_layout(table, r)[0]
            t0 = time.perf_counter()
            want = bd.balance(b1, b2, c, nbins, off)
            t_cpu = time.perf_counter() - t0
            st, per = stats[k]
            w = mx.weights(k)
            same = bool((np.isnan(w) == np.isnan(want.weights)).all()) and (st.iterations, st.converged, st.masked) == (want.iterations, want.converged, want.masked)
            ok = ~np.isnan(want.weights) & ~np.isnan(w)
            dev = float(np.abs(w[ok] / want.weights[ok] - 1.0).max()) if ok.any() else 0.0
            bound = want.iterations * want.longest_row * 2.0 ** -52
            cpu_per = t_cpu * 1e3 / max(want.iterations, 1)
            say(f"    {r:>10} {t_cpu:>7.2f} {cpu_per:>12.2f} {per:>12.4f} {cpu_per / per:>8.0f} {want.iterations:>6} {want.masked:>6} {'same as GPU' if same else 'DIFFERS FROM GPU'}"
                f"   {dev:.3e}   {bound:.3e}")
            del b1, b2, c
    for n in args.note:
        say(f"# {n}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
