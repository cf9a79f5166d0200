"""Cost of the insulation scores (mkt_matrix_insulation) on one MI355X -> stdout (kept as profiles/matrix_insulation.txt).

    python tools/insulation_bench.py [--pairs N] [--reps 3] [--cpu-chrom chr21] > profiles/matrix_insulation.txt

The data set and the nine resolutions of tools/matrix_bench.py (what profiles/matrix_bench.txt was measured on): the key list of the
bench's workload -> Matrix.add_keys -> run -> balance(k) -> insulation(k) with the windows among 100 / 250 / 500 kb that are whole
multiples of the resolution (a resolution with none is left out) and the default options.  Per resolution: device ms between HIP
events of the setup (the copy of the weights, the prefix count of the valid bins on the host, its upload) and of the sweep kernel
(mkt_matrix_insulation_timing), the median of --reps calls after one warm-up call; the stored cells inside the largest diamonds, counted
on the host from the cells (a cis cell at distance d >= ignore_diags lies in d + 1 diamonds for d < W and in 2 W - 1 - d for
W <= d <= 2 W - 2; masked rows and columns are not taken out), and that number over the sweep time.  CPU yardstick:
tests/insuldef.py (dense, so one chromosome only: --cpu-chrom) on one core on the cells and weights fetched from the GPU; the ratio
compares seconds per bin, the GPU's taken over all bins."""
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

WINDOWS_BP = (100_000, 250_000, 500_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-chrom", default="chr21")
    ap.add_argument("--cpu-bins", type=int, default=10_000, help="no CPU run for a chromosome of more bins (the restatement is dense)")
    args = ap.parse_args()
    import numpy as np
    import insuldef as idf
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("insulation_bench: no HIP device; nothing is measured without one")
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    table = [(nm.encode(), l) for nm, l in HG38]
    cc = [nm for nm, _ in HG38].index(args.cpu_chrom)
    with m.Matrix(TABLE, RES, device=0) as mx:
        mx.add_keys(ctx, True)
        ds.close(); ctx.close()
        mx.run()
        print(f"# insulation scores (default options, use_weights 1 after the default balance), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator", flush=True)
        print(f"# windows: those of {', '.join(map(str, WINDOWS_BP))} bp that are whole multiples of the resolution.  setup / sweep: ms between HIP events, median of {args.reps} calls;")
        print("# setup holds a copy of the weights to the host, the prefix count there and its upload; sweep is one kernel.  diamond cells: stored cells inside")
        print("# the largest diamonds, counted from the cells (masked bins not taken out).  cpu: tests/insuldef.py on one core")
        print(f"# ({cpu_model()}) for {args.cpu_chrom} alone; ratio: its seconds per bin over the sweep's seconds per bin.")
        print("    resolution  windows (bins)        bins        cells  lanes  defined  boundaries  setup ms  sweep ms   diamond cells  Gcells/s   cpu s  cpu bins      ratio")
        for k, r in enumerate(RES):
            windows = [b // r for b in WINDOWS_BP if b % r == 0 and b // r <= 1024]
            if not windows:
                continue
            mx.balance(k)
            info = mx.insulation(k, windows)
            t = [[], []]
            for _ in range(args.reps):
                info = mx.insulation(k, windows)
                for a, v in zip(t, mx.insulation_timing_ms(k)):
                    a.append(v)
            s_ms, w_ms = (statistics.median(a) for a in t)
            nbins, nnz, _ = mx.info(k)
            b1, b2, c = mx.cells(k)
            off, _, nb = md.bin_layout(table, r)
            offa = np.asarray(off)
            cis = np.searchsorted(offa, b1, side="right") == np.searchsorted(offa, b2, side="right")
            d = (b2.astype(np.int64) - b1.astype(np.int64))[cis]
            W = windows[-1]
            d = d[(d >= 2) & (d <= 2 * W - 2)]
            visited = int(np.where(d < W, d + 1, 2 * W - 1 - d).sum())
            per_row = nnz // max(nbins, 1)
            x = W if per_row >= 1 else W // 2
            lanes = 64 if x >= 48 else 32 if x >= 24 else 16 if x >= 12 else 8
            cpu, cbins, ratio = "-", "-", "-"
            lo, hi = off[cc], (off[cc + 1] if cc + 1 < len(off) else nb)
            if hi - lo <= args.cpu_bins:
                sel = (b1 >= lo) & (b1 < hi) & (b2 >= lo) & (b2 < hi)
                w = mx.weights(k)[lo:hi]
                t0 = time.perf_counter()
                idf.insulation(b1[sel].astype(np.int64) - lo, b2[sel].astype(np.int64) - lo, c[sel], hi - lo, [0], windows, weights=w)
                dt = time.perf_counter() - t0
                cpu, cbins = f"{dt:.2f}", str(hi - lo)
                ratio = f"{(dt / (hi - lo)) / (w_ms * 1e-3 / nbins):.0f}x" if w_ms > 0 else "-"
            print(f"{r:14d}  {','.join(map(str, windows)):>14} {nbins:11d} {nnz:12d} {lanes:6d} {info.defined[-1]:8d} {info.boundaries[-1]:11d} {s_ms:9.3f} {w_ms:9.3f} "
                  f"{visited:15d} {visited / (w_ms * 1e-3) / 1e9 if w_ms > 0 else 0.0:9.2f} {cpu:>7} {cbins:>9} {ratio:>10}", flush=True)


if __name__ == "__main__":
    main()
