"""Cost of the expected tables (mkt_matrix_expected) and of the per-cell values on one MI355X -> profiles/matrix_expected.txt.

    python tools/expected_bench.py [--pairs N] [--reps 3] [--cpu-cells 60000000] [--out profiles/matrix_expected.txt] [--note 'text' ...]

The data set and the nine resolutions of tools/matrix_bench.py: the key list of the bench's workload (C2: synthetic 150 bp pairs, hg38,
unc mode) -> Matrix.add_keys -> run -> balance(k) -> expected(k).  Per resolution: the one-time setup (grouping the cells by segment:
the radix passes, the grouped copy, the segment pointers) and the sums (validity bits, n_valid, the segment sums), device time between
HIP events (mkt_matrix_expected_timing); the host clock around the whole call, which adds the copy of the tables to the host and the
genome-wide and smoothed tables made there; the host clock around one values() fetch.  Bytes the sums have to move: 12 per cell of the
grouped copy, 4 per segment pointer, 16 per segment written, 8 per bin of n_valid -- the gathers of w[] are meant to hit in cache and
are not counted, nor are the validity bits that n_valid re-reads from cache.
CPU yardstick: tests/expecteddef.py on the cells and weights fetched from the GPU, one core (resolutions with at most --cpu-cells
cells), which also gives the largest relative deviation of the cis and trans sums next to the derived bound T x 2^-52.
--kernel-only: one expected() of every resolution and nothing written (for rocprofv3 --kernel-trace --stats)."""
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
    ap.add_argument("--cpu-cells", type=int, default=60_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_expected.txt"))
    ap.add_argument("--note", action="append", default=[])
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import expecteddef as ed
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("expected_bench: no HIP device; nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    table = [(nm.encode(), l) for nm, l in HG38]
    nchr = len(HG38)
    with m.Matrix(TABLE, RES, device=0) as mx:
        mx.add_keys(ctx, True)
        ds.close(); ctx.close()
        mx.run()
        for k in range(len(RES)):
            mx.balance(k)
        if args.kernel_only:
            for k in range(len(RES)):
                mx.expected(k)
            return
        say(f"# expected tables (use_weights 1, after the default balance), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator (tools/matrix_bench.py), resolutions {','.join(map(str, RES))}")
        say("# setup / sums: device ms between HIP events; call: host clock around mkt_matrix_expected with the setup reused (adds the copy of the tables and the host-side genome-wide and smoothed tables);")
        say("# values: host clock around one fetch of all oe values (kernel + 8 bytes per cell to the host); sums bytes: 12 per cell + 20 per segment + 8 per bin")
        say("    resolution      nbins        cells lanes long segs   chunks  setup ms   sums ms  call ms values ms   GB/s of sums bytes (share of 6.29 TB/s)")
        sums_ms, setups = {}, {}
        for k, r in enumerate(RES):
            nbins, nnz, _tb = mx.info(k)
            nseg = nbins + nchr * (nchr - 1) // 2
            avg = nnz // nseg
            lanes = 64 if avg >= 48 else 32 if avg >= 24 else 16 if avg >= 12 else 8   # the rule of mkt_expected.hip
            mx.expected(k)                                                   # the first call pays the setup
            setup = mx.expected_timing_ms(k)[0]
            sums, calls, vals = [], [], []
            for _ in range(max(args.reps, 1)):
                t0 = time.perf_counter()
                mx.expected(k)
                calls.append((time.perf_counter() - t0) * 1e3)
                sums.append(mx.expected_timing_ms(k)[1])
                t0 = time.perf_counter()
                v = mx.values(k, "oe")
                vals.append((time.perf_counter() - t0) * 1e3)
            del v
            b1, b2, _c = mx.cells(k)
            off = np.asarray(md.bin_layout(table, r)[0])
            chrom = np.searchsorted(off, np.arange(nbins), side="right") - 1
            ca, cb = chrom[b1], chrom[b2]
            seg = np.where(ca == cb, off[ca] + (b2.astype(np.int64) - b1), nbins + ca * (2 * nchr - ca - 1) // 2 + (cb - ca - 1))
            per = np.bincount(seg, minlength=nseg)
            nlong = int((per > 1024).sum())
            chunks = int(((per[per > 1024] + 4095) // 4096).sum())
            del b1, b2, _c, seg, ca, cb
            s_ms = statistics.median(sums)
            sums_ms[k], setups[k] = s_ms, setup
            rate = (12.0 * nnz + 20.0 * nseg + 8.0 * nbins) / (s_ms * 1e-3)
            say(f"    {r:>10} {nbins:>10} {nnz:>12} {lanes:>5} {nlong:>9} {chunks:>8} {setup:>9.3f} {s_ms:>9.3f} {statistics.median(calls):>8.2f} {statistics.median(vals):>9.2f}"
                f"   {rate / 1e9:8.1f} ({100.0 * rate / HBM_ACHIEVABLE:.1f} %)")
            flush()
        say(f"# CPU yardstick: tests/expecteddef.py (numpy: np.bincount sums, one popcount-free loop over the diagonals for n_valid) on the GPU's cells and weights, one core of {cpu_model()}")
        say("    resolution   CPU s   GPU setup + sums ms    ratio   integers and NaN pattern   max rel dev of cis / trans sums   largest T x 2^-52")
        for k, r in enumerate(RES):
            nbins, nnz, _tb = mx.info(k)
            if nnz > args.cpu_cells:
                say(f"    {r:>10}   skipped: {nnz} cells > --cpu-cells")
                continue
            b1, b2, c = mx.cells(k)
            w = mx.weights(k)
            off = md.bin_layout(table, r)[0]
            t0 = time.perf_counter()
            want = ed.expected(b1, b2, c, nbins, off, weights=w)
            t_cpu = time.perf_counter() - t0
            got = mx.expected(k)
            gpu_ms = setups[k] + sums_ms[k]
            same = all((a == b).all() for a, b in ((got.cis.n_valid, want.cis.n_valid), (got.cis.count_sum, want.cis.count_sum), (got.trans.n_valid, want.trans.n_valid),
                                                   (got.trans.count_sum, want.trans.count_sum), (got.genome.n_valid, want.genome.n_valid)))
            same = same and bool((np.isnan(got.genome.expected_smooth) == np.isnan(want.genome.expected_smooth)).all())
            gs = np.concatenate([got.cis.balanced_sum, got.trans.balanced_sum])
            ws = np.concatenate([want.cis.balanced_sum, want.trans.balanced_sum])
            ok = ws != 0
            dev = float(np.abs(gs[ok] / ws[ok] - 1.0).max()) if ok.any() else 0.0
            say(f"    {r:>10} {t_cpu:>7.2f} {gpu_ms:>21.3f} {t_cpu * 1e3 / gpu_ms:>8.0f}   {'same as GPU' if same else 'DIFFERS FROM GPU'}   {dev:.3e}   {float(want.seg_cells.max()) * 2.0 ** -52:.3e}")
            del b1, b2, c, want, got
            flush()
    for n in args.note:
        say(f"# {n}")
    flush()


if __name__ == "__main__":
    main()
