"""Cost of the compartment eigenvectors (mkt_matrix_eigs) on one MI355X -> stdout (kept in profiles/matrix_eigs.txt).

    python tools/eigs_bench.py [--pairs N] [--max-res 100000] [--cpu-bins 3000] > profiles/matrix_eigs.txt

The data set of tools/matrix_bench.py at its resolutions of --max-res and coarser: the key list of the bench's workload -> Matrix.add_keys
-> run -> balance(k) -> expected(k) -> eigs(k) with the default options.  Per resolution: setup ms, the HIP-event time of all sweeps of
the call and the rest of the loop (reductions, the 8 x 8 step on the host with its copies) with its share, iterations per chromosome;
then ONE FULL SWEEP, timed on its own: the sweep of eigs(k, max_iters=1), in which no chromosome is done yet (the sweeps of a whole call
get cheaper as chromosomes freeze, so their mean says nothing about the kernel), median of --reps calls; the bytes that sweep must
move (16 per cell: each cell is walked from both sides, 8 bytes each; 8 per bin of pointers; 64 per bin written) over that time
against the achievable HBM rate -- the X gathers, weights and E are meant to hit in cache and are not counted -- and tests/eigsdef.py reference_eigs (dense eigh) on one core for the same
chromosomes when the largest chromosome has at most --cpu-bins bins.  Whether the leading vector is the all-ones direction of a mostly
empty matrix (lambda_1 ~ -n_good) is printed per resolution: there compartments mean nothing."""
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
    ap.add_argument("--max-res", type=int, default=100000)
    ap.add_argument("--cpu-bins", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import eigsdef as gd
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("eigs_bench: no HIP device; nothing is measured without one")
    res_list = [r for r in RES if r >= args.max_res]
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    table = [(nm.encode(), l) for nm, l in HG38]
    with m.Matrix(TABLE, res_list, device=0) as mx:
        mx.add_keys(ctx, True)
        ds.close(); ctx.close()
        mx.run()
        print(f"# compartment eigenvectors (default options, use_weights 1 after the default balance), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator", flush=True)
        print(f"# cpu: tests/eigsdef.py reference_eigs (numpy eigh of the dense A_c) on one core ({cpu_model()}), building A_c not counted")
        print("    resolution     bins        cells  solved  conv  iterations (min / median / max)  setup ms  sweeps ms  rest ms  rest %  full sweep ms  its GB/s (share)   all-ones chroms   cpu eigh s")
        for k, r in enumerate(res_list):
            mx.balance(k)
            e = mx.expected(k)
            mx.eigs(k)                                                        # warm-up
            res = mx.eigs(k)
            s_ms, w_ms, o_ms = mx.eigs_timing_ms(k)
            nbins, nnz, _ = mx.info(k)
            it = res.iterations[res.iterations > 0]
            sweeps = int(it.max()) if it.size else 0
            one = []
            for _ in range(args.reps):                                        # one sweep with every chromosome live
                mx.eigs(k, max_iters=1)
                one.append(mx.eigs_timing_ms(k)[1])
            per = statistics.median(one)
            rate = (16.0 * nnz + 72.0 * nbins) / (per * 1e-3) if per > 0 else 0.0
            ones = int(sum(1 for c in range(len(res.n_good)) if res.iterations[c] and res.lambdas[c, 0] < -0.5 * res.n_good[c]))
            cpu = "-"
            off, _, nb = md.bin_layout(table, r)
            if max(np.diff(off + [nb])) <= args.cpu_bins:
                b1, b2, c = mx.cells(k)
                chs = gd.chromosomes(b1, b2, c, nb, off, e.genome.expected_smooth, weights=mx.weights(k))
                t0 = time.perf_counter()
                for ch in chs:
                    if not ch.skipped:
                        gd.reference_eigs(ch, 3)
                cpu = f"{time.perf_counter() - t0:.2f}"
            med = float(np.median(it)) if it.size else 0.0
            print(f"{r:14d} {nbins:8d} {nnz:12d} {res.info.solved:7d} {res.info.converged:5d}   {int(it.min()) if it.size else 0:5d} / {med:6.1f} / {sweeps:5d}        {s_ms:9.3f} {w_ms:10.3f} {o_ms:8.2f} {100.0 * o_ms / max(o_ms + w_ms, 1e-9):7.1f}"
                  f"  {per:13.4f} {rate / 1e9:9.1f} ({100.0 * rate / HBM_ACHIEVABLE:5.2f} %)  {ones:8d} of {res.info.solved:3d}   {cpu:>10}", flush=True)
            print(f"#   lambda_1 per chromosome: {' '.join(f'{v:.1f}' for v in res.lambdas[:, 0])}", flush=True)


if __name__ == "__main__":
    main()
