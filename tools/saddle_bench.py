"""Cost of the saddle tables (mkt_matrix_saddle) on one MI355X -> stdout (kept as profiles/matrix_saddle.txt).

    python tools/saddle_bench.py [--pairs N] [--reps 3] > profiles/matrix_saddle.txt

The data set of tools/matrix_bench.py (what profiles/matrix_bench.txt was measured on): the key list of the bench's workload ->
Matrix.add_keys -> run -> balance(k) -> expected(k) -> eigs(k) at 1 Mb, 500 kb, 250 kb and 100 kb, then saddle(k) with the first
eigenvector as the track for Q = 5, 50 and 64, cis and trans, the other options at their defaults: the setup (on the host: the groups,
the positions, the copy of the weights, the upload of the groups; wall ms) and the sweep (the chunk kernel and the fold; ms between HIP
events) from mkt_matrix_saddle_timing, the median of --reps calls after one warm-up call, and the wall time of the whole call.  CPU
yardstick: tests/saddledef.py on one core on the cells, weights and tables fetched from the GPU, for Q = 50 of both contacts; its
tables must be the bytes of the GPU's."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from matrix_bench import HG38, TABLE, cpu_model  # noqa: E402

RES = (1_000_000, 500_000, 250_000, 100_000)
GROUPS = (5, 50, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import matrixdef as md
    import microcket_amd as m
    import saddledef as sd
    if m.device_count() < 1:
        raise SystemExit("saddle_bench: no HIP device; nothing is measured without one")
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    table = [(nm.encode(), l) for nm, l in HG38]
    with m.Matrix(TABLE, list(RES), device=0) as mx:
        mx.add_keys(ctx, True)
        ds.close(); ctx.close()
        mx.run()
        print(f"# saddle tables (track: eigenvector 1 of the default eigs; trims 250 / 250, kind oe, min_diag 2, after the default balance and expected), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator", flush=True)
        print(f"# setup: wall ms on the host (groups, positions, copy of the weights, upload of the groups); sweep: ms between HIP events (chunk kernel + fold); median of {args.reps} calls.")
        print(f"# call: wall ms of mkt_matrix_saddle.  cpu: tests/saddledef.py on one core ({cpu_model()}), Q = 50 only, same bytes checked.")
        print("    resolution contact   Q      bins        cells   cells used  chunks  setup ms  sweep ms   call ms  Mcells/s    cpu s")
        for k, r in enumerate(RES):
            mx.balance(k)
            ex = mx.expected(k)
            track = mx.eigs(k).vectors[0]
            nbins, nnz, _ = mx.info(k)
            b1, b2, c = mx.cells(k)
            off, _, nb = md.bin_layout(table, r)
            w = mx.weights(k)
            for contact in ("cis", "trans"):
                for Q in GROUPS:
                    info = mx.saddle(k, track, n_groups=Q, contact=contact)
                    t, wall = [[], []], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        info = mx.saddle(k, track, n_groups=Q, contact=contact)
                        wall.append((time.perf_counter() - t0) * 1e3)
                        for x, v in zip(t, mx.saddle_timing_ms(k)):
                            x.append(v)
                    s_ms, w_ms, c_ms = statistics.median(t[0]), statistics.median(t[1]), statistics.median(wall)
                    cpu = ""
                    if Q == 50:
                        t0 = time.perf_counter()
                        want = sd.saddle(b1, b2, c, nb, off, track, weights=w, expected=ex.genome.expected, expected_smooth=ex.genome.expected_smooth,
                                         trans_expected=ex.trans.expected, n_groups=Q, contact=contact)
                        cpu = f"{time.perf_counter() - t0:8.2f}"
                        got = mx.saddle_result(k)
                        assert all(getattr(got, f).tobytes() == getattr(want, f).tobytes() for f in sd.FIELDS), (r, contact, Q)
                    print(f"{r:14d} {contact:>7s} {Q:3d} {nbins:9d} {nnz:12d} {info.cells_used:12d} {info.chunks:7d} {s_ms:9.3f} {w_ms:9.3f} {c_ms:9.3f} {nnz / (w_ms * 1e-3) / 1e6:9.1f} {cpu:>8s}", flush=True)


if __name__ == "__main__":
    main()
