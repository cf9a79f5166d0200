"""Cost of the pileup (mkt_matrix_pileup) on one MI355X -> stdout (kept as profiles/matrix_pileup.txt).

    python tools/pileup_bench.py [--pairs N] [--reps 3] [--cpu-features 10000] > profiles/matrix_pileup.txt

The data set of tools/matrix_bench.py (what profiles/matrix_bench.txt was measured on): the key list of the bench's workload ->
Matrix.add_keys -> run -> balance(k) -> expected(k) at 10 kb and 5 kb, then pileup(k) with the default options (oe_smooth, corner 6)
around features drawn from a seed: stored cis cells at distances 20 .. 400 bins, with repeats when there are fewer than asked for.
Per resolution 10^4 and 10^6 features at flank 10 and 10^4 at flank 32: device ms between HIP events of the setup (the upload of the
features and statuses) and of the sweep (the chunk kernel and the fold) from mkt_matrix_pileup_timing, the median of --reps calls after
one warm-up call, and the wall time of the whole call (the statuses on the host and the copies included).  CPU yardstick:
tests/piledef.py on one core on the cells, weights and tables fetched from the GPU, for the first --cpu-features features; the ratio
compares seconds per feature with the wall time of the call."""
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

RES = (10_000, 5_000)
CASES = ((10_000, 10), (1_000_000, 10), (10_000, 32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-features", type=int, default=10_000)
    args = ap.parse_args()
    import numpy as np
    import matrixdef as md
    import microcket_amd as m
    import piledef as pd
    if m.device_count() < 1:
        raise SystemExit("pileup_bench: no HIP device; nothing is measured without one")
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
        print(f"# pileup (default options: oe_smooth, corner 6, ignore_diags 2, edges 0, after the default balance and expected), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator", flush=True)
        print(f"# features: stored cis cells at distances 20 .. 400 bins drawn from a seed.  setup / sweep: ms between HIP events, added over the batches, median of {args.reps} calls;")
        print("# setup is the upload of the features and their statuses, sweep the chunk kernel and the fold.  call: wall ms of mkt_matrix_pileup (statuses on the")
        print(f"# host, uploads, kernels, the copy back).  cpu: tests/piledef.py on one core ({cpu_model()}) for the first")
        print(f"# {args.cpu_features} features; ratio: its seconds per feature over the call's seconds per feature.")
        print("    resolution    features  flank   used  chunks        cells  setup ms  sweep ms   call ms   Mpositions/s   cpu s  cpu features     ratio")
        for k, r in enumerate(RES):
            mx.balance(k)
            ex = mx.expected(k)
            nbins, nnz, _ = mx.info(k)
            b1, b2, c = mx.cells(k)
            off, _, nb = md.bin_layout(table, r)
            offa = np.asarray(off)
            d = b2.astype(np.int64) - b1.astype(np.int64)
            cand = np.flatnonzero((np.searchsorted(offa, b1, side="right") == np.searchsorted(offa, b2, side="right")) & (d >= 20) & (d <= 400))
            rng = np.random.default_rng(7)
            w = mx.weights(k)
            for nf, flank in CASES:
                pick = cand[rng.integers(0, cand.size, nf)]
                a, b = b1[pick].copy(), b2[pick].copy()
                info = mx.pileup(k, a, b, flank=flank)
                t, wall = [[], []], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    info = mx.pileup(k, a, b, flank=flank)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    for x, v in zip(t, mx.pileup_timing_ms(k)):
                        x.append(v)
                s_ms, w_ms, c_ms = statistics.median(t[0]), statistics.median(t[1]), statistics.median(wall)
                nc = min(nf, args.cpu_features)
                t0 = time.perf_counter()
                want = pd.pileup(b1.astype(np.int64), b2.astype(np.int64), c, nb, off, a[:nc].astype(np.int64), b[:nc].astype(np.int64), weights=w,
                                 expected=ex.genome.expected, expected_smooth=ex.genome.expected_smooth, flank=flank)
                dt = time.perf_counter() - t0
                if nc == nf:                                                  # the whole list went through the definition: the bits must agree
                    got = mx.pileup_result(k)
                    assert got.vsum.tobytes() == want.vsum.tobytes() and got.n.tobytes() == want.n.tobytes(), (r, nf, flank)
                side = 2 * flank + 1
                print(f"{r:14d} {nf:11d} {flank:6d} {info.used:6d} {info.chunks:7d} {nnz:12d} {s_ms:9.3f} {w_ms:9.3f} {c_ms:9.3f} {info.used * side * side / (w_ms * 1e-3) / 1e6:14.1f} "
                      f"{dt:7.2f} {nc:13d} {(dt / nc) / (c_ms * 1e-3 / nf):9.0f}x", flush=True)


if __name__ == "__main__":
    main()
