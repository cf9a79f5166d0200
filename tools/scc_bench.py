"""Cost of the replicate comparison (mkt_matrix_scc) on one MI355X -> stdout (kept as profiles/matrix_scc.txt).

    python tools/scc_bench.py [--pairs N] [--reps 3] [--res 40000] > profiles/matrix_scc.txt

The data set of tools/matrix_bench.py (what profiles/matrix_bench.txt was measured on): the key list of the bench's workload, split by
the parity of the pair's index into two pseudo-replicates (Matrix.add_keys with skip flags) -> run at --res (40 kb) -> scc(A, B) with
h = 5 and 5 Mb of diagonals, raw counts and, after the default balance of both, with the weights; both weightings are host work and are
not varied.  Per call the fill (zeroing and scattering the bands) and the sweep (with the fold) from mkt_matrix_scc_timing (ms between
HIP events, added over the slabs), the median of --reps calls after one warm-up call, and the wall time of the whole call; the same with
slab_rows 256 (every slab one chunk high).  CPU yardstick: tests/sccdef.py on one core on the cells fetched from the GPU, cut down to
single chromosomes (the largest first); the first one that finishes in under a minute is reported, and its rows of the strata table
must be the bytes of the GPU's."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--res", type=int, default=40_000)
    ap.add_argument("--max-bp", type=int, default=5_000_000)
    args = ap.parse_args()
    import numpy as np
    import matrixdef as md
    import microcket_amd as m
    import sccdef as sd
    if m.device_count() < 1:
        raise SystemExit("scc_bench: no HIP device; nothing is measured without one")
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    nkeys = ctx.ext_key_count(True)
    odd = (np.arange(nkeys) & 1).astype(np.uint8)
    r, h, md_ = args.res, 5, args.max_bp // args.res
    table = [(nm.encode(), l) for nm, l in HG38]
    off, _, nb = md.bin_layout(table, r)
    with m.Matrix(TABLE, [r], device=0) as a, m.Matrix(TABLE, [r], device=0) as b:
        a.add_keys(ctx, True, flags=odd.tobytes())                               # the even pairs
        b.add_keys(ctx, True, flags=(1 - odd).tobytes())                         # the odd pairs
        ds.close(); ctx.close()
        pa, pb = a.run()[0], b.run()[0]
        print(f"# replicate comparison (SCC), one MI355X; data set: {nkeys} reported pairs of the bench's C2 generator split by parity into {pa} + {pb} pairs", flush=True)
        print(f"# resolution {r}, h = {h}, diagonals 0 .. {md_} ({args.max_bp} bp), min_n 3; {nb} bins, {a.info(0)[1]} + {b.info(0)[1]} stored cells")
        print(f"# fill, sweep: ms between HIP events added over the slabs (sweep includes the fold); call: wall ms of mkt_matrix_scc; median of {args.reps} calls after a warm-up")
        print("    weights  weighting  slab_rows   candidates         used  scored      count_a      count_b                   scc   fill ms  sweep ms   call ms  Mpos/s")
        for use_w in (0, 1):
            if use_w:
                a.balance(0)
                b.balance(0)
            for weighting in ("n", "var"):
                for slab in (0, 256):
                    o = dict(h=h, max_diag=md_, use_weights=use_w, weighting=weighting, slab_rows=slab)
                    info = a.scc(b, 0, **o)
                    t, wall = [[], []], []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        info = a.scc(b, 0, **o)
                        wall.append((time.perf_counter() - t0) * 1e3)
                        for x, v in zip(t, a.scc_timing_ms(0)):
                            x.append(v)
                    f_ms, s_ms, c_ms = statistics.median(t[0]), statistics.median(t[1]), statistics.median(wall)
                    print(f"{use_w:11d} {weighting:>10s} {slab:10d} {info.candidates:12d} {info.used:12d} {info.scored:7d} {info.count_a:12d} {info.count_b:12d} {info.scc:21.17g} {f_ms:9.3f} {s_ms:9.3f} {c_ms:9.3f} "
                          f"{info.candidates / (s_ms * 1e-3) / 1e6:7.0f}", flush=True)
        # CPU yardstick: the definition, dense, one chromosome at a time, the largest first
        info = a.scc(b, 0, h=h, max_diag=md_)
        got = a.scc_result(0)
        D = info.strata
        ca, cb = (tuple(x.astype(np.int64) for x in mx.cells(0)) for mx in (a, b))
        sizes = [((off[c + 1] if c + 1 < len(off) else nb) - off[c], c) for c in range(len(off))]
        for nc, c in sorted(sizes, reverse=True):
            lo = off[c]
            cut = [tuple(x[(s[0] >= lo) & (s[1] < lo + nc)] - (lo if k < 2 else 0) for k, x in enumerate(s)) for s in (ca, cb)]
            t0 = time.perf_counter()
            want = sd.scc(cut[0], cut[1], nc, [0], h=h, max_diag=md_)
            dt = time.perf_counter() - t0
            same = all(getattr(want, f).tobytes() == getattr(got, f)[c * D:(c + 1) * D].tobytes() for f in sd.STRATA)
            print(f"# cpu: tests/sccdef.py on one core ({cpu_model()}), {HG38[c][0]} alone ({nc} bins, {cut[0][0].size} + {cut[1][0].size} cis cells, dense {nc} x {nc}): {dt:.2f} s; "
                  f"its {D} strata rows {'are the bytes of' if same else 'DIFFER from'} the GPU's", flush=True)
            assert same, HG38[c][0]
            if dt < 60:
                break


if __name__ == "__main__":
    main()
