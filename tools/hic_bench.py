"""Cost of the .hic container (mkt_matrix_hic) on one MI355X -> profiles/matrix_hic.txt.

    python tools/hic_bench.py [--pairs 100000000] [--levels 2,1,0]

The data set is tools/matrix_bench.py's: the key list of the bench's workload -> Matrix.add_keys -> run at the driver's nine default
resolutions.  Then Matrix.hic() per level: one warm-up and one timed call; the per-resolution device times are the library's HIP events.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from matrix_bench import RES, TABLE  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--levels", default="2,1,0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_hic.txt"))
    args = ap.parse_args()
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("hic_bench: no HIP device; nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    say(f"# .hic container, one MI355X; data set: {ds.total_groups} synthetic 150 bp read pairs (hg38 names, unc mode, seed 1), {ctx.ext_key_count(True)} reported pairs;"
        f" resolutions {','.join(map(str, RES))}; block_bins 1000")
    with m.Matrix(TABLE, RES, device=0) as mx:
        mx.add_keys(ctx, True)
        pairs, skipped = mx.run()
        say(f"pairs {pairs}, skipped {skipped}")
        for level in [int(x) for x in args.levels.split(",")]:
            mx.hic(level=level)                                              # warm-up
            t0 = time.perf_counter()
            info = mx.hic(level=level)
            wall = (time.perf_counter() - t0) * 1e3
            say(f"level {level}: call {wall:.1f} ms (host clock; includes the allocations, the copies of the block tables and the layout on the host); " +
                ", ".join(f"{k} {v}" for k, v in info.items()))
            say("  r\tcells\tsort_ms\tserialise_ms\tdeflate_ms\tpack_ms")
            tot = [0.0] * 4
            for k, r in enumerate(RES):
                t = mx.hic_timing_ms(k)
                tot = [a + b for a, b in zip(tot, t)]
                say(f"  {r}\t{mx.info(k)[1]}\t" + "\t".join(f"{x:.3f}" for x in t))
            say("  all\t\t" + "\t".join(f"{x:.3f}" for x in tot))
            if tot[2] > 0:
                say(f"  deflate: {info['raw_bytes'] / tot[2] / 1e6:.2f} GB/s of payload, ratio {info['deflated_bytes'] / info['raw_bytes']:.3f}")
    ds.close()
    ctx.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
