"""Cost of the contact-matrix stage (mkt_matrix_*, bin/pairs2matrix) on one MI355X -> profiles/matrix_bench.txt.

    python tools/matrix_bench.py [--pairs N] [--reps 5] [--text-gb 4] [--cpu-sample 4000000] [--out profiles/matrix_bench.txt]
                                 [--bench-line 'this commit=<json>' ...]

(a) resident route: the key list of the bench's workload (C2: synthetic 150 bp pairs, hg38, unc mode) -> Matrix.add_keys -> run at
    the driver's nine default resolutions; per resolution the device time between two HIP events (mkt_matrix_timing), in total the
    host clock around mkt_matrix_run, which ends in a synchronise; one warm-up run, then the median of --reps runs.
(b) text route: bin/pairs2matrix end to end (process start to exit, wall clock) on a .pairs file in /dev/shm made from the same data set
    and sorted by bin/pairsort.
(c) CPU yardstick: tests/matrixdef.py's numpy definition on a sample of the same keys, same nine resolutions.
--bench-line adds lines measured elsewhere in the same GPU call (python bench.py of this commit and of its parent) verbatim.
Kernel times are not taken here: run this tool with --kernel-only under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RES = [2500000, 1000000, 500000, 250000, 100000, 50000, 25000, 10000, 5000]      # microcket:98
HG38 = [("chr1", 248956422), ("chr10", 133797422), ("chr11", 135086622), ("chr12", 133275309), ("chr13", 114364328), ("chr14", 107043718),
        ("chr15", 101991189), ("chr16", 90338345), ("chr17", 83257441), ("chr18", 80373285), ("chr19", 58617616), ("chr2", 242193529),
        ("chr20", 64444167), ("chr21", 46709983), ("chr22", 50818468), ("chr3", 198295559), ("chr4", 190214555), ("chr5", 181538259),
        ("chr6", 170805979), ("chr7", 159345973), ("chr8", 145138636), ("chr9", 138394717), ("chrM", 16569), ("chrX", 156040895),
        ("chrY", 57227415)]
TABLE = "".join(f"{n}\t{l}\n" for n, l in HG38).encode()


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--text-gb", type=float, default=4.0)
    ap.add_argument("--cpu-sample", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_bench.txt"))
    ap.add_argument("--bench-line", action="append", default=[])
    ap.add_argument("--kernel-only", action="store_true", help="one warm-up and one run of the resident route, nothing written (for rocprofv3)")
    args = ap.parse_args()
    import numpy as np
    import matrixdef as md
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("matrix_bench: no HIP device; nothing is measured without one")
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
    say(f"# contact-matrix stage, one MI355X; data set: {ds.total_groups} synthetic 150 bp read pairs (hg38 names, unc mode, seed 1, the bench's C2 generator),"
        f" {nkeys} reported pairs in the context's key list; resolutions {','.join(map(str, RES))}")
    # (a) resident route
    with m.Matrix(TABLE, RES, device=0) as mx:
        t0 = time.perf_counter()
        mx.add_keys(ctx, True)
        t_add = (time.perf_counter() - t0) * 1e3
        pairs, skipped = mx.run()                                            # warm-up
        if args.kernel_only:
            mx.run()
            ds.close(); ctx.close()
            return
        per, tot = [[] for _ in RES], []
        for _ in range(max(args.reps, 5)):
            t0 = time.perf_counter()
            mx.run()
            tot.append((time.perf_counter() - t0) * 1e3)
            for k in range(len(RES)):
                per[k].append(mx.timing_ms(k))
        say(f"(a) resident route: mkt_matrix_add_keys {t_add:.2f} ms (once; KeyRec -> 16-byte records), pairs {pairs}, skipped {skipped}")
        say(f"    mkt_matrix_run, all nine resolutions: median {statistics.median(tot):.2f} ms of {len(tot)} runs after one warm-up (min {min(tot):.2f}, max {max(tot):.2f}; host clock"
            f" around the call, which ends in a synchronise; includes the per-run hipMalloc / hipFree of keys and results)")
        say("    resolution      nbins        cells   COO bytes   device ms (median, HIP events: keys + radix passes + run-length + text)")
        for k, r in enumerate(RES):
            nbins, nnz, tb = mx.info(k)
            say(f"    {r:>10} {nbins:>10} {nnz:>12} {tb:>11}   {statistics.median(per[k]):8.3f}")
        say(f"    sum of the nine device times: {sum(statistics.median(x) for x in per):.2f} ms")
        gpu_cells = {r: mx.cells(k) for k, r in enumerate(RES) if r in (2500000, 5000)}
    for bl in args.bench_line:
        say(f"    bench.py, same GPU call: {bl}")
    # (c) CPU yardstick on a sample of the same keys
    keys = ctx.ext_keys_fetch(True)
    names = ctx.ext_chr_names()
    index = {nm.encode(): i for i, (nm, _) in enumerate(HG38)}
    lut = np.full(8192, -1, dtype=np.int64)
    for slot, nm in names.items():
        lut[slot] = index.get(nm, -1)
    k0, k1 = keys[:, 0], keys[:, 1]
    ia = lut[((k0 >> np.uint64(45)) & np.uint64(8191)).astype(np.int64)]
    ib = lut[((k0 >> np.uint64(32)) & np.uint64(8191)).astype(np.int64)]
    pa = (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    pb = (k1 >> np.uint64(32)).astype(np.int64)
    table = [(nm.encode(), l) for nm, l in HG38]
    ns = min(args.cpu_sample, nkeys)
    t0 = time.perf_counter()
    md.definition_arrays(table, RES, ia[:ns], pa[:ns], ib[:ns], pb[:ns])
    t_cpu = time.perf_counter() - t0
    say(f"(c) CPU yardstick: tests/matrixdef.py (numpy: bin ids, np.unique per resolution) on the first {ns} of those keys, nine resolutions: {t_cpu * 1e3:.0f} ms"
        f" = {t_cpu / ns * 1e9:.0f} ns per pair ({t_cpu / ns * nkeys:.1f} s for all {nkeys} at that rate); host {cpu_model()}, the job is limited to 16 CPUs, numpy runs this on one")
    if ns == nkeys:                                                          # the whole set was binned on the CPU: compare
        want = md.definition_arrays(table, [5000], ia, pa, ib, pb)[5000][0]
        b1, b2, c = gpu_cells[5000]
        assert want.shape[0] == b1.size and (want[:, 0] == b1).all() and (want[:, 1] == b2).all() and (want[:, 2] == c).all()
        say("    the GPU's cells at 5000 equal the CPU's")
    del keys, k0, k1, ia, ib, pa, pb
    # (b) text route: a sorted .pairs file in /dev/shm, bin/pairs2matrix end to end
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    raw, srt, pre = os.path.join(shm, "mx_bench.raw.pairs"), os.path.join(shm, "mx_bench.pairs"), os.path.join(shm, "mx_bench.out")
    try:
        want_bytes = int(args.text_gb * 1e9)
        with m.Context("unc", 0.5, 10, False, 8, device=0, ordered=True) as c2, open(raw, "wb") as f:
            wrote = 0
            for (p, n, _g) in ds.blocks:
                c2.reset()
                c2.submit_device(p, n)
                c2.sync()
                pb_, _ = c2.fetch_last_block()
                pb_ = pb_[:pb_.rfind(b"\n") + 1]
                f.write(pb_)
                wrote += len(pb_)
                if wrote >= want_bytes:
                    break
        ds.close(); ctx.close()
        with open(srt, "wb") as f:
            subprocess.run([os.path.join(ROOT, "microcket_amd", "bin", "pairsort"), raw], stdout=f, check=True)
        os.remove(raw)
        size = os.path.getsize(srt)
        exe = os.path.join(ROOT, "microcket_amd", "bin", "pairs2matrix")
        tab = os.path.join(shm, "mx_bench.sizes")
        open(tab, "wb").write(TABLE)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            subprocess.run([exe, "-g", tab, "-r", ",".join(map(str, RES)), "-o", pre, srt], check=True)
            walls.append(time.perf_counter() - t0)
        stat = open(pre + ".matrix.stat").read().split("\n")
        say(f"(b) text route: bin/pairs2matrix end to end on {size / 1e9:.2f} GB of sorted .pairs text in {shm} ({stat[0].split()[1]} pairs, {'sorted by bin/pairsort' }), nine resolutions,"
            f" outputs written to {shm}: wall {min(walls):.2f} s best of {len(walls)} ({', '.join(f'{w:.2f}' for w in walls)}) = {size / 1e9 / min(walls):.2f} GB/s of text"
            f" (process start, HIP runtime and context creation, 64 MiB reads + synchronous copies, binning, fetching and writing {sum(os.path.getsize(f'{pre}.{r}.coo') for r in RES) / 1e9:.2f} GB of COO text and the bins files)")
    finally:
        for fn in [raw, srt, pre + ".matrix.stat", os.path.join(shm, "mx_bench.sizes")] + [f"{pre}.{r}.{e}" for r in RES for e in ("coo", "bins.bed")]:
            if os.path.exists(fn):
                os.remove(fn)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
