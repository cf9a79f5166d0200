"""Cost of the viewpoint contact profiles (mkt_matrix_viewpoint) on one MI355X -> profiles/matrix_viewpoint.txt.

    python tools/viewpoint_bench.py [--pairs N] [--reps 7] [--out profiles/matrix_viewpoint.txt]
    python tools/viewpoint_bench.py --cpu-only [--perl-dir DIR] [--cpu-sample 1000000]

(a) the data set of profiles/matrix_bench.txt (the bench's C2 generator: synthetic 150 bp pairs, hg38, unc mode; 100 M groups give 67 M
    reported pairs) as resident records (Matrix.add_keys, run at one resolution), then mkt_matrix_viewpoint in two configurations:
    a small viewpoint (chrM, the stand-in for an episome such as chrEBV) and chr1, where the atomics of the tracks and the sort of the
    keys matter.  Two warm-up calls, then --reps calls; per call the two device times of mkt_matrix_viewpoint_timing (HIP events: the
    two scans of the records; the sort with the run-length passes) and the host clock around the call.  The scan reads every 16-byte
    record twice (count, then emit): its share of the HBM rate is 2 * 16 * n bytes over the scan time against 8 TB/s.
(b) --cpu-only, for scale, on one core: the reference's two Perl scripts (--perl-dir, when given) and tests/viewpointdef.py on a seeded
    .pairs sample of --cpu-sample lines with 0.1 % of the pairs on chrEBV.  No GPU is needed or used."""
import argparse
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from matrix_bench import HG38, TABLE                                              # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def cpu_part(args, say):
    import viewpointdef as vd
    rng = random.Random(1)
    table = HG38 + [("chrEBV", 171823)]
    lens = dict(table)
    names = [n for n, _ in HG38]
    rows = []
    for i in range(args.cpu_sample):
        a = rng.choice(names)
        b = "chrEBV" if rng.random() < 0.001 else rng.choice(names)
        rows.append(f"r{i}\t{a}\t{rng.randint(1, lens[a])}\t{b}\t{rng.randint(1, lens[b])}\t+\t-\n")
    text = "".join(rows).encode()
    tt = "".join(f"{n}\t{l}\n" for n, l in table).encode()
    t0 = time.perf_counter()
    bg, ln, pt = vd.ebv_texts(text, tt, "chrEBV", r"chr\d+$", 200, 1000000, 0.01, 1000, 5)
    t_def = time.perf_counter() - t0
    say(f"(b) one core, {args.cpu_sample} .pairs lines, 0.1 % with chrEBV on the second side ({bg.count(bytes([10]))} bedgraph lines, {ln.count(bytes([10]))} links, {pt.count(bytes([10]))} partner cells):")
    say(f"    tests/viewpointdef.py (parse + both profiles + texts): {t_def:.2f} s")
    if args.perl_dir:
        env = dict(os.environ, LC_ALL="C")
        with tempfile.TemporaryDirectory() as d:
            fn = os.path.join(d, "s.pairs")
            with open(fn, "wb") as f:
                f.write(text)
            t0 = time.perf_counter()
            a = subprocess.run(["perl", os.path.join(args.perl_dir, "calc.inter.EBV.matrix.and.circos.pl"), fn], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            t1 = time.perf_counter()
            b = subprocess.run(["perl", os.path.join(args.perl_dir, "calc.loop2EBV.pl"), fn], env=env, stdout=subprocess.PIPE, check=True)
            s = subprocess.run(["sort", "-k1,1", "-k2,2n"], input=b.stdout, env=env, stdout=subprocess.PIPE, check=True)
            t2 = time.perf_counter()
        same = (a.stdout, a.stderr, s.stdout) == (bg, ln, pt)
        say(f"    the reference's Perl scripts, wall time: links + bedgraph {t1 - t0:.2f} s, partner track + sort {t2 - t1:.2f} s; their three texts equal the definition's: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--block-groups", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--perl-dir", default=None)
    ap.add_argument("--cpu-sample", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_viewpoint.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.cpu_only:
        cpu_part(args, say)
        return
    import microcket_amd as m
    if m.device_count() < 1:
        raise SystemExit("viewpoint_bench: no HIP device; nothing is measured without one")
    ctx = m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS)
    ds = ctx.dataset(1, 0, args.pairs, args.block_groups, genome=0, read_len=150, lanes=1, tail_group=True)
    for (p, n, _g) in ds.blocks:
        ctx.submit_device(p, n)
    ctx.sync()
    with m.Matrix(TABLE, [2500000], device=0) as mx:
        mx.add_keys(ctx, True)
        pairs, skipped = mx.run()
        n = pairs
        say(f"# viewpoint contact profiles, one MI355X; data set: {ds.total_groups} synthetic 150 bp read pairs (hg38 names, unc mode, seed 1, the bench's C2 generator), {pairs} resident"
            f" pair records ({skipped} skipped); partners: every other chromosome; either side may be the viewpoint")
        say(f"# per configuration 2 warm-up calls, then {args.reps} calls: median (min .. max) ms.  scan = the two passes over the records (HIP events), sort = radix passes + run lengths (HIP events),"
            f" call = host clock around mkt_matrix_viewpoint (allocations, memsets of the dense tracks, copies back and the host half included)")
        for name, o in (("chrM", dict(vbin=200, pbin=1000000)), ("chr1", dict(vbin=200, pbin=1000000)), ("chr1", dict(vbin=100000, pbin=1000))):
            scan, sort, call = [], [], []
            for k in range(2 + args.reps):
                t0 = time.perf_counter()
                info = mx.viewpoint(name, None, **o)
                t = (time.perf_counter() - t0) * 1e3
                if k >= 2:
                    a, b = mx.viewpoint_timing_ms()
                    scan.append(a); sort.append(b); call.append(t)
            f = lambda v: f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"
            share = 2 * 16 * n / (statistics.median(scan) * 1e-3) / HBM_BYTES_PER_S
            say(f"viewpoint {name:5} vbin {o['vbin']:>7} pbin {o['pbin']:>8}: matching pairs {info.total} ({100.0 * info.total / n:.3f} % of the records), links {info.links}, viewpoint bins {info.viewpoint_bins},"
                f" partner cells {info.partner_cells}, min_loop {info.min_loop}")
            say(f"    scan {f(scan)}   sort {f(sort)}   call {f(call)}")
            say(f"    scan traffic 2 x 16 B x {n} records = {2 * 16 * n / 1e9:.2f} GB -> {2 * 16 * n / (statistics.median(scan) * 1e-3) / 1e12:.2f} TB/s = {100 * share:.0f} % of 8 TB/s")
    ds.close()
    ctx.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
