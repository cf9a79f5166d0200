"""Cost of final.pairs.gz + .px2 on the GPU (mkt_pairsgz_*) on a synthetic sorted final.pairs of 10 M lines (one block
of 100 000 records with ascending pos1, repeated under 100 different chromosome pairs): the five phase times the library measures
with HIP events, the whole Python call and the wall time of bin/pairsbgz.  With --reference DIR (a host that has the reference's
binaries; no GPU needed with --reference-only) the wall time of `bgzip -@ 8 -c | pairix` on the same file.

    python tools/pairsgz_bench.py [--lines 10000000] [--level 1] [--reference DIR [--reference-only]] [--out profiles/pairsgz_bench.txt]
"""
import argparse
import os
import platform
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCK = 100000
HEADER = b"## pairs format v1.0\n#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"


def make_input(lines):
    block = b"".join(b"K84:1101:%07d:XXXXXX\tchrAA\t%d\tchrBB\t%d\t%s\t%s\n" % (i, 1 + i * 1987 + i % 13, 1 + (i * 7919) % 190000000, b"+-"[i & 1:(i & 1) + 1], b"-+"[i % 3 & 1:(i % 3 & 1) + 1])
                     for i in range(BLOCK))
    reps = max(1, lines // BLOCK)
    names = [(a, b) for a in range(1, 24) for b in range(a, 24)][:reps]
    return HEADER + b"".join(block.replace(b"chrAA", b"chr%d" % a).replace(b"chrBB", b"chr%d" % b) for a, b in names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--reference-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = make_input(a.lines)
    out = [f"final.pairs: {text.count(10)} lines, {len(text) / 1e6:.0f} MB, sorted, {max(1, a.lines // BLOCK)} chromosome pairs"]
    with tempfile.TemporaryDirectory(prefix="pairsgz_") as d:
        src = os.path.join(d, "final.pairs")
        with open(src, "wb") as f:
            f.write(text)
        if not a.reference_only:
            import microcket_amd as m
            exe = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairsbgz")
            res = []
            for run in range(a.runs + 1):                # run 0 warms up
                with m.PairsGz() as g:
                    t0 = time.perf_counter()
                    g.add(text)
                    t1 = time.perf_counter()
                    info = g.run(level=a.level)
                    dt = time.perf_counter() - t0
                    tm = g.timing_ms()
                if run:
                    res.append((dt, t1 - t0, tm))
            dt, tadd, tm = min(res, key=lambda r: r[0])
            dev = sum(tm.values())
            out.append(f"  level {a.level}: {info.blocks} blocks, .gz {info.gz_bytes / 1e6:.1f} MB, .px2 {info.px2_bytes} bytes; {info.names} names, {info.chunks} chunks")
            out.append(f"  library on one MI355X, best of {a.runs}: whole call {dt * 1e3:.1f} ms (copying the text in {tadd * 1e3:.1f} ms); on the device {dev:.1f} ms: deflate + pack {tm['deflate']:.1f}, "
                       f"line index {tm['line_index']:.1f}, per-line kernel {tm['lines']:.1f}, names + chunks (scans, name table, host check) {tm['names_chunks']:.1f}, index serialised + deflated {tm['index']:.1f} ms")
            best = None
            for _ in range(a.runs):
                t0 = time.perf_counter()
                p = subprocess.run([exe, "-f", "-l", str(a.level), src, os.path.join(d, "ours.pairs.gz")], stderr=subprocess.PIPE)
                w = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr.decode()
                best = w if best is None else min(best, w)
            out.append(f"  bin/pairsbgz -l {a.level} final.pairs ours.pairs.gz (file in the page cache), best of {a.runs}: {best:.2f} s wall")
        if a.reference:
            gz = os.path.join(d, "ref.pairs.gz")
            t0 = time.perf_counter()
            with open(gz, "wb") as f:
                subprocess.run([os.path.join(a.reference, "bin", "bgzip"), "-@", "8", "-c", src], stdout=f, check=True)
            t1 = time.perf_counter()
            subprocess.run([os.path.join(a.reference, "bin", "pairix"), "-f", gz], check=True)
            t2 = time.perf_counter()
            out.append(f"  the reference on host {platform.node()} ({os.cpu_count()} CPUs, no GPU; NOT the host of the lines above), one run: bgzip -@ 8 -c {t1 - t0:.2f} s + pairix {t2 - t1:.2f} s = {t2 - t0:.2f} s wall"
                       f" (.gz {os.path.getsize(gz) / 1e6:.1f} MB)")
    s = "\n".join(out) + "\n"
    sys.stdout.write(s)
    if a.out:
        with open(a.out, "a") as f:
            f.write(s)


if __name__ == "__main__":
    main()
