"""Cost of reading BAM on the GPU (mkt_bamtext_*) on a BAM that sam2bam wrote from synthetic SAM text (the generator of the
other profiles): per stage the ms the library measures with HIP events (header, index guess, resolve, length, scan, emit), the GB/s of
text, info.repairs, the same at segment_bytes of 64 KiB, 256 KiB and 1 MiB, and beside them the inflate of the same file (mkt_bgzf_*) and
the wall time of bin/bam2sam, so that the share of the inflate in the whole run can be read off.  Nothing is gated on a time.  The
reference's `samtools view -@ 8` is timed on the build host where it lies, never here: the two are set side by side without a ratio.

    python tools/bamtext_bench.py [--groups 4300000] [--out profiles/bamtext_bench.txt]
    python tools/bamtext_bench.py --groups 4300000 --samtools /path/to/samtools --out profiles/bamtext_bench.txt      # appends the yardstick's line
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make_sam(groups):
    import util
    body = util.synth("unc", 5, groups)
    names = set()
    for ln in body.split(b"\n"):
        f = ln.split(b"\t", 7)
        if len(f) > 6:
            names.update((f[2], f[6]))
    hdr = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:250000000\n" % n for n in sorted(names - {b"*", b"="}))
    return hdr, hdr + body


def time_samtools(a):
    """the yardstick, on the host where the reference lies: `samtools view -@ 8 x.bam > /dev/null` on the coordinate-sorted BAM samtools
    itself writes from the same SAM text (its compression differs from sam2bam's; the records are the same)"""
    hdr, sam = make_sam(a.groups)
    with tempfile.TemporaryDirectory(prefix="bamtext_") as tmp:
        bam = os.path.join(tmp, "x.bam")
        subprocess.run([a.samtools, "sort", "-@", "8", "--no-PG", "-o", bam, "-"], input=sam, check=True, stderr=subprocess.DEVNULL)
        lines = sam.count(b"\n") - hdr.count(b"\n")
        del sam
        best = None
        for _ in range(a.runs):
            t0 = time.perf_counter()
            with open(os.devnull, "wb") as null:
                subprocess.run([a.samtools, "view", "-@", "8", bam], stdout=null, check=True)
            w = time.perf_counter() - t0
            best = w if best is None else min(best, w)
        s = f"  beside it, on the build host ({os.cpu_count()} CPUs), not on the GPU machine: samtools 1.17 `view -@ 8 x.bam > /dev/null` on its own sorted BAM of the same {lines} records ({os.path.getsize(bam) / 1e6:.0f} MB): {best:.2f} s wall, best of {a.runs}; no ratio is claimed\n"
    sys.stdout.write(s)
    if a.out:
        with open(a.out, "a") as f:
            f.write(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=2500000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--samtools", default=None, help="time this samtools' `view -@ 8` on a BAM it writes from the same SAM text (no GPU needed), then stop")
    a = ap.parse_args()
    if a.samtools:
        return time_samtools(a)
    import microcket_amd as m
    hdr, sam = make_sam(a.groups)
    bam = m.sam_to_bam(sam, sorted=True, level=2)[0]
    lines = sam.count(b"\n") - hdr.count(b"\n")
    del sam
    out = [f"BAM of sam2bam (sorted, level 2): {lines} records, {len(bam) / 1e6:.0f} MB; one MI355X; best of {a.runs} after a warm-up"]
    with m.BgzfReader() as z:
        z.add(bam)
        best = None
        for run in range(a.runs + 1):
            z.run()
            t = z.timing_ms()
            if run and (best is None or t["inflate"] < best["inflate"]):
                best = t
        d, n = z.device_text()
        out.append(f"  inflate of the file: {best['inflate']:.1f} ms + CRC {best['crc']:.1f} ms for {n / 1e6:.0f} MB of records ({n / best['inflate'] / 1e6:.2f} GB/s)")
        inflate_ms = best["inflate"] + best["crc"]
        for seg in (64 << 10, 256 << 10, 1 << 20):
            res = []
            with m.BamReader() as r:
                for run in range(a.runs + 1):
                    r.add_device(d, n)
                    info = r.run(segment_bytes=seg)
                    r.finish()
                    if run:
                        res.append(r.timing_ms())
            t = min(res, key=lambda x: sum(x.values()))
            dev = sum(t.values())
            out.append(f"  segment_bytes {seg >> 10} KiB: {info.records} records, {info.text_bytes / 1e6:.0f} MB of text, {info.segments} segments, repairs {info.repairs}; on the device {dev:.1f} ms "
                       f"({info.text_bytes / dev / 1e6:.2f} GB/s of text): " + ", ".join(f"{k} {v:.2f}" for k, v in t.items()))
            out.append(f"    emit {t['emit']:.1f} ms against the inflate of the same records {inflate_ms:.1f} ms; decode stages / (inflate + decode) = {dev / (dev + inflate_ms):.2f}")
    exe = os.path.join(os.path.dirname(m.lib_path()), "bin", "bam2sam")
    with tempfile.TemporaryDirectory(prefix="bamtext_") as tmp:
        src = os.path.join(tmp, "x.bam")
        with open(src, "wb") as f:
            f.write(bam)
        best = None
        for _ in range(a.runs):
            t0 = time.perf_counter()
            with open(os.devnull, "wb") as null:
                p = subprocess.run([exe, src], stdout=null, stderr=subprocess.PIPE)
            w = time.perf_counter() - t0
            assert p.returncode == 0, p.stderr.decode()
            best = w if best is None else min(best, w)
        out.append(f"  bin/bam2sam x.bam > /dev/null (file in the page cache): {best:.2f} s wall")
    s = "\n".join(out) + "\n"
    sys.stdout.write(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
