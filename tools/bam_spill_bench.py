"""sam2bam's out-of-core mode on a synthetic .sam: the executable three ways -- one pass (no -m), -m 2G and -m 512M -- with wall
time, the library's phase marks (MKT_VERBOSE), runs, temporary bytes, peak device bytes; every BAM / BAI is compared with the
single-pass one.
    python tools/bam_spill_bench.py [groups=7500000] [level=2]        (7.5 M groups of the unc profile: ~7 GB of .sam)"""
import filecmp
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import util  # noqa: E402
import test_gpu_bam as T  # noqa: E402
import microcket_amd.build as b  # noqa: E402

groups = int(sys.argv[1]) if len(sys.argv) > 1 else 7500000
level = sys.argv[2] if len(sys.argv) > 2 else "2"
d = os.environ.get("TMPDIR", "/tmp")
sam = os.path.join(d, "spill_bench.sam")
t0 = time.time()
hdr = "".join(f"@SQ\tSN:{c}\tLN:250000000\n" for c in reversed(T.CHROMS)).encode()
size = 0
with open(sam, "wb") as f:                   # in slices, so that the whole text is never in this process either
    f.write(hdr)
    step = 500000
    for g0 in range(0, groups, step):
        part = util.synth("unc", 21, min(step, groups - g0), first=g0, tail=int(g0 + step >= groups))
        f.write(part)
        size += len(part)
print(f"synthetic .sam: {size / 1e9:.2f} GB ({time.time() - t0:.1f} s to make)", flush=True)
ref = None
for label, extra in (("one pass (no -m)", []), ("-m 2G", ["-m", "2G"]), ("-m 512M", ["-m", "512M"])):
    out = os.path.join(d, "spill_bench%s.bam" % ("" if not extra else extra[1]))
    t0 = time.time()
    r = subprocess.run([b.SAM2BAM, "-l", level, *extra, "-T", os.path.join(d, "spill_bench_tmp"), "-o", out, sam],
                       env=dict(os.environ, MKT_VERBOSE="1"), capture_output=True)
    dt = time.time() - t0
    err = r.stderr.decode()
    if r.returncode:
        print(err)
        sys.exit(1)
    m = re.search(r"runs (\d+), temporary bytes (\d+), peak device bytes (\d+)", err)
    runs, tmpb, peak = (int(x) for x in m.groups())
    same = "" if ref is None else ("  equal to the single pass" if filecmp.cmp(ref, out, shallow=False) and
                                   filecmp.cmp(ref + ".bai", out + ".bai", shallow=False) else "  DIFFERS from the single pass")
    print(f"{label:18s} wall {dt:7.2f} s  runs {runs:3d}  temporary {tmpb / 1e9:6.2f} GB  peak device {peak / 1e9:6.2f} GB  "
          f"bam {os.path.getsize(out) / 1e9:.3f} GB{same}", flush=True)
    print("".join("    " + ln + "\n" for ln in err.splitlines() if ln.startswith("[")), flush=True)
    if ref is None:
        ref = out
    else:
        os.remove(out); os.remove(out + ".bai")
    if any(f.startswith("spill_bench_tmp") for f in os.listdir(d)):
        print("temporary files left behind"); sys.exit(1)
os.remove(ref); os.remove(ref + ".bai"); os.remove(sam)
