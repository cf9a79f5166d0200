"""Cost of reading BGZF back on the GPU (mkt_bgzf_*) on the synthetic sorted final.pairs of tools/pairsgz_bench.py (10 M
lines, 575 MB), compressed by this project's own writer (PairsGz, levels 1 and 2) and by Python's zlib at level 6 in BGZF framing: the
phase times the library measures with HIP events (table upload, inflate, CRC) with the GB/s of text, the whole library call, the wall
time of bin/pairsgunzip, and beside them on the same machine and file Python's zlib.decompress per block on one core (the library
`bgzip -d` uses).  Nothing is gated on a time.  Region queries are not built, so no query batch is measured.

    python tools/inflate_bench.py [--lines 10000000] [--out profiles/inflate_bench.txt]
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from pairsgz_bench import make_input  # noqa: E402

RAW = 0xFF00
EOF = bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 0x42, 0x43, 2, 0, 0x1B, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def zlib_bgzf(text, level):
    out = []
    for a in range(0, len(text), RAW):
        piece = text[a:a + RAW]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = co.compress(piece) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
    out.append(EOF)
    return b"".join(out)


def zlib_inflate_one_core(gz):
    t0 = time.perf_counter()
    p = n = 0
    while p < len(gz):
        bsize = struct.unpack_from("<H", gz, p + 16)[0] + 1
        d = zlib.decompress(gz[p + 18:p + bsize - 8], -15)
        assert zlib.crc32(d) == struct.unpack_from("<I", gz, p + bsize - 8)[0]
        n += len(d)
        p += bsize
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import microcket_amd as m
    text = make_input(a.lines)
    out = [f"final.pairs: {text.count(10)} lines, {len(text) / 1e6:.0f} MB, sorted (the file of profiles/pairsgz_bench.txt); one MI355X; best of {a.runs} after a warm-up"]
    files = []
    for level in (1, 2):
        with m.PairsGz() as g:
            g.add(text)
            g.run(level=level)
            files.append((f"bin/pairsbgz -l {level}", g.gz_bytes()))
    files.append(("zlib level 6, BGZF framing", zlib_bgzf(text, 6)))
    exe = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairsgunzip")
    with tempfile.TemporaryDirectory(prefix="inflate_") as d:
        for name, gz in files:
            res = []
            for run in range(a.runs + 1):
                with m.BgzfReader() as r:
                    t0 = time.perf_counter()
                    r.add(gz)
                    t1 = time.perf_counter()
                    info = r.run()
                    dt = time.perf_counter() - t0
                    tm = r.timing_ms()
                    if run == 0:
                        assert r.text() == text
                if run:
                    res.append((dt, t1 - t0, tm))
            dt, tadd, tm = min(res, key=lambda x: x[0])
            dev = sum(tm.values())
            out.append(f"  {name}: .gz {len(gz) / 1e6:.1f} MB, {info.blocks} blocks, deflate blocks stored/fixed/dynamic {info.stored}/{info.fixed}/{info.dynamic}")
            out.append(f"    library: whole call {dt * 1e3:.1f} ms (copying the .gz in {tadd * 1e3:.1f} ms); on the device {dev:.1f} ms: table upload {tm['table_upload']:.2f}, "
                       f"inflate {tm['inflate']:.1f} ({len(text) / tm['inflate'] / 1e6:.1f} GB/s of text), CRC {tm['crc']:.1f} ({len(text) / tm['crc'] / 1e6:.1f} GB/s)")
            src = os.path.join(d, "in.pairs.gz")
            with open(src, "wb") as f:
                f.write(gz)
            best = None
            for _ in range(a.runs):
                t0 = time.perf_counter()
                p = subprocess.run([exe, src, os.path.join(d, "out.pairs")], stderr=subprocess.PIPE)
                w = time.perf_counter() - t0
                assert p.returncode == 0, p.stderr.decode()
                best = w if best is None else min(best, w)
            out.append(f"    bin/pairsgunzip in.pairs.gz out.pairs (file in the page cache): {best:.2f} s wall")
            tz, n = zlib_inflate_one_core(gz)
            assert n == len(text)
            out.append(f"    beside it, same machine and file: Python zlib.decompress + crc32 per block on one core {tz:.2f} s ({len(text) / tz / 1e9:.2f} GB/s)")
    out.append("  for scale: the GPU deflate wrote this text in 11.7 ms at level 1 (profiles/pairsgz_bench.txt, deflate and pack).  No ratio against the reference's bgzip is claimed:")
    out.append("  it does not exist on the GPU machine.  Region queries through the .px2 are not built yet, so no query batch is measured.")
    s = "\n".join(out) + "\n"
    sys.stdout.write(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
