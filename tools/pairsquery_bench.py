"""Cost of region queries through the .px2 on the GPU (mkt_bgzf_query) on the synthetic sorted final.pairs of
tools/pairsgz_bench.py (10 M lines, 100 chromosome pairs), compressed and indexed by this project's PairsGz at levels 1 and 2.
Batches of 1, 100 and 10 000 regions of about 1 Mb x 1 Mb, by both routes: without `run` (only the members the index points to are
inflated) and after `run` (the resident text).  Per batch: members inflated out of the file's, the two phase times the library
measures with HIP events (plan upload + inflate + CRC of the selected members; line index + filter + scan + gather), the whole Python
call (answer fetched to the host) and the wall time of bin/pairsquery -L.  The whole-file run() of the same build is the yardstick.
Times are the best of --runs after one warm-up call; nothing is asserted.

    python tools/pairsquery_bench.py [--lines 10000000] [--levels 1,2] [--out profiles/pairsquery_bench.txt]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pairsgz_bench  # noqa: E402

MB = 1000000


def make_regions(n, reps):
    """n regions of 1 Mb x 1 Mb spread over the pairs of the file and over their positions (deterministic)"""
    names = [(a, b) for a in range(1, 24) for b in range(a, 24)][:reps]
    out = []
    for k in range(n):
        a, b = names[(k * 37) % len(names)]
        s1, s2 = ((k * 7919) % 198) * MB, ((k * 104729) % 189) * MB
        out.append("chr%d:%d-%d|chr%d:%d-%d" % (a, s1 + 1, s1 + MB, b, s2 + 1, s2 + MB))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10000000)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batches", default="1,100,10000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import microcket_amd as m
    exe = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairsquery")
    text = pairsgz_bench.make_input(a.lines)
    reps = max(1, a.lines // pairsgz_bench.BLOCK)
    out = [f"final.pairs: {text.count(10)} lines, {len(text) / 1e6:.0f} MB, sorted, {reps} chromosome pairs; regions of 1 Mb x 1 Mb; one MI355X, best of {a.runs}"]
    with tempfile.TemporaryDirectory(prefix="pairsquery_") as d:
        for level in (int(x) for x in a.levels.split(",")):
            with m.PairsGz() as g:
                g.add(text)
                g.run(level=level)
                gz, px2 = g.gz_bytes(), g.px2_bytes()
            path = os.path.join(d, "l%d.pairs.gz" % level)
            with open(path, "wb") as f:
                f.write(gz)
            with open(path + ".px2", "wb") as f:
                f.write(px2)
            with m.BgzfReader() as r:
                r.add(gz)
                r.load_index(px2)
                runs = []
                for _ in range(a.runs + 1):
                    t0 = time.perf_counter()
                    info = r.run()
                    runs.append((time.perf_counter() - t0, r.timing_ms()))
                dt, tm = min(runs[1:], key=lambda x: x[0])
                out.append(f" level {level}: .gz {len(gz) / 1e6:.1f} MB in {info.blocks} members, .px2 {len(px2)} bytes; whole-file run(): {dt * 1e3:.1f} ms (inflate {tm['inflate']:.1f}, CRC {tm['crc']:.1f} ms on the device)")
            for nreg in (int(x) for x in a.batches.split(",")):
                regions = make_regions(nreg, reps)
                lst = os.path.join(d, "regions.txt")
                with open(lst, "w") as f:
                    f.write("".join(q + "\n" for q in regions))
                answers = []
                for route in ("selected members", "resident text"):
                    with m.BgzfReader() as r:
                        r.add(gz)
                        r.load_index(px2)
                        if route == "resident text":
                            r.run()
                        res = []
                        for _ in range(a.runs + 1):
                            t0 = time.perf_counter()
                            ans = r.query(regions)
                            res.append((time.perf_counter() - t0, r.query_timing_ms()))
                        qi = r.query_info
                        answers.append(ans)
                    dt, tm = min(res[1:], key=lambda x: x[0])
                    out.append(f"  {nreg:5d} regions, {route}: {qi.blocks_inflated} of {info.blocks} members inflated ({qi.bytes_inflated / 1e6:.1f} MB), {qi.chunks} chunks, {qi.candidate_lines} candidate lines, "
                               f"{qi.lines} lines answered ({qi.answer_bytes / 1e6:.2f} MB); plan upload + inflate + CRC {tm['inflate_selected']:.2f} ms, line index + filter + scan + gather {tm['filter_gather']:.2f} ms, "
                               f"whole call {dt * 1e3:.1f} ms")
                assert answers[0] == answers[1]
                best = None
                for _ in range(a.runs):
                    t0 = time.perf_counter()
                    p = subprocess.run([exe, "-L", path, lst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                    w = time.perf_counter() - t0
                    assert p.returncode == 0 and p.stdout == b"".join(answers[0]), p.stderr.decode()
                    best = w if best is None else min(best, w)
                out.append(f"  {nreg:5d} regions, bin/pairsquery -L (process start, both files read from the page cache, the .gz copied to the device): {best:.2f} s wall")
    s = "\n".join(out) + "\n"
    sys.stdout.write(s)
    if a.out:
        with open(a.out, "a") as f:
            f.write(s)


if __name__ == "__main__":
    main()
