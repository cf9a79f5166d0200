"""Diagnostic: how long a launch of the lean tile kernel waits for its slowest workgroup (stamp build, never shipped).

    python -c "from microcket_amd import build; build.build_stamps_lib()"
    MKT_LIB=microcket_amd/libmkt_hip_stamps.so python tools/fast_tail.py [pairs] [yes|no] [read_len]

One block per launch, read back after every launch.  On the 100 MHz clock the compute dies share: `wall` = latest end - earliest
first stamp over the launch's workgroups, `span` = a workgroup's end - its first stamp.  wall - mean span is what a perfect dealing
of the same tiles could save (it holds the spread of the starts as well); the HIP-event time of the launch stands beside it.
MKT_TILES=auto probes the tile geometry from the text, as the benchmark does (reads shorter than 150 bp need it).
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import microcket_amd as m

WGS = 1024

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
sam = len(sys.argv) > 2 and sys.argv[2] == "yes"
read_len = int(sys.argv[3]) if len(sys.argv) > 3 else 150
ctx = m.Context("unc", 0.5, 10, sam, 8, device=0, tiles=m.TILES_AUTO if os.environ.get("MKT_TILES") == "auto" else m.TILES_FAST)
ds = ctx.dataset(20260105, 0, pairs, 1 << 21, read_len=read_len)
ctx.L.mkt_debug_spans.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
out = (C.c_ulonglong * 4)()                            # sum of spans, longest span, latest end, 2^62 - earliest start
rows = []
for rep in range(3):
    for (p, n, g) in ds.blocks:
        ctx.reset_timing()
        ctx.submit_device(p, n)
        ctx.sync()
        ctx.L.mkt_debug_spans(ctx.h, out)
        t = ctx.timing()
        if rep == 0:
            continue                                   # (warm-up pass)
        wgs = min(WGS, t.tiles)
        wall = (out[2] - ((1 << 62) - out[3])) / 100.0                         # microseconds
        rows.append(dict(ms=t.tile_kernel_ms, tiles=t.tiles, deferred=t.deferred_tiles, wall=wall, span=out[0] / wgs / 100.0, span_max=out[1] / 100.0))
print(f"read_len {read_len} sam {'yes' if sam else 'no'} pairs {ds.total_groups} launches {len(rows)} (rounds held back: {os.environ.get('MKT_FAST_ROUNDS', 'default')})")
print(f"{'launch':>6s} {'tiles':>6s} {'defer':>5s} {'event us':>9s} {'wall us':>9s} {'mean span':>10s} {'max span':>9s} {'wall-mean span us':>18s} {'% of wall':>9s}")
for i, r in enumerate(rows):
    print(f"{i:6d} {r['tiles']:6d} {r['deferred']:5d} {1000 * r['ms']:9.1f} {r['wall']:9.1f} {r['span']:10.1f} {r['span_max']:9.1f} {r['wall'] - r['span']:18.1f} {100 * (r['wall'] - r['span']) / r['wall']:9.2f}")
n = len(rows)
ev, W, S = (sum(r[k] for r in rows) / n for k in ("ms", "wall", "span"))
print(f"mean per launch: event {1000 * ev:.1f} us, wall {W:.1f} us, mean span {S:.1f} us; wall - mean span = {W - S:.1f} us = {100 * (W - S) / W:.2f} % of the wall, "
      f"{100 * (W - S) / (1000 * ev):.2f} % of the event time")
