#!/usr/bin/env python3
"""One short run through the C ABI's resident path and two of its extensions, for counting HIP API calls:

    rocprofv3 --hip-trace --stats -- python tools/capi_calls.py

One context with MKT_EXT_KEYS, a data set of 8 blocks of 2^16 groups, submit_device of every block, finish, ext_dedup,
ext_chrstat, close.  The calls per HIP API name of two builds of the library (MKT_LIB selects another one) are compared in
profiles/capi_layers.txt: a change of the host side that is meant to move nothing leaves every count as it was."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import microcket_amd as m

BLOCKS, GROUPS_PER_BLOCK = 8, 1 << 16

with m.Context("unc", 0.5, 10, False, 8, device=0, extensions=m.EXT_KEYS) as ctx:
    ds = ctx.dataset(20260105, 0, BLOCKS * GROUPS_PER_BLOCK, GROUPS_PER_BLOCK)
    assert ds.n_blocks == BLOCKS, ds.n_blocks
    for (p, n, g) in ds.blocks:
        ctx.submit_device(p, n)
    st = ctx.finish(True)
    total, dups, _ = ctx.ext_dedup(True, want_flags=False)
    chrstat = ctx.ext_chrstat(True)
    ds.close()
print(f"capi_calls: {ds.n_blocks} blocks, {ds.total_bytes} bytes, {st.groups} groups, {st.pairs} pairs, {total} keys, {dups} duplicates, "
      f"{len(chrstat.splitlines())} chromosome pairs")
