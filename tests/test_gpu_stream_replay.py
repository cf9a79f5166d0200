"""The streaming replay (mkt_capi.cpp: stream_replay) on inputs that overflow the REAL sizing rules of the device buffers.

The streaming path sizes its buffers from guesses; the kernels check the real counts, an overflowing tile writes nothing, and the
worker repairs the cause and launches the failed job again, with every job queued behind it.  Every case here
  * asserts on the CPU, from the oracle's output and the sizing rule restated below, that the first attempt cannot fit,
  * runs the input and compares with the CPU oracle: .log byte for byte (quirk Q2 makes the logged selfCircle depend on the global
    group index, so a wrong group offset after rewind_run shows there), groups, pairs, pair_bytes, .pairs / .sam byte-equal in
    ordered mode and equal as line multisets (length + order-independent checksum of the lines) in any-order mode,
  * asserts from Context.replays() that the cause it is about was repaired: a case that takes no replay fails.
Nothing here provokes a fault: every overflow is one the kernels detect and report by design.

The sizing rules (mkt_capi.cpp), B = block_bytes, a buffer of `need` bytes being allocated with an eighth and a page of slack:
    .pairs  need = B // 3 + 65536                      16 equal regions in any-order mode, one region in ordered mode
    .sam    need = B + B // 4 + 65536                  likewise
    self-circle slices, per block of n bytes: regions * ((n // 256 // regions) * 2 + 1024) entries, no slack
"""
import functools

import numpy as np
import pytest

import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

REGIONS = 16


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device: the HIP path is the only path (no CPU fallback to test)")


def _alloc(need):
    return need + need // 8 + 4096          # ensure_dev


def pairs_cap(B):
    return _alloc(B // 3 + 65536)


def sam_cap(B):
    return _alloc(B + B // 4 + 65536)


def sc_slices(n, regions):
    return regions * ((n // 256 // regions) * 2 + 1024)


def lean_tile(avg):
    """mkt_fast.h lean_dims(): bytes per tile of the lean kernel for lines of `avg` bytes"""
    avg = min(max(avg, 48.0), 4096.0)
    r16 = lambda x: (int(x) + 15) & ~15
    hb = min(max(r16(7.5 * avg), 256), 3072)
    hf = min(max(r16(8.75 * avg), 512), 4096)
    w = 126 * avg
    t = min(r16(w - (hb + hf)) if w > hb + hf + 2048 else 2048, 49152)
    rem = (hb + t + hf) & 1023
    return t + 1024 - rem if rem >= 512 and t + 1024 - rem <= 49152 else t - rem


# ---- inputs: a few line templates, repeated.  Names only differ between neighbouring groups; the last group of a chunk and the first
# ---- group of the next repetition are differently named.
def _dense_chunk(groups=64):
    """read names of 120 bytes on 8-base reads, all cis10K: .pairs bytes are 0.43 of the input"""
    rows = []
    for g in range(groups):
        name = f"d{g:03d}:" + "N" * 115
        a = 100000 + 977 * g
        b = a + 20000 + 13 * g
        rows.append(f"{name}\t65\tchr1\t{a}\t60\t8M\t=\t{b}\t0\tACGTACGT\tFFFFFFFF\n")
        rows.append(f"{name}\t129\tchr1\t{b}\t60\t8M\t=\t{a}\t0\tACGTACGT\tFFFFFFFF\n")
    return "".join(rows).encode()


def _pe150_chunk(tag, mapq, groups=64):
    """150-base pairs, every line surviving at MAPQ 60 (none at MAPQ 0), cis10K on chr2"""
    seq, qual = "ACGTTGCAAC" * 15, "F" * 150
    rows = []
    for g in range(groups):
        a = 500000 + 1013 * g
        b = a + 30000 + 7 * g
        rows.append(f"{tag}{g:03d}\t65\tchr2\t{a}\t{mapq}\t150M\t=\t{b}\t0\t{seq}\t{qual}\tNM:i:0\n")
        rows.append(f"{tag}{g:03d}\t129\tchr2\t{b}\t{mapq}\t150M\t=\t{a}\t0\t{seq}\t{qual}\tNM:i:0\n")
    return "".join(rows).encode()


def _tiny_chunk(mapq=60, selfcircle=True, groups=64):
    """groups of two ~33-byte lines on chr1: 5' ends 4 apart (a self-circle, no pair) or 8000 apart (cis1K, a reported pair)"""
    rows = []
    for g in range(groups):
        a = 1000 + g
        b = a + (4 if selfcircle else 8000)
        rows.append(f"t{g:02d}\t65\tchr1\t{a}\t{mapq}\t5M\t=\t1\t0\tA\tF\n")
        rows.append(f"t{g:02d}\t129\tchr1\t{b}\t{mapq}\t5M\t=\t1\t0\tA\tF\n")
    return "".join(rows).encode()


class _Input:
    def __init__(self, text):
        self.text = text
        self._o = {}

    def oracle(self, T=4, sam=True):
        if (T, sam) not in self._o:
            self._o[(T, sam)] = util.oracle_run(self.text, "unc", T, 0.5, 10, sam)
        return self._o[(T, sam)]


PAIRS_B = 4 << 20


@functools.lru_cache(maxsize=None)
def pairs_input():
    """two and a bit blocks of ordinary 150 bp text, three blocks' worth of the dense reads, ordinary text again"""
    head, tail = util.synth("unc", 31, 10000, tail=0), util.synth("unc", 32, 4000, tail=1, first=10000)
    assert len(head) > 2 * PAIRS_B
    d = _dense_chunk()
    return _Input(head + d * (3 * PAIRS_B // len(d) + 1) + tail), len(head), d


def _dense_cannot_fit(B, d):
    """any block cut wholly from the dense stretch holds at least B - (one group + one line) bytes, i.e. that many whole chunks less
    one: their .pairs bytes alone exceed the whole buffer (so some region overflows whatever the split among the regions)"""
    per_chunk = len(util.oracle_run(d + d, "unc", 4, 0.5, 10, False)[0]) // 2          # (twice: quirk Q1 drops the input's last group)
    whole = (B - 3 * 170) // len(d) - 1
    assert per_chunk * whole > pairs_cap(B) > B // 3 + 65536, (per_chunk, whole, pairs_cap(B))


def _compare(got, want, ordered, tag):
    p, s, st, log = got
    po, so, lo, ost = want
    assert log == lo, (tag, log, lo)
    assert st.groups == ost.groups and st.pairs == ost.pairs and st.pair_bytes == len(po), tag
    if ordered:
        assert p == po and s == so, tag
    else:
        assert len(p) == len(po) and util.lines_checksum(p) == util.lines_checksum(po), tag
        assert len(s) == len(so) and util.lines_checksum(s) == util.lines_checksum(so), tag


def _repairs(r):
    return r.geometry + r.pairs_cap + r.sam_cap + r.sc_cap


@pytest.mark.parametrize("ordered", [True, False])
def test_pairs_overflow_in_mid_stream_reruns_the_queued_job(ordered):
    """block_bytes = 4 MiB, MKT_TILES_AUTO, pieces of 11 MiB + 1 byte.  The dense blocks report 0.43 of their bytes as .pairs, the
    buffer holds 0.39: E_PAIRS_CAP on the third block or later.  jobs_rerun > repairs: at least one job was launched again only
    because it was queued behind the failing one.  At most two jobs are in flight, and the next block has to be queued before the
    worker sees the failed result: with pieces of 1 300 001 bytes (a drain between any two blocks) that never happened on the
    MI355X at 4 MiB or 2 MiB blocks, ordered or not; with pieces that span two blocks and more (one mkt_submit call cuts and queues
    them back to back) it happened in every run at 4 MiB, so the blocks did not have to shrink.  Since the pipeline decides, the
    input is run up to four times: every run is checked in full against the oracle, and one of them must have re-run a queued job."""
    _need_gpu()
    inp, head, d = pairs_input()
    _dense_cannot_fit(PAIRS_B, d)
    want = inp.oracle(4, False)
    seen = []
    for attempt in range(4):
        with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=PAIRS_B, ordered=ordered) as c:
            got = c.run_bytes(inp.text, chunk=(11 << 20) + 1)
            r = c.replays()
        seen.append(r)
        print("pairs overflow, ordered" if ordered else "pairs overflow, any order", r)
        _compare(got, want, ordered, (ordered, r))
        assert r.pairs_cap >= 1 and r.sam_cap == 0, r
        if r.jobs_rerun > _repairs(r):
            break
    assert seen[-1].jobs_rerun > _repairs(seen[-1]), seen


SAM_B = 1 << 17


@functools.lru_cache(maxsize=None)
def sam_input():
    """five blocks of MAPQ 0 lines (no .sam at all), then four blocks of 150-base pairs whose every line survives"""
    lo, hi = _pe150_chunk("q", 0), _pe150_chunk("r", 60)
    return _Input(lo * (5 * SAM_B // len(lo)) + hi * (4 * SAM_B // len(hi)) + _pe150_chunk("z", 60, 2)), lo, hi


def test_sam_overflow_by_region_imbalance():
    """block_bytes = 128 KiB, any-order, .sam on: a block is three tiles in three of the 16 regions; a region owns 16 KiB of .sam and a
    tile whose lines all survive writes its ~43 KiB into one of them: E_SAM_CAP, on the first block behind the MAPQ 0 stretch (the
    sixth).  The same input in ordered mode never repairs .sam: one region of 1.25 x the block always fits (.sam <= input)."""
    _need_gpu()
    inp, lo, hi = sam_input()
    line = len(hi) // 128
    rcap = sam_cap(SAM_B) // REGIONS & ~15
    tile = lean_tile(len(lo) / 128)
    assert tile < SAM_B and tile - 2 * line > rcap, (tile, rcap)             # a tile's own lines, less the two at its ends
    assert sam_cap(SAM_B) >= SAM_B + 1                                       # ordered: one region holds any block's .sam
    assert inp.text.find(b"r000\t") > 4 * SAM_B                              # the first surviving line is in the fifth block or later
    want = inp.oracle(4, True)
    assert len(want[1]) > 3 * SAM_B
    for ordered in (False, True):
        with m.Context("unc", 0.5, 10, True, 4, device=0, block_bytes=SAM_B, ordered=ordered) as c:
            got = c.run_bytes(inp.text, chunk=70001)
            r = c.replays()
        print("sam overflow, ordered" if ordered else "sam overflow, any order", r)
        _compare(got, want, ordered, (ordered, r))
        if ordered:
            assert r.sam_cap == 0 and r.pairs_cap == 0 and r.sc_cap == 0, r
        else:
            assert r.sam_cap >= 1, r


SC_B = 8 << 20


@functools.lru_cache(maxsize=None)
def sc_input(with_head):
    """more than three blocks of self-circle groups of two ~33-byte lines; with_head: one block and 64 KiB of 150 bp text in front"""
    t = _tiny_chunk()
    head = b""
    if with_head:
        head = util.synth("unc", 33, 12000, tail=0)
        head = head[:head.rfind(b"\n", 0, SC_B + 65536) + 1]          # (wherever that cuts a group: the oracle sees the same bytes)
    return _Input(head + t * (3 * SC_B // len(t) + 500)), head, t


@pytest.mark.parametrize("with_head", [True, False])
def test_self_circle_slices_overflow(with_head):
    """block_bytes = 8 MiB, any-order.  A block of n bytes of these groups holds n / 66 self-circle entries; its slices hold
    n / 128 + 16384, a sixteenth of that per region.
    with_head: the geometry was chosen for 150 bp lines, so the second block (64 KiB of them, then tiny lines) overflows the line
    table first and its self-circle slices on the attempt after: `geometry` and `sc_cap` on the same job.
    without: the geometry is chosen for the tiny lines themselves and holds, only `sc_cap` fires (on the first job).  No line length
    gives sc_cap alone behind a longer-lined head: more than one entry per 128 bytes needs lines under 64 bytes, and a window chosen
    for >= 7 times longer lines then always overflows the 512-line table.
    The .log must match for ref_threads 2 and 8 (quirk Q2: the logged count depends on the global group indices)."""
    _need_gpu()
    inp, head, t = sc_input(with_head)
    per_chunk = util.oracle_run(t + t, "unc", 4, 0.5, 10, False)[3].selfCircle_all // 2
    assert per_chunk >= 63
    whole = (SC_B - 200) // len(t) - 1                                          # whole chunks in any block cut from the tiny lines
    assert per_chunk * whole > sc_slices(SC_B, REGIONS) == SC_B // 128 + 16384, (per_chunk * whole, sc_slices(SC_B, REGIONS))
    assert len(inp.text) - len(head) > 3 * SC_B
    if with_head:
        assert SC_B < len(head) < SC_B + (1 << 17)
        assert lean_tile(len(head) / head.count(b"\n")) // 34 > 512                # 150 bp geometry: more tiny lines per tile than the line table holds
    for T in (2, 8):
        want = inp.oracle(T, False)
        with m.Context("unc", 0.5, 10, False, T, device=0, block_bytes=SC_B) as c:
            got = c.run_bytes(inp.text, chunk=3000017)
            r = c.replays()
        print("self-circle overflow", "behind 150 bp text" if with_head else "alone", T, r)
        _compare(got, want, False, (with_head, T, r))
        assert got[2].selfCircle_all == want[3].selfCircle_all > 3 * per_chunk * whole
        assert r.sc_cap >= 1 and r.pairs_cap == 0 and r.sam_cap == 0, r
        assert (r.geometry >= 1) == with_head, r
        assert r.jobs_rerun >= _repairs(r), r


def test_keys_survive_a_replay_none_twice_none_lost():
    """The .pairs-overflow input with MKT_EXT_KEYS: the jobs that are run again place their key records again, on top of run totals
    that were rewound.  The key list must hold every reported pair once (ordinals 0 .. n-1), and duplicate marking and the
    chromosome statistics must equal those of a control context that takes the same bytes as one block (no replay: its counters
    are all zero)."""
    _need_gpu()
    inp, head, d = pairs_input()
    _dense_cannot_fit(PAIRS_B, d)
    want = inp.oracle(4, False)
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=64 << 20, extensions=m.EXT_KEYS) as c:
        assert len(inp.text) < (64 << 20) and 2 * len(want[0]) < pairs_cap(64 << 20)      # one block, room for any imbalance among the regions
        ctl = c.run_bytes(inp.text)
        ctl_dedup, ctl_chr, ctl_keys, r0 = c.ext_dedup(True), c.ext_chrstat(True), c.ext_keys_fetch(True), c.replays()
    assert r0 == (0, 0, 0, 0, 0), r0
    _compare(ctl, want, False, "control")
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=PAIRS_B, extensions=m.EXT_KEYS) as c:
        got = c.run_bytes(inp.text, chunk=(11 << 20) + 1)
        r = c.replays()
        n, keys, dedup, chrstat = c.ext_key_count(True), c.ext_keys_fetch(True), c.ext_dedup(True), c.ext_chrstat(True)
    print("keys across a replay", r)
    _compare(got, want, False, r)
    assert r.pairs_cap >= 1, r
    assert n == got[2].pairs == want[3].pairs == keys.shape[0]
    assert np.array_equal(keys[:, 2], np.arange(n, dtype=np.uint64))
    assert np.array_equal(keys[:, 1], ctl_keys[:, 1]) and np.array_equal(keys[:, 0] & np.uint64(0xFFFFFFFF), ctl_keys[:, 0] & np.uint64(0xFFFFFFFF))
    assert dedup == ctl_dedup and chrstat == ctl_chr
    assert dedup[0] == n and dedup[2] == util.expected_dups(want[0])


KEY_PERIOD = 64


def test_key_list_grows_past_its_first_reservation():
    """More than 2^22 + 2^20 reported pairs from ~33-byte lines (one pair per 66 input bytes), the first fifth of the input at MAPQ 0:
    the run's key list starts at 2^22 records and has to grow while holding the records of the blocks already folded, on a
    reservation made from a density that the first blocks understate.  The key array must be periodic as the input is.
    These lines also report 0.45 of their bytes as .pairs, so the first surviving 64 MiB block overflows the .pairs buffer (0.38 of
    a block): the key records of that block are placed twice, by the failed attempt's successor.  As observed on the MI355X
    (profiles/stream_replay_tests.txt): pairs_cap = 1, and the key-list reservation held -- growth by doubling, no sc_cap replay."""
    _need_gpu()
    hi, lo = _tiny_chunk(60, selfcircle=False, groups=KEY_PERIOD), _tiny_chunk(0, selfcircle=False, groups=KEY_PERIOD)
    n_hi = ((1 << 22) + (1 << 20) + 4096) // KEY_PERIOD + 1
    text = lo * (n_hi // 4) + hi * n_hi
    po, so, lo_log, ost = util.oracle_run(text, "unc", 4, 0.5, 10, False)
    assert ost.pairs == n_hi * KEY_PERIOD - 1 > (1 << 22) + (1 << 20)       # (quirk Q1: the input's last group is dropped)
    B = 64 << 20                                                            # the default block; whole periods of any block cut from `hi`:
    assert len(hi) * n_hi > 3 * B and (len(po) // n_hi) * ((B - 200) // len(hi) - 1) > pairs_cap(B)
    with m.Context("unc", 0.5, 10, False, 4, device=0, extensions=m.EXT_KEYS) as c:
        p, s, st, log = c.run_bytes(text, chunk=48 << 20)
        r = c.replays()
        n, keys, chrstat = c.ext_key_count(True), c.ext_keys_fetch(True), c.ext_chrstat(True)
    print("key list past 2^22", r)
    assert log == lo_log and st.pairs == ost.pairs and st.groups == ost.groups and st.pair_bytes == len(po)
    assert len(p) == len(po) and util.lines_checksum(p) == util.lines_checksum(po)
    assert n == ost.pairs == keys.shape[0]
    assert np.array_equal(keys[:, 2], np.arange(n, dtype=np.uint64))
    assert np.array_equal(keys[KEY_PERIOD:, :2], keys[:-KEY_PERIOD, :2])
    assert len(np.unique(keys[:KEY_PERIOD, 1])) == KEY_PERIOD                  # ... and a period holds 64 different records
    assert chrstat == b"chr1\tchr1\t%d\n" % ost.pairs
    assert r.pairs_cap >= 1 and r.sam_cap == 0, r
    assert r.sc_cap == 0, r                                                     # the reservation held: the list grew by doubling, records kept


def test_resident_path_does_not_repair_a_capacity_error():
    """mkt_sync replays geometry only.  Self-circle groups of ~33-byte lines as device blocks: a block of n bytes holds n / 66 entries,
    mkt_submit_device's slices hold n / 128 + 16384 (the run's list, sc_estimate, is sized at one entry per 64 bytes before a sync
    has shown the density, and is never what overflows here).  512 KiB blocks fit and give the oracle's statistics; an 8 MiB block
    does not fit and raises an error that names the self-circle buffer -- it never returns counters."""
    _need_gpu()
    t = _tiny_chunk()
    small, big = t * ((1 << 19) // len(t)), t * ((8 << 20) // len(t))
    per_chunk = util.oracle_run(t + t, "unc", 4, 0.5, 10, False)[3].selfCircle_all // 2
    assert 2 * per_chunk * (len(small) // len(t)) // REGIONS < sc_slices(len(small), REGIONS) // REGIONS      # twice a region's share: room for imbalance
    assert per_chunk * (len(big) // len(t)) > sc_slices(len(big), REGIONS)
    text = small * 3
    po, so, lo, ost = util.oracle_run(text, "unc", 4, 0.5, 10, False)
    with m.Context("unc", 0.5, 10, False, 4, device=0) as c:
        for _ in range(3):
            c.submit_device(c.device_text(small), len(small))
        st = c.finish(True)
        assert c.format_log(st) == lo and st.groups == ost.groups and st.selfCircle_all == ost.selfCircle_all and st.pairs == 0
        assert c.replays() == (0, 0, 0, 0, 0)
    with m.Context("unc", 0.5, 10, False, 4, device=0) as c:
        with pytest.raises(m.MktError, match="self-circle buffer"):
            c.submit_device(c.device_text(small), len(small))
            c.submit_device(c.device_text(big), len(big))
            c.submit_device(c.device_text(small), len(small))
            c.finish(True)
        r = c.replays()
        assert r.sc_cap == 0 and r.jobs_rerun == 0, r
