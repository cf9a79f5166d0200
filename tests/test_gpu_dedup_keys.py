"""Duplicate marking of caller-supplied key records (Context.ext_dedup_keys) against a numpy restatement of the definition:
a record is a duplicate iff an earlier record has the same k0 and the same k1 & 0xFFFFFFFFC000FFFF.

The kernels sort one u64 per record, (top 64 - ib hash bits) << ib | index with ib = ceil(log2 n), by the low bits of the
hash field (log2 n + 2, in whole 7-bit digits, tiles of 8192 records) and compare keys only inside runs of equal sorted
bits.  The cases below sit at the steps of those rules and feed keys whose hashes collide on the sorted bits or on the
whole compared hash field, and runs of one key far longer than a tile."""
import numpy as np
import pytest

import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

MASK1 = np.uint64(0xFFFFFFFFC000FFFF)
TILE = 8192


def key_hash(k):
    return util._mix64_np(k[:, 0] ^ util._mix64_np(k[:, 1] & MASK1))


def idx_bits(n):
    return max(1, (n - 1).bit_length())


def sorted_bits(n):
    bits = 2
    while bits < 34 and (1 << (bits - 2)) < n:
        bits += 1
    bits = min(max(bits, 12), 32)
    return min(-(-bits // 7) * 7, 64 - idx_bits(n))


def expected(k):
    a, b = k[:, 0], k[:, 1] & MASK1
    order = np.lexsort((np.arange(k.shape[0]), b, a))         # by key, then input order
    sa, sb = a[order], b[order]
    later = np.zeros(k.shape[0], dtype=bool)
    later[1:] = (sa[1:] == sa[:-1]) & (sb[1:] == sb[:-1])
    flags = np.zeros(k.shape[0], dtype=np.uint8)
    flags[order[later]] = 1
    return flags


def random_keys(rng, n):
    k = rng.integers(0, 1 << 63, size=(n, 3), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 3), dtype=np.uint64)
    return k


def noise_outside_key(rng, k):
    """ord and the k1 bits the key drops are not part of the key: change them all"""
    k = k.copy()
    k[:, 2] = rng.integers(0, 1 << 62, size=k.shape[0], dtype=np.uint64)
    k[:, 1] = (k[:, 1] & MASK1) | (rng.integers(0, 1 << 14, size=k.shape[0], dtype=np.uint64) << np.uint64(16))
    return k


@pytest.fixture(scope="module")
def ctx():
    with m.Context("unc", 0.5, 10, False, 8, device=0) as c:
        yield c


def check(ctx, k):
    flags, dups = ctx.ext_dedup_keys(k)
    want = expected(k)
    bad = np.nonzero(flags != want)[0]
    assert bad.size == 0, f"n={k.shape[0]}: {bad.size} flags differ, first at {bad[:8].tolist()}"
    assert dups == int(want.sum())
    return flags


# the steps of the rules: passes (bits 14 -> 15 at 4097, 21 -> 22 at 2^19 + 1), index bits (powers of two), tiles of 8192
SIZES = [1, 2, 3, 64, 65, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, (1 << 19), (1 << 19) + 1, 3_000_017]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_repeats(ctx, n):
    rng = np.random.default_rng(n)
    pool = random_keys(rng, max(1, (3 * n) // 4))
    k = noise_outside_key(rng, pool[rng.integers(0, pool.shape[0], size=n)])
    flags = check(ctx, k)
    if n == 1:
        assert flags.tolist() == [0]


def test_collisions_on_sorted_bits(ctx):
    """distinct keys that agree on every sorted hash bit: one run of ~1000 keys that must all be compared, none equal"""
    n = 4096
    ib, sb = idx_bits(n), sorted_bits(n)
    rng = np.random.default_rng(5)
    cand = random_keys(rng, 1 << 24)
    s = (key_hash(cand) >> np.uint64(ib)) & np.uint64((1 << sb) - 1)
    same = cand[s == s[0]][:1200]
    assert same.shape[0] > 600
    assert np.unique(same[:, :2], axis=0).shape[0] == same.shape[0]
    k = random_keys(rng, n)
    pos = rng.choice(n, size=same.shape[0], replace=False)
    k[pos] = same
    k[rng.choice(n, size=100, replace=False)] = same[rng.integers(0, same.shape[0], size=100)]   # a few real repeats inside the run
    check(ctx, noise_outside_key(rng, k))
    distinct = random_keys(rng, n)
    distinct[pos] = same
    assert check(ctx, distinct).sum() == 0


def test_collisions_on_the_whole_compared_hash(ctx):
    """distinct keys whose hash fields (every bit the look-back compares) are equal: found by a birthday search"""
    n = (1 << 24) + 3
    ib = idx_bits(n)
    pairs = []
    for seed in range(8):
        cand = random_keys(np.random.default_rng(100 + seed), 1 << 21)
        f = key_hash(cand) >> np.uint64(ib)
        o = np.argsort(f, kind="stable")
        hit = np.nonzero(f[o][1:] == f[o][:-1])[0]
        pairs += [(cand[o[i]], cand[o[i + 1]]) for i in hit if not np.array_equal(cand[o[i], :2], cand[o[i + 1], :2])]
        if len(pairs) >= 2:
            break
    assert pairs, "no collision found"
    rng = np.random.default_rng(9)
    k = random_keys(rng, n)
    where = rng.choice(n, size=2 * len(pairs), replace=False)
    for t, (x, y) in enumerate(pairs):
        hx, hy = key_hash(np.stack([x, y]))
        assert hx >> np.uint64(ib) == hy >> np.uint64(ib)
        k[where[2 * t]], k[where[2 * t + 1]] = x, y
    flags = check(ctx, k)
    assert flags[where].sum() == 0


@pytest.mark.parametrize("reps", [TILE + 5, 300_000])
def test_one_key_repeated(ctx, reps):
    n = reps + 200_000
    rng = np.random.default_rng(reps)
    k = random_keys(rng, n)
    pos = np.sort(rng.choice(n, size=reps, replace=False))
    k[pos] = k[pos[0]]
    k = noise_outside_key(rng, k)
    flags = check(ctx, k)
    assert flags[pos[0]] == 0 and flags[pos[1:]].sum() == reps - 1


def test_lane_bits_make_keys_distinct(ctx):
    n = 50_000
    rng = np.random.default_rng(3)
    k = random_keys(rng, n)
    k[:, 1] &= ~np.uint64(0xFFFF)
    base = k[: n // 4].copy()
    k[n // 4: n // 2] = base
    k[n // 4: n // 2, 1] |= np.uint64(1) + rng.integers(0, 0xFFFF, size=n // 4, dtype=np.uint64)   # lane differs: distinct
    k[n // 2: 3 * n // 4] = base                                                                  # same lane: duplicates
    flags = check(ctx, noise_outside_key(rng, k))
    assert flags[n // 4: n // 2].sum() == 0 and flags[n // 2: 3 * n // 4].sum() == n // 4


def test_ord_and_dropped_bits_do_not_count(ctx):
    n = 20_000
    rng = np.random.default_rng(4)
    k = random_keys(rng, n // 2)
    twin = k.copy()
    twin[:, 2] ^= np.uint64(0xABCDEF)                                        # ord
    twin[:, 1] ^= np.uint64(0x3FFF0000)                                      # every bit kKeyMask1 drops
    flags = check(ctx, np.concatenate([k, twin]))
    assert flags[: n // 2].sum() == 0 and flags[n // 2:].sum() == n // 2
