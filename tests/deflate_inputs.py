"""TEST INFRASTRUCTURE: the byte strings of the deflate edge tests (tests/test_gpu_deflate_edges.py feeds them to the GPU deflate
inside B:C arrays; tests/test_inflatedef_host.py feeds them to zlib and to tests/inflatedef.py), and the SAM text that puts
such a string at a chosen offset of the BAM's uncompressed stream.  Seeded, plain Python, nothing from the package."""
import random

BGZF_RAW = 0xff00
DZ_WAVES = 8                       # follows MKT_DZ_WAVES in microcket_amd/csrc/mkt_deflate.hip
DZ_Q = BGZF_RAW // DZ_WAVES        # bytes of a block that one wave parses: matches never leave a share
REC_HEAD = 46                      # block_size 4 + fixed fields 32 + "r\0" 2 + tag XB:B:C 4 + count 4
FILL = bytes([1, 2, 3, 7])         # filler alphabet: compressible, and never a run byte of the tests


def filler(rng, k):
    return bytes(rng.choice(FILL) for _ in range(k))


def header_only_sam(total):
    """SAM header whose BAM is `total` uncompressed bytes long: magic 4 + l_text 4 + text + n_ref 4 (no reference, no record)"""
    assert total == 12 or total >= 17
    if total == 12:
        return b""
    rng = random.Random(total)
    return b"@CO\t" + bytes(rng.choice(b"ACGTNacgtn =:") for _ in range(total - 17)) + b"\n"


def header_only_raw(total):
    text = header_only_sam(total)
    return b"BAM\x01" + len(text).to_bytes(4, "little") + text + (0).to_bytes(4, "little")


def payload_sam(payload, at=BGZF_RAW):
    """SAM text of one unmapped record that carries `payload` in a B:C array, behind a header padded so that the payload's
    first byte is byte `at` of the uncompressed stream (the default: the first byte of the second BGZF block)"""
    assert at >= 12 + 5 + REC_HEAD and payload
    text = b"@CO\t" + b"." * (at - REC_HEAD - 12 - 5) + b"\n"
    return text + b"r\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tXB:B:C," + b",".join(b"%d" % x for x in payload) + b"\n"


def random_bytes(seed, k):
    return random.Random(seed).randbytes(k)


def periodic(seed, period, k):
    """k bytes of period `period`; one period holds no 4-gram twice where 256 values allow it (period <= 256: distinct bytes)"""
    rng = random.Random(seed)
    if period == 2:
        unit = b"AB"
    elif period <= 256:
        unit = bytes(rng.sample(range(256), period))
    else:
        unit = rng.randbytes(period)
    return (unit * (k // period + 1))[:k]


def no_repeated_4gram(seed, k, alphabet):
    """k bytes over `alphabet` by a seeded walk that never lets a 4-gram occur twice inside one share of DZ_Q bytes (shares
    counted from the string's first byte: put it at the start of a block)"""
    rng = random.Random(seed)
    out = bytearray()
    seen = set()
    while len(out) < k:
        if len(out) % DZ_Q == 0:
            seen = set()
        for _ in range(1000):
            c = rng.choice(alphabet)
            g = bytes(out[-3:]) + bytes([c]) if len(out) % DZ_Q >= 3 else None
            if g is None or g not in seen:
                break
        else:
            raise AssertionError("walk stuck")
        if g is not None:
            seen.add(g)
        out.append(c)
    return bytes(out)


def has_repeated_4gram(block):
    """does any share of the block hold a 4-gram twice"""
    for q in range(0, len(block), DZ_Q):
        sh = block[q:q + DZ_Q]
        grams = [sh[i:i + 4] for i in range(len(sh) - 3)]
        if len(set(grams)) != len(grams):
            return True
    return False


def ends_in_run(seed, n, run, byte, at):
    """payload of a single-block file of n uncompressed bytes (payload at `at`) that ends in exactly `run` bytes of `byte`"""
    rng = random.Random(seed)
    k = n - at
    assert k >= run + 1
    return filler(rng, k - run) + bytes([byte]) * run


RUN_BYTES = bytes(range(0x50, 0x58))   # one run byte per share of a block (none of them in FILL)


def share_end_runs(seed, nblocks):
    """nblocks whole blocks of filler; before every share end a run starts 255..262 bytes early and goes on 40 bytes into the next
    share.  The run opens with a literal and its match starts one byte in, so 254..261 bytes are left up to the share end while
    the run itself measures 258: the match is cut to 254..257, ends exactly at the share end (258), or leaves 1..3 bytes that no
    longer hash.  Every share of a block has a run byte of its own (RUN_BYTES): the tail of the previous share's run, which
    opens this share, must not put this run's four bytes into the share's hash table, or the run would open with a far match."""
    rng = random.Random(seed)
    out = bytearray(filler(rng, nblocks * BGZF_RAW + 40))
    k = 0
    for q1 in range(DZ_Q, nblocks * BGZF_RAW + 1, DZ_Q):
        start = q1 - 1 - (254 + (k * 3 + k // 8) % 8)
        byte = RUN_BYTES[k % DZ_WAVES]
        k += 1
        out[start:q1 + 40] = bytes([byte]) * (q1 + 40 - start)
    return bytes(out)


def fibonacci_block(seed, nsym=22, run_byte=0xEE):
    """one block: nsym byte values with exact Fibonacci counts (1, 1, 2, 3, 5, ...: 46 367 bytes for 22 values), shuffled and dealt
    out share by share, every share topped up with one run of run_byte"""
    rng = random.Random(seed)
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    lits = bytearray()
    for i, c in enumerate(f):
        lits += bytes([0x20 + 3 * i]) * c
    assert len(lits) <= BGZF_RAW - 8 * 8
    lits = list(lits)
    rng.shuffle(lits)
    per = (len(lits) + DZ_WAVES - 1) // DZ_WAVES
    out = bytearray()
    for w in range(DZ_WAVES):
        part = bytes(lits[w * per:(w + 1) * per])
        out += part + bytes([run_byte]) * (DZ_Q - len(part))
    assert len(out) == BGZF_RAW
    return bytes(out)


def host_strings():
    """(name, bytes) of every kind of string above, at sizes a plain-Python inflate handles quickly"""
    rng = random.Random(5)
    return [
        ("one-byte", b"\x00"),
        ("header-63", header_only_raw(63)),
        ("header-share", header_only_raw(DZ_Q + 3)),
        ("random", random_bytes(1, 3000)),
        ("zeros", bytes(20000)),
        ("run-0x41", b"\x41" * 20000),
        ("period-2", periodic(2, 2, 5000)),
        ("period-3", periodic(2, 3, 5000)),
        ("period-70", periodic(2, 70, 5000)),
        ("period-258", periodic(2, 258, 5000)),
        ("period-259", periodic(2, 259, 5000)),
        ("no-4gram-24", no_repeated_4gram(3, 9000, bytes(range(40, 64)))),
        ("ends-in-zeros", ends_in_run(4, 2001, 257, 0, 63)),
        ("ends-in-0x41", ends_in_run(4, 2003, 300, 0x41, 63)),
        ("share-end-runs", share_end_runs(6, 1)[:20000]),
        ("fibonacci", fibonacci_block(7)[:DZ_Q * 2]),
        ("filler", filler(rng, 4000)),
    ]
