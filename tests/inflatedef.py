"""TEST INFRASTRUCTURE: a small, plain inflate written from RFC 1951 only (3.2.2 canonical codes, 3.2.4 stored, 3.2.5 length and
distance symbols, 3.2.6 fixed codes, 3.2.7 dynamic codes).  Unlike zlib it shows what a stream is made of: the block type, the
code lengths as sent in the header, and the tokens; and it refuses what the format forbids.  It is the second checker of the
GPU BGZF deflate (tests/test_gpu_deflate_edges.py) beside Python's zlib; tests/test_inflatedef_host.py proves it equal to zlib.
Product code never imports this file, and this file imports nothing from the package.  Speed does not matter."""

import heapq

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CODELEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class InflateError(Exception):
    pass


class Block:
    """One deflate block: btype (0 stored, 1 fixed, 2 dynamic), bfinal, the code lengths as sent (dynamic blocks only:
    ll_lengths has HLIT + 257 entries, d_lengths HDIST + 1, cl_lengths 19 in symbol order with HCLEN + 4 of them sent as
    n_cl_sent, cl_symbols the symbols 0..18 that spell the other lengths), tokens (an int for a literal byte, (length, distance) for a match), nbits (size of the block in the stream)."""

    def __init__(self):
        self.btype = self.bfinal = None
        self.ll_lengths = self.d_lengths = self.cl_lengths = None
        self.n_cl_sent = None
        self.cl_symbols = None
        self.stored_len = None
        self.tokens = []
        self.nbits = 0


class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def peek(self, n):
        """the next n <= 24 bits, the first one in bit 0 (zeros behind the end of the data)"""
        q = self.p >> 3
        return (int.from_bytes(self.d[q:q + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def take(self, n):
        if self.p + n > 8 * len(self.d):
            raise InflateError("the stream ends inside a block")
        v = self.peek(n)
        self.p += n
        return v


class _Code:
    """canonical Huffman code of 3.2.2 from code lengths; refuses over-subscribed and incomplete sets of lengths"""

    def __init__(self, lengths, what, allow_single=False):
        used = [l for l in lengths if l]
        if not used:
            raise InflateError(f"{what} code: no symbol has a code")
        maxl = max(used)
        kraft = sum(1 << (maxl - l) for l in used)
        if kraft > 1 << maxl:
            raise InflateError(f"{what} code: over-subscribed")
        if kraft < 1 << maxl and not (allow_single and len(used) == 1 and used[0] == 1):
            raise InflateError(f"{what} code: incomplete")
        bl_count = [0] * (maxl + 2)
        for l in used:
            bl_count[l] += 1
        next_code, code = [0] * (maxl + 2), 0
        for bits in range(1, maxl + 1):
            code = (code + bl_count[bits - 1]) << 1
            next_code[bits] = code
        self.map = {}                                         # (length, the code as it lies in the stream: first bit in bit 0) -> symbol
        for s, l in enumerate(lengths):
            if l:
                self.map[(l, int(format(next_code[l], "0%db" % l)[::-1], 2))] = s     # codes are packed starting from their most significant bit
                next_code[l] += 1
        self.maxl = maxl
        self.what = what

    def read(self, bits):
        w = bits.peek(self.maxl)
        for l in range(1, self.maxl + 1):
            s = self.map.get((l, w & ((1 << l) - 1)))
            if s is not None:
                bits.take(l)
                return s
        raise InflateError(f"{self.what} code: a bit pattern that is no code (the unused code of a single-code set)")


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


def inflate(data, max_out=1 << 30):
    """(blocks, inflated bytes) of one raw deflate stream that fills `data` up to the padding of its last byte"""
    bits = _Bits(data)
    out = bytearray()
    blocks = []
    while True:
        b = Block()
        start = bits.p
        b.bfinal = bits.take(1)
        b.btype = bits.take(2)
        if b.btype == 0:
            while bits.p & 7:
                if bits.take(1):
                    raise InflateError("stored block: the bits up to the byte boundary are not zero")
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xFFFF:
                raise InflateError("stored block: NLEN is not the complement of LEN")
            q = bits.p >> 3
            if q + n > len(data):
                raise InflateError("the stream ends inside a stored block")
            out += data[q:q + n]
            b.tokens = list(data[q:q + n])
            b.stored_len = n
            bits.p += 8 * n
        elif b.btype in (1, 2):
            if b.btype == 1:
                ll, dc = _Code(_FIXED_LL, "fixed literal/length"), _Code(_FIXED_D, "fixed distance")
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if hlit > 286:
                    raise InflateError("dynamic block: more than 286 literal/length codes")
                if hdist > 30:
                    raise InflateError("dynamic block: more than 30 distance codes")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CODELEN_ORDER[i]] = bits.take(3)
                b.cl_lengths, b.n_cl_sent = cl, hclen
                cc = _Code(cl, "code-length")
                lens = []
                b.cl_symbols = []
                while len(lens) < hlit + hdist:
                    s = cc.read(bits)
                    b.cl_symbols.append(s)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise InflateError("dynamic block: repeat of a previous length at the first length")
                        lens += [lens[-1]] * (3 + bits.take(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.take(3))
                    else:
                        lens += [0] * (11 + bits.take(7))
                if len(lens) != hlit + hdist:
                    raise InflateError("dynamic block: a repeat runs past the last code length")
                b.ll_lengths, b.d_lengths = lens[:hlit], lens[hlit:]
                if not b.ll_lengths[256]:
                    raise InflateError("dynamic block: no code for end of block")
                ll = _Code(b.ll_lengths, "literal/length")
                dc = _Code(b.d_lengths, "distance", allow_single=True) if any(b.d_lengths) else None      # (literals only: no distance code at all)
            while True:
                s = ll.read(bits)
                if s < 256:
                    out.append(s)
                    b.tokens.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise InflateError(f"length symbol {s}")
                    length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    if dc is None:
                        raise InflateError("a match in a block without distance codes")
                    ds = dc.read(bits)
                    if ds > 29:
                        raise InflateError(f"distance symbol {ds}")
                    dist = DIST_BASE[ds] + bits.take(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise InflateError(f"distance {dist} reaches before the start of the data ({len(out)} bytes so far)")
                    for _ in range(length):
                        out.append(out[-dist])
                    b.tokens.append((length, dist))
                if len(out) > max_out:
                    raise InflateError("output larger than allowed")
        else:
            raise InflateError("block type 3")
        b.nbits = bits.p - start
        blocks.append(b)
        if b.bfinal:
            break
    while bits.p & 7:
        if bits.take(1):
            raise InflateError("trailing bits that are not padding")
    if bits.p >> 3 != len(data):
        raise InflateError(f"{len(data) - (bits.p >> 3)} trailing bytes after the final block")
    return blocks, bytes(out)


def replay(tokens):
    """the bytes a token list stands for"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            if not 3 <= length <= 258 or not 1 <= dist <= min(32768, len(out)):
                raise InflateError(f"token {t} at {len(out)}")
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def histograms(block):
    """(literal/length counts [286] with end of block, distance counts [30]) of a block's tokens"""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in block.tokens:
        if isinstance(t, tuple):
            ll[257 + max(i for i, b in enumerate(LENGTH_BASE) if b <= t[0])] += 1
            d[max(i for i, b in enumerate(DIST_BASE) if b <= t[1])] += 1
        else:
            ll[t] += 1
    return ll, d


# the plain reference of the code construction (tests/test_deflate_codes_host.py, tests/test_gpu_deflate_edges.py)
def heap_huffman(counts):
    """{symbol: length} of a Huffman code for the used symbols: a heap of (weight, depth, ...); among equal weights the
    shallower subtree is merged first, which gives the optimal code of least depth.  One symbol: length 1."""
    used = [(c, s) for s, c in enumerate(counts) if c]
    if len(used) == 1:
        return {used[0][1]: 1}
    heap = [(c, 0, s, (s,)) for c, s in used]
    heapq.heapify(heap)
    depth = {s: 0 for _, s in used}
    tick = len(counts)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        tick += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick, a[3] + b[3]))
    return depth
