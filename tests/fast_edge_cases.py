"""Inputs that sit on the byte limits of the lean tile kernel (k_fast in mkt_kernels.hip, phase functions in mkt_fast.h).

Deterministic builders, no randomness, no files.  cases() gives (name, text, modes, expect): `expect` is the number of tiles
of the forced 48 KiB geometry (tile 49152, halos 3072 / 4096, 168 lines: MKT_TILES_FAST, emulation config 10) that the LEAN
path must take, an integer or "all".  A case that is meant to be refused is refused in exactly one tile, and the line that
does it sits alone among plain two-line groups in the middle of that tile; a case that is meant to be accepted loses no
tile at all.  Both are functions of the text alone (one block), so the CPU test (test_fast_edges_host.py) pins them on the
emulation and the GPU test (test_gpu_fast_edges.py) asks the kernel for the same count.

Lines are bwa shaped (150 bytes of SEQ and of QUAL); a plain line is 384 bytes, a plain group 768, so that 64 plain groups are
one tile and tile starts fall on group starts until a case moves them.  Every text ends in a sacrificial last group (quirk
Q1: the reference never classifies the input's last group).

The filtered lines of the group cases carry FLAG 321 (secondary) and MAPQ 0: the suite also runs with a MAPQ threshold of 0,
where MAPQ alone would let them survive and the number of lean tiles would depend on the parameters.
"""

TILE, HB, HF, LCAP, GCAP = 49152, 3072, 4096, 168, 96
PLAIN = 384
BOTH = ("unc", "flash")
SEQ = (b"ACGT" * 38)[:150]
QUAL = b"F" * 150


def line(q, flag=b"65", rname=b"chr1", pos=b"1000", mapq=b"60", cigar=b"150M", length=None, tag=b"NM:i:0", seqlen=150, seps=b"\t\t\t\t\t"):
    """one SAM line; `length`: total bytes with the newline, made up by the tag column (16 bytes more where the fields need it); seps: the five separators of the six leading fields"""
    f = (q, flag, rname, pos, mapq, cigar)
    head = b"".join(f[k] + seps[k:k + 1] for k in range(5)) + cigar
    body = b"\t=\t1\t0\t" + SEQ[:seqlen] + b"\t" + QUAL[:seqlen] + b"\t"
    if length is not None:
        k = length - len(head) - len(body) - 1
        while k < 1:                   # long leading fields: the next length of the same residue mod 16
            k += 16
        tag = (b"XT:Z:" + b"x" * k)[:k]
    return head + body + tag + b"\n"


def plain_group(k, la=PLAIN, lb=PLAIN, seqlen=150):
    """group k of the filler: a cis pair 20 kb apart (every fifth one trans), both mates kept"""
    q = b"pl%07d" % k
    return [line(q, b"65", b"chr1", b"%d" % (1000000 + 1000 * k), length=la, seqlen=seqlen),
            line(q, b"145", b"chr2" if k % 5 == 0 else b"chr1", b"%d" % (1020000 + 1001 * k), length=lb, seqlen=seqlen)]


def filtered(q, length=PLAIN):
    return line(q, b"321", b"chr7", b"777", b"0", length=length)


def pair(q, mate=None, **kw):
    """a two-line group: the line under test (first mate, fields from kw) and a plain second mate of the same name"""
    m = dict(flag=b"145", rname=b"chr1", pos=b"1020304", length=PLAIN)
    m.update(mate or {})
    kw.setdefault("length", PLAIN)
    return [line(q, **kw), line(q, **m)]


TAIL = [line(b"zz", b"65", b"chr1", b"1", cigar=b"1M", length=PLAIN), line(b"zz", b"129", b"chr1", b"1", cigar=b"1M", length=PLAIN)]


class Text:
    def __init__(self):
        self.lines, self.n, self.k = [], 0, 0

    def add(self, lines):
        for ln in ([lines] if isinstance(lines, bytes) else lines):
            self.lines.append(ln)
            self.n += len(ln)
        return self

    def plain(self, groups=1, **kw):
        for _ in range(groups):
            self.add(plain_group(self.k, **kw))
            self.k += 1
        return self

    def plain_until(self, target):
        """whole plain groups, the last one stretched, so that the next line starts at byte `target` exactly"""
        assert target - self.n >= 700, (target, self.n)
        while target - self.n >= 2 * PLAIN + 700:
            self.plain()
        rem = target - self.n
        return self.plain(la=rem // 2, lb=rem - rem // 2)

    def end(self, tail=TAIL):
        return b"".join(self.lines) + b"".join(tail)


def ntiles(text):
    return (len(text) + TILE - 1) // TILE


def window_lines(text):
    """entries of the lean line table per tile: the 16-byte vectors of the window that hold a newline (+ the block's first line)"""
    out = []
    for t in range(ntiles(text)):
        t0, t1 = t * TILE, min((t + 1) * TILE, len(text))
        w0, w1 = max(t0 - HB, 0), min(t1 + HF, len(text))
        out.append(sum(1 for v in range(w0, w1, 16) if b"\n" in text[v:min(v + 16, w1)]) + (1 if w0 == 0 else 0))
    return out


def iso(test_lines, refused, pre=32, shift=0, modes=BOTH):
    """the lines under test behind `pre` plain groups (the last line of those `shift` bytes longer: the residue of the test line's
    start mod 16), then plain groups past the end of the tile: (text, modes, expect)"""
    t = Text()
    if pre:
        t.plain(pre - 1).plain(lb=PLAIN + shift)
    t.add(test_lines)
    while t.n < TILE + 6 * 2 * PLAIN:
        t.plain()
    text = t.end()
    assert pre == 0 or t.n > TILE > pre * 2 * PLAIN + sum(len(x) for x in test_lines) + HF      # alone in tile 0, outside tile 1's window
    return text, modes, (ntiles(text) - 1 if refused else "all")


def qn(n, k=0):
    return (b"%09d" % k).rjust(n, b"q")[-n:] if n >= 9 else (b"abcdefgh"[:n - 1] + b"%d" % (k % 10))


def cigar_of(n):
    """a CIGAR token of n bytes (n >= 12): cycles of 10M1I10M1D, then 1I operations and a last M; no count above two digits"""
    c = b""
    while len(c) + 10 <= n - 2:
        c += b"10M1I10M1D"
    r = n - len(c)
    c += b"1I" * (r // 2 - 1) + b"9M" if r % 2 == 0 else b"1I" * ((r - 3) // 2) + b"10M"
    assert len(c) == n
    return c


def _parser(C):
    # QNAME length: p[3] >= 12 needs five bytes when the fields behind it are as short as they get; 62 is the last a head takes
    for n, refused in ((4, True), (5, False), (62, False), (63, True), (100, True), (101, True)):
        C["qname_%d" % n] = iso(pair(qn(n), rname=b"1", pos=b"7", mate=dict(rname=b"1", pos=b"20007")), refused)
    # the sixth separator 64 / 65 bytes behind the QNAME's: by RNAME length (13 + R + C with a two-digit FLAG, POS 1000, MAPQ 60) ...
    C["sep6_rname_64"] = iso(pair(qn(9), rname=b"chrUn_" + b"K" * 41), False)
    C["sep6_rname_65"] = iso(pair(qn(9), rname=b"chrUn_" + b"K" * 42), True)
    # ... and by CIGAR length (RNAME of 20 bytes)
    C["sep6_cigar_64"] = iso(pair(qn(9), rname=b"chrUn_KI270742v1_abc", cigar=cigar_of(31)), False)
    C["sep6_cigar_65"] = iso(pair(qn(9), rname=b"chrUn_KI270742v1_abc", cigar=cigar_of(32)), True)
    # six fields ending at head byte 127 - soff and one further (QNAME of 62 bytes: the separator is byte 75 + R + 4 of the line).
    # soff = 1: byte 126 is also the 64th behind the QNAME; soff = 0 (the block's first line) cannot reach byte 127 for that reason
    for soff, r in ((16, 32), (8, 40), (1, 47), (0, 47)):
        for d in (0, 1):
            C["head_soff%d_%s" % (soff, "last" if d == 0 else "past")] = iso(pair(qn(62), rname=b"c" * (r + d)), d == 1, pre=32 if soff else 0, shift=soff % 16)
    # FLAG: 1..4 characters (lean_uint4), 5..10 with leading zeros (lean_uint12); 11 characters: the generic parser decides
    g = []
    for k, f in enumerate((b"0", b"65", b"081", b"1089", b"00065", b"000097", b"0000065", b"00000081", b"000000065", b"0000000065")):
        g += pair(b"fl%07d" % k, flag=f, pos=b"%d" % (5000 + k))
    C["flag_forms"] = iso(g, False)
    g = []
    for k, p in enumerate((b"7", b"42", b"512", b"4096", b"65536", b"100000", b"1234567", b"12345678", b"123456789", b"2147483000", b"0000001000")):
        g += pair(b"po%07d" % k, pos=p)
    C["pos_forms"] = iso(g, False)
    C["pos_above_int"] = iso(pair(b"po4294967", pos=b"4294967295"), False)          # (the reference reads POS into an int: REF_UNPINNED)
    g = []
    for k, q in enumerate((b"9", b"10", b"060", b"255", b"00060", b"0000000060")):
        g += pair(b"mq%07d" % k, mapq=q, pos=b"%d" % (7000 + k))
    C["mapq_forms"] = iso(g, False)
    C["flag_11_chars"] = iso(pair(b"fl11chars", flag=b"00000000065"), True)
    C["pos_11_chars"] = iso(pair(b"po11chars", pos=b"00001000000"), True)
    C["mapq_11_chars"] = iso(pair(b"mq11chars", mapq=b"00000000060"), True)
    C["mapq_11_chars_low"] = iso(pair(b"mq11chlow", mapq=b"00000000009"), True)
    # CIGAR: tokens of up to 32 bytes, counts of up to nine digits; odd shapes both parsers treat like the reference
    g = []
    for k, c in enumerate((cigar_of(32), b"50M1234N100M", b"50M12345N100M", b"50M123456789N100M", b"M150M", b"150M7", b"60S90M", b"9999S1M")):
        g += pair(b"cg%07d" % k, cigar=c, pos=b"%d" % (9000 + 37 * k))
        g += pair(b"ch%07d" % k, mate=dict(cigar=c), pos=b"%d" % (9500 + 41 * k))
    C["cigar_forms"] = iso(g, False)
    # (no segment at all: the reference then reads what the record before left behind, REF_UNPINNED)
    C["cigar_star"] = iso(pair(b"cgstar001", cigar=b"*") + pair(b"cgstar002", mate=dict(cigar=b"*")), False)
    C["cigar_no_operation"] = iso(pair(b"cgnoop001", cigar=b"150") + pair(b"cgnoop002", mate=dict(cigar=b"150")), False)
    C["cigar_33_bytes"] = iso(pair(b"cg33bytes", cigar=cigar_of(33)), True)
    C["cigar_count_10_digits"] = iso(pair(b"cg10digit", cigar=b"50M1234567890N100M"), True)
    # separators: any byte <= 0x20 that is no tab inside the six fields hands the tile over (for the reference 0x01 and 0x1f are name bytes)
    # (white space there would split the name and leave a POS that is no number: out of contract; it stands for a tab below)
    for b in (0x01, 0x1f):
        C["byte_%02x_in_rname" % b] = iso(pair(b"sp%07d" % b, rname=b"ch" + bytes([b]) + b"r1"), True)
    for b in (0x20, 0x0d, 0x0b):
        C["byte_%02x_for_a_tab" % b] = iso(pair(b"st%07d" % b, seps=b"\t" + bytes([b]) + b"\t\t\t"), True)
    C["double_tab"] = iso(pair(b"dbltab000", seps=b"\t\t\t\t\t", rname=b"\tchr1"), True)
    # bytes above 0x20 are name bytes: 0x8a is a newline with the top bit set (the scan's and sep_flags' bit tricks)
    g = []
    for k, b in enumerate((0x21, 0x7f, 0x80, 0x8a, 0xff)):
        g += pair(b"nm" + bytes([b]) * 3 + b"%04d" % k, pos=b"%d" % (3000 + k))
        g += pair(bytes([b]) + b"x%06d" % k + bytes([b]), pos=b"%d" % (3100 + k))
    C["qname_bytes"] = iso(g, False)
    g = []
    for k, b in enumerate((0x0b, 0x8a, 0x09, 0x20)):
        g += pair(b"tg%07d" % k, tag=b"XT:Z:a" + bytes([b]) * 2 + b"b" + bytes([b]), length=None, pos=b"%d" % (4000 + k))
    C["tag_bytes"] = iso(g, False)
    # a line of six fields and nothing behind them is a record; lines of fewer fields (five, a header in mid-text) are none.
    # (unc mode only: in flash mode the reference makes a fragment of such a line from the fields of the line before, out of contract)
    C["six_fields"] = iso(pair(b"nr0000001") + [b"sixfields\t65\tchr1\t1000\t60\t150M\n"] + pair(b"nr0000002"), False)
    g = pair(b"nr0000001") + [b"fivefield\t65\tchr1\t1000\t60\n"] + pair(b"nr0000002") + [b"@SQ\tSN:chr1\tLN:248956422\n"] + pair(b"nr0000003")
    C["no_records"] = iso(g, False, modes=("unc",))


def _window(C):
    # line starts at every residue mod 16 (the newline in front of them at every byte of its vector, 15 included)
    t = Text().plain(8)
    for r in range(16):
        t.plain(la=PLAIN + r, lb=PLAIN + 2 * r + 1)
    while t.n < TILE + 8 * PLAIN:
        t.plain()
    C["line_start_residues"] = (t.end(), BOTH, "all")
    # a newline at w1 - 2, w1 - 1 (the line behind it starts at w1: a table entry that is no line of this window) and w1
    for d in (-2, -1, 0):
        t = Text().plain_until(TILE + HF + d + 1).plain(8)
        C["newline_at_w1%+d" % d] = (t.end(), BOTH, "all")
    # a line that starts at t1 - 1 (the tile's last own line), t1 (the next tile's first), t1 + 1
    for d in (-1, 0, 1):
        t = Text().plain_until(TILE + d).plain(8)
        C["line_start_at_t1%+d" % d] = (t.end(), BOTH, "all")
    # text lengths of every residue mod 16, the last line with and without its newline.  The end lies inside tile 0's forward
    # halo: tile 0 runs the scan's tail mask, the staging's block-end path and `reach`; tile 1 holds the last group, whose last
    # member lacks its newline in the second form (AB_LAST_LINE)
    for r in range(16):
        t = Text().plain_until(TILE + 2 * PLAIN)
        tail = [TAIL[0], line(b"zz", b"129", b"chr1", b"1", cigar=b"1M", length=PLAIN + r)]
        text = t.end(tail)
        assert len(text) % 16 == r and ntiles(text) == 2
        C["text_length_%02d" % r] = (text, BOTH, "all")
        C["text_length_%02d_no_newline" % ((r - 1) % 16)] = (text[:-1], BOTH, 1)
    # windows of exactly 168 and 169 lines: the middle tile of three; lines of 352 bytes (160 per window), some of 320 between tile 0's
    # window and tile 2's (SEQ of 130 bytes here)
    for want in (LCAP, LCAP + 1):
        for short in range(0, 132, 2):
            t, used = Text(), 0
            while t.n < 3 * TILE - 4000:
                s = t.n >= TILE + HF and used < short
                used += 2 if s else 0
                t.plain(la=320 if s else 352, lb=320 if s else 352, seqlen=130)
            text = t.end()
            nl = window_lines(text)
            if nl[1] >= want:
                break
        assert nl[1] == want and ntiles(text) == 3 and nl[0] < LCAP and nl[2] < LCAP, nl
        C["window_of_%d_lines" % want] = (text, BOTH, "all" if want == LCAP else 2)
    # a line of fewer than 16 bytes: both of its newlines in one vector (the table misses a line) or in two (unc mode: see no_records)
    short = b"xy\tshort\tline1\n"
    assert len(short) == 15
    C["short_line_two_vectors"] = iso(pair(b"sh0000001") + [short] + pair(b"sh0000002"), False, shift=2, modes=("unc",))
    C["short_line_one_vector"] = iso(pair(b"sh0000001") + [short] + pair(b"sh0000002"), True, shift=1, modes=("unc",))
    # several blocks (run with small block sizes by the tests): three tiles of plain groups of many lengths
    t = Text()
    while t.n < 2 * TILE + 9000:
        t.plain(la=PLAIN + (7 * t.k) % 23, lb=PLAIN - (5 * t.k) % 19)
    C["three_tiles"] = (t.end(), BOTH, "all")


def group_of(q, n, k0=0):
    return [line(q, b"65" if k % 2 == 0 else b"145", b"chr1" if k % 3 else b"chr3", b"%d" % (40000 + 977 * (k0 + k)), length=PLAIN) for k in range(n)]


def _groups(C):
    # a group of 63 lines closes inside the 64-line word of its first line; 64 and 65 do not
    for n in (63, 64, 65):
        C["group_of_%d" % n] = iso(group_of(b"biggroup0", n), n > 63, pre=16)
    # ... but the block's last group may have 64: nothing can follow it
    for n in (64, 65):
        text = Text().plain(10).end(group_of(b"zz", n))
        C["last_group_of_%d" % n] = (text, BOTH, "all" if n == 64 else 0)
    # opens in tile 0's last own line (line 127); lines 127 .. 137 are complete inside the window, line 138 starts in it
    for n in (11, 12):
        t = Text().plain(63).add(line(b"single001", length=PLAIN)).add(group_of(b"halogroup", n)).plain(10)
        C["group_to_halo_line_%d" % n] = (t.end(), BOTH, "all" if n == 11 else 1)
    # the previous surviving line 62, 63 and 64 lines back, filtered strangers in between.  The line before the run is a group of its
    # own (one line): a longer one would not close inside its 64-line word.  With the same name behind the run the lines are ONE
    # group of d + 1 lines, which closes inside its word up to d = 62
    for d in (62, 63, 64):
        run = [filtered(b"fs%07d" % k) for k in range(d - 1)]
        C["prev_survivor_%d_back_new_name" % d] = iso([line(b"before000", length=PLAIN)] + run + pair(b"after0000"), d > 63, pre=12)
        C["prev_survivor_%d_back_same_name" % d] = iso([line(b"around000", length=PLAIN)] + run + [line(b"around000", b"145", pos=b"31000", length=PLAIN)], d > 62, pre=12)
    # the block's first surviving line is a start by itself while it is one of the first 64 lines
    for n in (63, 64):
        t = Text().add([filtered(b"ff%07d" % k) for k in range(n)])
        while t.n < TILE + 8 * PLAIN:
            t.plain()
        text = t.end()
        C["first_survivor_is_line_%d" % n] = (text, BOTH, "all" if n == 63 else ntiles(text) - 1)
    # strangers between two surviving lines (d > 1) whose names differ in their last byte only: the direct comparison.
    # (61 bytes in common: a lean QNAME has at most 62)
    p = b"P" * 61
    g = pair(p + b"a") + [filtered(p + b"b") for _ in range(3)] + pair(p + b"c") + [filtered(p + b"d") for _ in range(2)]
    g += [line(p + b"c", b"2113", b"chr3", b"900", cigar=b"80H70M", length=PLAIN)]
    C["strangers_share_61_bytes"] = iso(g, False)
    # three-line groups (1 + 2 in unc mode) across line indices 63 | 64 and 127 | 128 of tile 0's window: m_emit's two-word OR
    def three(k):
        q = b"tr%07d" % k
        return [line(q, b"65", b"chr2", b"%d" % (5000 + k), length=PLAIN), line(q, b"129", b"chr2", b"%d" % (5300 + k), length=PLAIN),
                line(q, b"2177", b"chr3", b"%d" % (900 + k), cigar=b"80H70M", length=PLAIN)]
    t = Text().plain(31).add(three(0)).add(three(1)).plain(29).add(three(2)).plain(12)         # lines 62-64, 65-67, 126-128
    C["emit_across_words_a"] = (t.end(), BOTH, "all")
    t = Text().add(three(0)).plain(30).add(three(1)).add(three(2)).plain(29).add(three(3)).plain(12)     # lines 0-2, 63-65, 66-68, 127-129
    C["emit_across_words_b"] = (t.end(), BOTH, "all")
    # flash mode: single-line fragments report a pair each; tile 0 holds 96 / 97 of them and filtered lines.  (A text of nothing
    # but such lines has ~123 reporting groups per tile: every tile goes to the generic kernel with reason AB_GCAP.)
    for n in (GCAP, GCAP + 1):
        t = Text().add([filtered(b"fg%07d" % k) for k in range(128 - n)])
        t.add([line(b"sg%07d" % k, b"0", b"chr1", b"%d" % (60000 + 13 * k), length=PLAIN) for k in range(n)]).plain(10)
        C["flash_%d_reporting_groups" % n] = (t.end(), ("flash",), "all" if n == GCAP else 1)


def _outputs(C):
    # .pairs lines of every length mod 4: names of 5 .. 20 bytes, positions of 1 .. 10 digits
    g = []
    for k in range(32):
        g += pair(qn(5 + k % 16, k), pos=b"%d" % (10 ** (k % 10) + k % 7), mate=dict(pos=b"%d" % (2 * 10 ** ((k * 3) % 10) + k)))
    C["pairs_line_lengths"] = iso(g, False, pre=20)
    # .sam: reporting and silent groups interleaved (gaps in the source of the copy), lines of every length mod 16
    g = []
    for k in range(16):
        g += pair(b"em%07d" % k, length=PLAIN + (5 * k) % 16, mate=dict(length=PLAIN - (3 * k) % 16))
        g += [filtered(b"no%07d" % k, PLAIN + k % 5)] * (k % 3) + [line(b"un%07d" % k, b"65", length=PLAIN + k % 11)]
    C["sam_gaps"] = iso(g, False, pre=12)
    # a reporting group whose last line ends the block (read through the block's own outputs: quirk Q1 drops it from the run's).
    # Few reporting lines: a resident block's .sam buffer is cut into 16 regions of (1.25 n + 64 KiB) / 16 bytes, and this one
    # tile writes into one of them
    for r in (0, 5, 11):
        t = Text().add([filtered(b"fb%07d" % k) for k in range(30)]).plain(3)
        C["block_end_reports_%02d" % r] = (t.end(plain_group(99, lb=PLAIN + r)), BOTH, "all")
    C["chr_cache"] = (chr_cache_text(), BOTH, "all")


CC_MULT = 0x9E3779B1


def cc_idx(name):
    """fast_chr_slot's cache index of a name of up to six bytes"""
    return ((int.from_bytes(name, "little") * CC_MULT) >> 30) & 63


def chr_cache_names():
    """70 names of 1..6 bytes, most of them from the two-way sets (idx, idx ^ 1) with the most candidates, and three long ones"""
    cand = [b"%d" % k for k in range(1, 100)] + [b"c%d" % k for k in range(1, 100)] + [b"chr%d" % k for k in range(1, 100)] + [b"chrX", b"chrY", b"chrM", b"MT", b"X", b"chrEBV"]
    sets = {}
    for nm in cand:
        sets.setdefault(cc_idx(nm) >> 1, []).append(nm)
    order = sorted(sets, key=lambda s: (-len(sets[s]), s))
    names = []
    for s in order:
        names += sets[s]
        if len(names) >= 70:
            break
    return names[:70] + [b"chrUn_KI270742v1", b"chr1_KI270706v1_random", b"scaffold"]


def chr_cache_text():
    names = chr_cache_names()
    t = Text()
    for k in range(2 * len(names)):
        a, b = names[k % len(names)], names[(7 * k + 3) % len(names)]
        t.add(pair(b"cc%07d" % k, rname=a, pos=b"%d" % (1000 + k), mate=dict(rname=b, pos=b"%d" % (91000 + 3 * k))))
    return t.end()


MULTIBLOCK = ("three_tiles", "line_start_residues", "sam_gaps")
BLOCK_SIZES = (4096, TILE + 3 * PLAIN)
BLOCK_END = ("block_end_reports_00", "block_end_reports_05", "block_end_reports_11")
# cases the reference itself is not compared on: its behaviour there is undefined (out of contract), and what the oracle
# defines is what the emulation and the kernel have to give
REF_UNPINNED = ("pos_above_int", "cigar_star", "cigar_no_operation")
_cases = None


def cases():
    global _cases
    if _cases is None:
        C = {}
        _parser(C)
        _window(C)
        _groups(C)
        _outputs(C)
        _cases = [(name,) + C[name] for name in C]
        for name, text, modes, expect in _cases:
            assert len(text) < 300000 and (expect == "all" or 0 <= expect < ntiles(text)), name
    return _cases


def case(name):
    return next(c for c in cases() if c[0] == name)
