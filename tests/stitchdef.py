"""The definition of read stitching (the driver's `flash -m 10 -M 150 --interleaved-input -To -c - | deal.flash.pl - PREFIX`,
microcket:405-408 / 430-438) in plain Python / numpy, and a seeded generator of interleaved FASTQ for it.  This file is what
mkt_stitch_* (include/mkt.h) and bin/stitch are compared with byte for byte; it is itself pinned against the program it restates
by tests/golden/stitch_golden.json (made by tests/golden/make_stitch_golden.py) and, where that program is present, by a live run.

The rule (qualities are Phred values, byte - phred_offset):
  reading      letters are upper-cased, anything outside ACGT becomes N (shown that way in every output); the tag is read 1's header
               without '@' and without white space at its end; a combined pair's is cut at its LAST '/' if it has one, an
               uncombined pair's only loses a "/1" or "/2" at its very end ("a/b x" -> "a" combined, whole uncombined)
  orientation  read 2 is reverse-complemented, its qualities reversed
  candidates   offsets i = max(0, n1 - n2) .. n1 - m into read 1, overlap length n1 - i, in this order
  scoring      a position where either base is N is uncalled; eff = overlap - uncalled, mm = called positions that differ,
               mq = sum of min(q1, q2) over those; a candidate counts only if eff >= m
  comparing    float32: sl = min(eff, M), d = mm / sl, qs = mq / sl; best starts at d = x + 1, qs = 0; a candidate replaces the best
               when d <= best_d and (d < best_d or qs < best_qs); best_d > x after the scan: not combined
  combining    read 1 before the offset | the overlap | the rest of the reverse-complemented read 2.  In the overlap equal bases keep
               the base with max(q1, q2); different bases get max(|q1 - q2|, 2) and the base of the higher quality, on a tie read 2's
               unless that is N
  lines        combined: tag \\t seq \\t qual;  uncombined: tag \\t seq1 \\t qual1 \\t seq2 \\t qual2 (read 2 as it came in)
  second half  deal.flash.pl: combined -> PREFIX.ext.fq; uncombined with len(seq1) >= min_size + cut_tail -> PREFIX.cut.read{1,2}.fq
               with the last cut_tail characters cut from all four strings; PREFIX.stitch.stat
"""
import hashlib

import numpy as np

MAX_READ = 512          # MKT_STITCH_MAX_READ
MAX_M = 255             # MKT_STITCH_MAX_M: up to here comparing the float32 quotients and cross-multiplying integers agree
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_NORM = bytes(ord(chr(k).upper()) if chr(k).upper() in "ACGT" else ord("N") for k in range(256))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def header_of(line):
    """read 1's header line without '@' and the white space at its end"""
    return (line[1:] if line.startswith(b"@") else line).rstrip(b" \t\r\v\f")


def tag_of(header, combined=True):
    """the tag of a pair from header_of(): a combined pair's is cut at the last '/', an uncombined pair's keeps everything but a
    closing "/1" or "/2" """
    if combined:
        k = header.rfind(b"/")
        return header[:k] if k >= 0 else header
    return header[:-2] if header.endswith((b"/1", b"/2")) else header


def parse(text, phred=33):
    """-> [(header_of(read 1's header), seq1, qual1, seq2, qual2)] with the sequences normalised.  A last line without its newline still counts."""
    if not text:
        return []
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    if len(lines) % 8:
        raise ValueError(f"{len(lines)} lines: not whole read pairs (8 lines each)")
    out = []
    for k in range(0, len(lines), 8):
        s1, q1, s2, q2 = lines[k + 1], lines[k + 3], lines[k + 5], lines[k + 7]
        if len(s1) != len(q1) or len(s2) != len(q2):
            raise ValueError(f"pair {k // 8}: sequence and quality differ in length")
        if not s1 or not s2:      # (the program's own handling of empty reads is erratic, and deal.flash.pl misreads their lines)
            raise ValueError(f"pair {k // 8}: an empty read")
        if max(len(s1), len(s2)) > MAX_READ:
            raise ValueError(f"pair {k // 8}: a read of {max(len(s1), len(s2))} bases (limit {MAX_READ})")
        if any(not phred <= c <= phred + 93 for c in q1 + q2):
            raise ValueError(f"pair {k // 8}: a quality byte outside {phred} .. {phred + 93}")
        out.append((header_of(lines[k]), s1.translate(_NORM), q1, s2.translate(_NORM), q2))
    return out


def _best_offsets(pairs, m, M, x, phred):
    """For every pair the chosen offset into read 1, or -1.  All pairs at once: read 1 right-aligned and the reverse-complemented
    read 2 left-aligned in a common width, so the candidate of overlap length L is the same columns for every pair."""
    P = len(pairs)
    n1 = np.array([len(p[1]) for p in pairs], dtype=np.int64)
    n2 = np.array([len(p[3]) for p in pairs], dtype=np.int64)
    W = int(max(n1.max(), n2.max(), 1))
    a = np.full((P, W), ord("N"), dtype=np.uint8)
    qa = np.zeros((P, W), dtype=np.int64)
    b = np.full((P, W), ord("N"), dtype=np.uint8)
    qb = np.zeros((P, W), dtype=np.int64)
    for k, (_t, s1, q1, s2, q2) in enumerate(pairs):
        if s1:
            a[k, W - len(s1):] = np.frombuffer(s1, dtype=np.uint8)
            qa[k, W - len(s1):] = np.frombuffer(q1, dtype=np.uint8).astype(np.int64) - phred
        if s2:
            b[k, :len(s2)] = np.frombuffer(s2.translate(_COMP)[::-1], dtype=np.uint8)
            qb[k, :len(s2)] = np.frombuffer(q2[::-1], dtype=np.uint8).astype(np.int64) - phred
    best_d = np.full(P, np.float32(x) + np.float32(1), dtype=np.float32)
    best_q = np.zeros(P, dtype=np.float32)
    best_L = np.full(P, -1, dtype=np.int64)
    lim = np.minimum(n1, n2)
    for L in range(W, m - 1, -1):                      # offsets ascending = overlap lengths descending
        live = lim >= L
        if not live.any():
            continue
        ra, rb = a[:, W - L:], b[:, :L]
        called = (ra != ord("N")) & (rb != ord("N"))
        eff = called.sum(axis=1)
        diff = called & (ra != rb)
        mm = diff.sum(axis=1)
        mq = (np.minimum(qa[:, W - L:], qb[:, :L]) * diff).sum(axis=1)
        ok = live & (eff >= m)
        sl = np.minimum(eff, M).astype(np.float32)
        sl[sl == 0] = 1
        d = mm.astype(np.float32) / sl
        qs = mq.astype(np.float32) / sl
        take = ok & (d <= best_d) & ((d < best_d) | (qs < best_q))
        best_d[take] = d[take]
        best_q[take] = qs[take]
        best_L[take] = L
    off = np.where((best_L >= 0) & ~(best_d > np.float32(x)), n1 - best_L, -1)
    return off


def candidates(pair, m, M, phred=33):
    """[(offset, eff, mm, mq)] of one parsed pair, every candidate offset in scan order, by plain loops over the positions (those
    with eff < m are listed too; they do not count).  The second, slow statement of the scoring: tests/stitch_edge_cases.py works out
    from it which classes its inputs reach, and tests/test_stitch_edges_host.py holds it against _best_offsets.  (M and phred only
    bound and shift: sl = min(eff, M) is left to choose().)"""
    _t, s1, q1, s2, q2 = pair
    n1, n2 = len(s1), len(s2)
    r2, p2 = s2.translate(_COMP)[::-1], q2[::-1]
    out = []
    for i in range(max(0, n1 - n2), n1 - m + 1):
        eff = mm = mq = 0
        for c1, c2, a, b in zip(s1[i:], r2, q1[i:], p2):
            if c1 != 78 and c2 != 78:
                eff += 1
                if c1 != c2:
                    mm += 1
                    mq += (a if a < b else b) - phred
        out.append((i, eff, mm, mq))
    return out


def choose(cands, m, M, x):
    """The comparing rule on candidates(): the chosen offset, or -1."""
    one = np.float32(1)
    best_d, best_q, best = np.float32(x) + one, np.float32(0), -1
    for i, eff, mm, mq in cands:
        if eff < m:
            continue
        sl = np.float32(min(eff, M))
        d, qs = np.float32(mm) / sl, np.float32(mq) / sl
        if d <= best_d and (d < best_d or qs < best_q):
            best_d, best_q, best = d, qs, i
    return best if best >= 0 and not best_d > np.float32(x) else -1


def threshold(sl, x):
    """The largest mm for which float32(mm) / float32(sl) > float32(x) is false, searched up to MAX_READ as mkt_stitch.h does."""
    mm = 0
    while mm < MAX_READ and not np.float32(mm + 1) / np.float32(sl) > np.float32(x):
        mm += 1
    return mm


def _combine(s1, q1, s2, q2, i, phred):
    r2 = s2.translate(_COMP)[::-1]
    p2 = q2[::-1]
    L = len(s1) - i
    seq, qual = bytearray(s1[:i]), bytearray(q1[:i])
    for j in range(L):
        c1, c2, a, b = s1[i + j], r2[j], q1[i + j] - phred, p2[j] - phred
        if c1 == c2:
            seq.append(c1)
            qual.append(max(a, b) + phred)
        else:
            qual.append(max(abs(a - b), 2) + phred)
            if a > b:
                seq.append(c1)
            elif b > a:
                seq.append(c2)
            else:
                seq.append(c1 if c2 == ord("N") else c2)
    seq += r2[L:]
    qual += p2[L:]
    return bytes(seq), bytes(qual)


def kept(n, cut_tail):
    """Characters that deal.flash.pl's substr(s, 0, length(s) - cut_tail) keeps of n: a NEGATIVE length argument means "leave that
    many off the end", so a string shorter than cut_tail keeps 2 n - cut_tail characters, or none.  (Only read 2 can be that short.)"""
    return n - cut_tail if n >= cut_tail else max(2 * n - cut_tail, 0)


def stitch(text, m=10, M=150, x=0.25, phred=33, cut_tail=10, min_size=36):
    """-> dict(tab, ext, cut1, cut2, stat (all bytes), total, combined, uncombined, passed, percent (str, two decimals))"""
    if not (1 <= m <= M <= MAX_M and 0 <= x <= 1):
        raise ValueError("need 1 <= m <= M <= %d and 0 <= x <= 1" % MAX_M)
    pairs = parse(text, phred)
    tab, ext, c1, c2 = [], [], [], []
    comb = unc = passed = 0
    off = _best_offsets(pairs, m, M, x, phred) if pairs else []
    for (head, s1, q1, s2, q2), i in zip(pairs, off):
        tag = tag_of(head, i >= 0)
        if i >= 0:
            seq, qual = _combine(s1, q1, s2, q2, int(i), phred)
            comb += 1
            tab.append(tag + b"\t" + seq + b"\t" + qual + b"\n")
            ext.append(b"@" + tag + b"\n" + seq + b"\n+\n" + qual + b"\n")
        else:
            unc += 1
            tab.append(b"\t".join((tag, s1, q1, s2, q2)) + b"\n")
            if len(s1) >= min_size + cut_tail:
                passed += 1
                k1, k2 = len(s1) - cut_tail, kept(len(s2), cut_tail)
                c1.append(b"@" + tag + b"\n" + s1[:k1] + b"\n+\n" + q1[:k1] + b"\n")
                c2.append(b"@" + tag + b"\n" + s2[:k2] + b"\n+\n" + q2[:k2] + b"\n")
    total = comb + unc
    return dict(tab=b"".join(tab), ext=b"".join(ext), cut1=b"".join(c1), cut2=b"".join(c2),
                stat=b"Combined\t%d\tUncombined\t%d\tPass\t%d\n" % (comb, unc, passed),
                total=total, combined=comb, uncombined=unc, passed=passed, percent=percent(comb, total))


def by_kind(tab):
    """(the combined lines, the uncombined lines) of a tab stream, each in the stream's order.  stitch() and the GPU write the tab
    stream in INPUT order.  The program itself does not, even with one combiner thread: it hands combined and uncombined records
    to its writers in separate blocks of 35, so its stream alternates between runs of the two kinds -- but each kind by itself is
    in input order, and that is all deal.flash.pl's three files can see.  So a tab stream is compared with the program's kind by
    kind: every line, in order, none left out."""
    lines = tab.split(b"\n")[:-1]
    return (b"".join(l + b"\n" for l in lines if l.count(b"\t") == 2), b"".join(l + b"\n" for l in lines if l.count(b"\t") != 2))


def percent(comb, total):
    """'Percent combined' with two decimals: printf("%.2f") of the double 100 * comb / total (0.00 for no pairs)."""
    return "%.2f" % (100.0 * comb / total) if total else "0.00"


_B = np.frombuffer(b"ACGT", dtype=np.uint8)


def synth(seed, pairs, read_len=None):
    """Seeded interleaved FASTQ.  read_len None: the mixed classes -- read lengths 20 .. 160, unequal; fragments shorter than a read
    (the read runs on into random bases); 15 % tandem repeats (ties between offsets); substitution rates 0 .. 30 % with N among
    them; random and constant qualities; fragments too long to overlap.  read_len given: both reads that long, the same classes."""
    R = np.random.RandomState(seed)
    out = []
    for k in range(pairs):
        n1 = read_len or int(R.randint(20, 161))
        n2 = read_len or (n1 if R.rand() < 0.3 else int(R.randint(20, 161)))
        frag = int(R.randint(12, 2 * max(n1, n2) + 40))
        if R.rand() < 0.15:
            unit = _B[R.randint(0, 4, size=int(R.randint(1, 7)))]
            f = np.resize(unit, frag)
        else:
            f = _B[R.randint(0, 4, size=frag)]
        rc = np.frombuffer(f.tobytes().translate(_COMP)[::-1], dtype=np.uint8)
        reads = []
        rate = (0.0, 0.0, 0.01, 0.05, 0.1, 0.2, 0.3)[int(R.randint(0, 7))]
        const_q = R.rand() < 0.3
        for src, n in ((f, n1), (rc, n2)):
            s = src[:n].copy()
            if len(s) < n:
                s = np.concatenate([s, _B[R.randint(0, 4, size=n - len(s))]])
            hit = R.rand(n) < rate
            sub = np.frombuffer(b"ACGTN", dtype=np.uint8)[R.randint(0, 5, size=n)]
            s = np.where(hit, sub, s)
            q = np.full(n, 33 + int(R.randint(2, 41)), dtype=np.uint8) if const_q else (33 + R.randint(2, 42, size=n)).astype(np.uint8)
            reads.append((s.tobytes(), q.tobytes()))
        out.append(b"@p%d/1\n%s\n+\n%s\n@p%d/2\n%s\n+\n%s\n" % (k, reads[0][0], reads[0][1], k, reads[1][0], reads[1][1]))
    return b"".join(out)
