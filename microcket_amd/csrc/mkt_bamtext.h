// mkt_bamtext.h -- the half of the BAM-to-SAM-text decoder (mkt_bamtext.hip) that host and device share: the reasons a
// stream is refused for, the header walk (host), the plausibility test and the chain walk of the record index, its resolve step, the
// validation of one record with the length of its SAM line, and the routines that write the line.  tests/host/bamtext_host.cpp runs the
// same functions serially on the CPU; tests/bamtextdef.py states in Python what they have to give.
//
// The input is the inflated BAM stream (SAMv1 4.2).  Records are not aligned in it, so every field is put together from single bytes:
// no pointer into the stream is ever dereferenced as anything wider than a byte.  Every function says which bytes it may read; none
// reads at or past the `n` or `end` it is given.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define MKT_BT_HD __host__ __device__
#else
#define MKT_BT_HD
#endif

namespace mkt {

enum : uint32_t {
    BT_OK = 0, BT_BAD_MAGIC, BT_BAD_HEADER, BT_NO_SQ_LINES, BT_BLOCK_SMALL, BT_BLOCK_LARGE, BT_PAST_END, BT_REFID, BT_NAME, BT_CIGAR_OP,
    BT_TAG_OVERRUN, BT_TAG_TYPE, BT_B_SUBTYPE, BT_Z_UNTERMINATED, BT_CG_TAG, BT_TRUNCATED, BT_HEADER_TRUNCATED, BT_CIGAR_SEQ, BT_HEADER_NUL, BT_REASONS
};
inline const char* bt_reason_key(uint32_t r) {
    static const char* const k[BT_REASONS] = {"ok", "bad_magic", "bad_header", "no_sq_lines", "block_size_small", "block_size_large", "past_end", "ref_id", "read_name",
        "cigar_op", "tag_overrun", "tag_type", "b_subtype", "z_unterminated", "cg_tag", "truncated", "header_truncated", "cigar_seq_length", "header_nul"};
    return r < BT_REASONS ? k[r] : "?";
}
inline const char* bt_reason_text(uint32_t r) {
    static const char* const t[BT_REASONS] = {"ok", "no BAM stream (the magic bytes are not BAM\\1)", "the header is malformed (a negative length, or a reference name without its NUL)",
        "the header text has no @SQ line while the stream has references (samtools would make the lines up)", "block_size is below the 32 bytes of the fixed fields",
        "block_size exceeds max_record", "the name, CIGAR, SEQ and QUAL of the record pass its end", "refID or next_refID is below -1 or not below n_ref",
        "the read name is empty or does not end with a NUL", "a CIGAR operation code above 8", "the tags do not end exactly at the end of the record",
        "a tag type outside AcCsSiIfZHB", "a B array subtype outside cCsSiIf", "a Z or H tag without a NUL inside the record",
        "the record carries its CIGAR in a CG:B:I tag (samtools rewrites such a record)", "the stream ends inside a record", "the stream ends inside the header",
        "the CIGAR of a mapped record takes another number of bases than l_seq (samtools ends there)",
        "the header text holds a NUL in front of its last byte that is not NUL (samtools cuts and mends such a text)"};
    return r < BT_REASONS ? t[r] : "?";
}

constexpr uint32_t kBtFixed = 36;                        // block_size and the 32 bytes of fixed fields
constexpr uint32_t kBtChain = 3;                         // records a guessed start has to chain through
constexpr uint32_t kBtDefaultSegment = 256u << 10, kBtMinSegment = 256u;
constexpr uint32_t kBtMaxRecord = 16u << 20;
constexpr uint64_t kBtNone = ~0ull;
constexpr uint32_t kBtFloatSlot = 16;                    // bytes of one formatted float ("%g" of a float: at most 13)

MKT_BT_HD inline uint32_t bt_u16(const uint8_t* s, uint64_t o) { return (uint32_t)s[o] | ((uint32_t)s[o + 1] << 8); }
MKT_BT_HD inline uint32_t bt_u32(const uint8_t* s, uint64_t o) { return (uint32_t)s[o] | ((uint32_t)s[o + 1] << 8) | ((uint32_t)s[o + 2] << 16) | ((uint32_t)s[o + 3] << 24); }

struct BtRec {                                          // the fixed fields of the record at `off` (36 bytes read)
    uint32_t bs;
    int32_t refid, pos;
    uint32_t l_name, mapq, n_cig, flag, l_seq;
    int32_t nrefid, npos, tlen;
};
MKT_BT_HD inline BtRec bt_fixed(const uint8_t* s, uint64_t off) {
    BtRec r;
    r.bs = bt_u32(s, off);
    r.refid = (int32_t)bt_u32(s, off + 4);
    r.pos = (int32_t)bt_u32(s, off + 8);
    r.l_name = s[off + 12];
    r.mapq = s[off + 13];
    r.n_cig = bt_u16(s, off + 16);
    r.flag = bt_u16(s, off + 18);
    r.l_seq = bt_u32(s, off + 20);
    r.nrefid = (int32_t)bt_u32(s, off + 24);
    r.npos = (int32_t)bt_u32(s, off + 28);
    r.tlen = (int32_t)bt_u32(s, off + 32);
    return r;
}
MKT_BT_HD inline uint64_t bt_var_bytes(const BtRec& r) { return 32ull + r.l_name + 4ull * r.n_cig + (((uint64_t)r.l_seq + 1) >> 1) + r.l_seq; }

// ---- the record index -----------------------------------------------------------------------------------------------------------------
// Is `off` plausibly the start of a record, and the kBtChain records behind it too?  Reads only below n.  Where the data ends before the
// test can be made the answer is yes: a wrong yes costs a repair, never a wrong text.
MKT_BT_HD inline bool bt_plausible(const uint8_t* s, uint64_t n, uint64_t off, int32_t n_ref, uint32_t max_record) {
    for (uint32_t k = 0; k <= kBtChain; ++k) {
        if (off + kBtFixed > n) return true;
        const BtRec r = bt_fixed(s, off);
        if (r.bs > max_record || bt_var_bytes(r) > r.bs) return false;
        if (r.refid < -1 || r.refid >= n_ref || r.nrefid < -1 || r.nrefid >= n_ref || r.pos < -1 || r.l_name < 1) return false;
        const uint64_t nul = off + kBtFixed + r.l_name - 1;
        if (nul < n && s[nul] != 0) return false;
        off += 4ull + r.bs;
        if (off >= n) return true;
    }
    return true;
}

struct BtSeg {                                          // what a walk through one segment found
    uint64_t entry;                                     // the record start it began at (kBtNone: no start in this segment)
    uint64_t exit;                                      // status 0: the first record start at or past the segment's end; else the offset of the record that stopped it
    uint32_t count;                                     // complete records that start in the segment
    uint32_t status;                                    // 0; 1: the record at `exit` is not complete (the tail); else the reason the record at `exit` is refused for
};
// Walks the chain from `from` (< hi) to the first start at or past hi.  Every read lies below n: a record is counted only when it ends
// at or below n.
MKT_BT_HD inline BtSeg bt_walk(const uint8_t* s, uint64_t n, uint64_t from, uint64_t hi, uint32_t max_record) {
    BtSeg g;
    g.entry = from; g.count = 0; g.status = 0;
    uint64_t off = from;
    while (off < hi) {
        if (off + 4 > n) { g.status = 1; break; }
        const uint32_t bs = bt_u32(s, off);
        if (bs < 32) { g.status = BT_BLOCK_SMALL; break; }
        if (bs > max_record) { g.status = BT_BLOCK_LARGE; break; }
        if (off + 4 + bs > n) { g.status = 1; break; }
        ++g.count;
        off += 4ull + bs;
    }
    g.exit = off;
    return g;
}
struct BtIndex {
    uint64_t records, tail;                             // complete records; where they end (the carry begins there)
    uint64_t repairs;
    uint32_t reason; uint32_t pad;                      // 0, or why the record `bad_record` (an ordinal of this run) at bad_offset is refused
    uint64_t bad_record, bad_offset;
};
// The segments in order: a guess that did not begin where the segment before it ended is walked again from the true start.  After it
// seg[k] is the true walk of segment k (count 0 and entry kBtNone where a record spans it), whatever the guesses were.
MKT_BT_HD inline void bt_resolve(const uint8_t* s, uint64_t n, uint64_t start, uint64_t seg_bytes, uint64_t nseg, uint32_t max_record, BtSeg* seg, BtIndex* X) {
    uint64_t cur = start, total = 0, repairs = 0;
    bool done = false;
    X->reason = 0; X->pad = 0; X->bad_record = X->bad_offset = 0;
    for (uint64_t k = 0; k < nseg; ++k) {
        const uint64_t hi = start + (k + 1) * seg_bytes;
        if (done || cur >= hi) { seg[k].entry = kBtNone; seg[k].count = 0; seg[k].status = 0; seg[k].exit = cur; continue; }
        if (seg[k].entry != cur) { seg[k] = bt_walk(s, n, cur, hi, max_record); ++repairs; }
        total += seg[k].count;
        cur = seg[k].exit;
        if (seg[k].status == 1) done = true;
        else if (seg[k].status) { done = true; X->reason = seg[k].status; X->bad_record = total; X->bad_offset = cur; }
    }
    X->records = total; X->tail = cur; X->repairs = repairs;
}

// ---- one record -----------------------------------------------------------------------------------------------------------------------
MKT_BT_HD inline uint32_t bt_ndig(uint64_t v) { uint32_t d = 1; while (v >= 10) { v /= 10; ++d; } return d; }
MKT_BT_HD inline uint32_t bt_nint(int64_t v) { return v < 0 ? 1u + bt_ndig((uint64_t)(-v)) : bt_ndig((uint64_t)v); }
MKT_BT_HD inline uint32_t bt_put_u(uint8_t* d, uint64_t v) {
    const uint32_t n = bt_ndig(v);
    for (uint32_t k = n; k-- > 0;) { d[k] = (uint8_t)('0' + v % 10); v /= 10; }
    return n;
}
MKT_BT_HD inline uint32_t bt_put_i(uint8_t* d, int64_t v) {
    if (v < 0) { d[0] = '-'; return 1u + bt_put_u(d + 1, (uint64_t)(-v)); }
    return bt_put_u(d, (uint64_t)v);
}

struct BtTag {                                          // one tag, parsed: its payload lies inside the record
    uint8_t t0, t1, type, sub;
    uint32_t count;                                     // Z, H: bytes before the NUL; B: elements; else 1
    uint32_t size;                                      // bytes of one element
    uint64_t data;                                      // offset of the payload (B: of the first element)
    uint64_t next;                                      // offset behind the tag
};
MKT_BT_HD inline uint32_t bt_int_size(uint8_t t) { return (t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : (t == 'i' || t == 'I' || t == 'f') ? 4u : 0u; }
// the tag at p < end; reads only below end
MKT_BT_HD inline uint32_t bt_tag(const uint8_t* s, uint64_t p, uint64_t end, BtTag* T) {
    if (p + 3 > end) return BT_TAG_OVERRUN;
    T->t0 = s[p]; T->t1 = s[p + 1]; T->type = s[p + 2]; T->sub = 0; T->count = 1;
    p += 3;
    T->data = p;
    const uint8_t ty = T->type;
    if (ty == 'A') { T->size = 1; }
    else if (bt_int_size(ty)) { T->size = bt_int_size(ty); }
    else if (ty == 'Z' || ty == 'H') {
        uint64_t e = p;
        while (e < end && s[e]) ++e;
        if (e >= end) return BT_Z_UNTERMINATED;
        T->size = 1; T->count = (uint32_t)(e - p);      // below max_record
        T->next = e + 1;
        return BT_OK;
    } else if (ty == 'B') {
        if (p + 5 > end) return BT_TAG_OVERRUN;
        T->sub = s[p];
        T->size = bt_int_size(T->sub);
        if (!T->size) return BT_B_SUBTYPE;
        T->count = bt_u32(s, p + 1);
        T->data = p + 5;
        if (T->data + (uint64_t)T->count * T->size > end) return BT_TAG_OVERRUN;
        T->next = T->data + (uint64_t)T->count * T->size;
        if (T->t0 == 'C' && T->t1 == 'G' && T->sub == 'I') return BT_CG_TAG;
        return BT_OK;
    } else return BT_TAG_TYPE;
    if (p + T->size > end) return BT_TAG_OVERRUN;
    T->next = p + T->size;
    return BT_OK;
}
// element k of an integer tag or array as a signed 64-bit value
MKT_BT_HD inline int64_t bt_tag_int(const uint8_t* s, uint8_t ty, uint64_t o) {
    switch (ty) {
    case 'c': return (int8_t)s[o];
    case 'C': return s[o];
    case 's': return (int16_t)bt_u16(s, o);
    case 'S': return bt_u16(s, o);
    case 'i': return (int32_t)bt_u32(s, o);
    default: return bt_u32(s, o);
    }
}

struct BtRefs {                                         // the reference names: one byte table (no NULs) and n_ref + 1 offsets into it
    const uint8_t* names;
    const uint32_t* off;
    int32_t n_ref;
};
struct BtFloats {                                       // the floats of the stream in record order, as the host formatted them (nullptr: lengths count as 0)
    const uint8_t* str;                                 // kBtFloatSlot bytes each
    const uint8_t* len;
};
struct BtLine {
    uint64_t len;                                       // bytes of the SAM line, '\n' included
    uint32_t seq_at;                                    // where SEQ begins in the line
    uint32_t floats;                                    // f tags and elements of B:f arrays
};
MKT_BT_HD inline uint32_t bt_rname_len(const BtRefs& R, int32_t id) { return id < 0 ? 1u : R.off[id + 1] - R.off[id]; }
MKT_BT_HD inline uint32_t bt_name_len(const uint8_t* s, uint64_t at, uint32_t l_name) {      // bytes before the first NUL
    uint32_t k = 0;
    while (k < l_name && s[at + k]) ++k;
    return k;
}

// Validates the record at off (it is complete: off + 4 + block_size <= the data, block_size >= 32) and measures its line.  `fbase` is the
// index of the record's first float in F.  Reads only inside the record.
MKT_BT_HD inline uint32_t bt_record_len(const uint8_t* s, uint64_t off, const BtRefs& R, const BtFloats& F, uint64_t fbase, BtLine* L) {
    const BtRec r = bt_fixed(s, off);
    const uint64_t end = off + 4ull + r.bs;
    L->len = 0; L->seq_at = 0; L->floats = 0;
    if (bt_var_bytes(r) > r.bs) return BT_PAST_END;
    if (r.refid < -1 || r.refid >= R.n_ref || r.nrefid < -1 || r.nrefid >= R.n_ref) return BT_REFID;
    uint64_t p = off + kBtFixed;
    if (r.l_name < 1 || s[p + r.l_name - 1] != 0) return BT_NAME;
    uint64_t len = bt_name_len(s, p, r.l_name) + 1u;
    p += r.l_name;
    len += bt_ndig(r.flag) + 1u + bt_rname_len(R, r.refid) + 1u + bt_nint((int64_t)r.pos + 1) + 1u + bt_ndig(r.mapq) + 1u;
    if (!r.n_cig) len += 1;
    uint64_t qlen = 0;
    for (uint32_t k = 0; k < r.n_cig; ++k) {
        const uint32_t v = bt_u32(s, p + 4ull * k), op = v & 15u;
        if (op > 8u) return BT_CIGAR_OP;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) qlen += v >> 4;
        len += bt_ndig(v >> 4) + 1u;
    }
    if (r.n_cig && r.l_seq && !(r.flag & 4u) && qlen != r.l_seq) return BT_CIGAR_SEQ;
    p += 4ull * r.n_cig;
    len += 1u + ((r.nrefid >= 0 && r.nrefid == r.refid) ? 1u : bt_rname_len(R, r.nrefid)) + 1u + bt_nint((int64_t)r.npos + 1) + 1u + bt_nint(r.tlen) + 1u;
    L->seq_at = (uint32_t)len;                           // below 2^32: a name, ten numbers and at most 65535 operations
    len += (r.l_seq ? r.l_seq : 1u) + 1u;
    p += ((uint64_t)r.l_seq + 1) >> 1;
    len += (r.l_seq && s[p] != 0xFF) ? r.l_seq : 1u;
    p += r.l_seq;
    uint32_t nf = 0;
    while (p < end) {
        BtTag T;
        if (const uint32_t e = bt_tag(s, p, end, &T)) return e;
        if (T.type == 'A') len += 7;
        else if (T.type == 'Z' || T.type == 'H') len += 6ull + T.count;
        else if (T.type == 'f') { len += 6u + (F.len ? F.len[fbase + nf] : 0u); ++nf; }
        else if (T.type == 'B') {
            len += 7;
            if (T.sub == 'f') { for (uint32_t k = 0; k < T.count; ++k) len += 1u + (F.len ? F.len[fbase + nf + k] : 0u); nf += T.count; }
            else for (uint32_t k = 0; k < T.count; ++k) len += 1u + bt_nint(bt_tag_int(s, T.sub, T.data + (uint64_t)k * T.size));
        } else len += 6u + bt_nint(bt_tag_int(s, T.type, T.data));
        p = T.next;
    }
    L->len = len + 1;
    L->floats = nf;
    return BT_OK;
}
// the floats of a record that bt_record_len accepted, as their bits, in stored order
MKT_BT_HD inline void bt_record_floats(const uint8_t* s, uint64_t off, uint32_t* out) {
    const BtRec r = bt_fixed(s, off);
    const uint64_t end = off + 4ull + r.bs;
    uint64_t p = off + bt_var_bytes(r) + 4;
    uint32_t nf = 0;
    BtTag T;
    while (p < end && bt_tag(s, p, end, &T) == BT_OK) {
        if (T.type == 'f') out[nf++] = bt_u32(s, T.data);
        else if (T.type == 'B' && T.sub == 'f') for (uint32_t k = 0; k < T.count; ++k) out[nf++] = bt_u32(s, T.data + 4ull * k);
        p = T.next;
    }
}

// ---- writing the line of a record that bt_record_len accepted -------------------------------------------------------------------------
MKT_BT_HD inline uint32_t bt_put_rname(uint8_t* d, const BtRefs& R, int32_t id) {
    if (id < 0) { d[0] = '*'; return 1; }
    const uint32_t a = R.off[id], n = R.off[id + 1] - a;
    for (uint32_t k = 0; k < n; ++k) d[k] = R.names[a + k];
    return n;
}
// QNAME to TLEN and the tab in front of SEQ: L.seq_at bytes
MKT_BT_HD inline uint32_t bt_emit_head(const uint8_t* s, uint64_t off, const BtRefs& R, uint8_t* d) {
    const BtRec r = bt_fixed(s, off);
    uint64_t p = off + kBtFixed;
    uint32_t w = 0;
    const uint32_t nl = bt_name_len(s, p, r.l_name);
    for (uint32_t k = 0; k < nl; ++k) d[w++] = s[p + k];
    p += r.l_name;
    d[w++] = '\t'; w += bt_put_u(d + w, r.flag);
    d[w++] = '\t'; w += bt_put_rname(d + w, R, r.refid);
    d[w++] = '\t'; w += bt_put_i(d + w, (int64_t)r.pos + 1);
    d[w++] = '\t'; w += bt_put_u(d + w, r.mapq);
    d[w++] = '\t';
    if (!r.n_cig) d[w++] = '*';
    for (uint32_t k = 0; k < r.n_cig; ++k) {
        const uint32_t v = bt_u32(s, p + 4ull * k);
        w += bt_put_u(d + w, v >> 4);
        d[w++] = (uint8_t)"MIDNSHP=X"[v & 15u];          // <= 8: checked by bt_record_len
    }
    d[w++] = '\t';
    if (r.nrefid >= 0 && r.nrefid == r.refid) d[w++] = '='; else w += bt_put_rname(d + w, R, r.nrefid);
    d[w++] = '\t'; w += bt_put_i(d + w, (int64_t)r.npos + 1);
    d[w++] = '\t'; w += bt_put_i(d + w, r.tlen);
    d[w++] = '\t';
    return w;
}
// SEQ and QUAL are written in chunks of 8 characters, any chunk by any lane; a full chunk is one 8-byte store (memcpy: the line is not
// aligned).  Chunk j of SEQ reads the 4 bytes at seq + 4 j, chunk j of QUAL the 8 bytes at qual + 8 j: both inside the record.
MKT_BT_HD inline void bt_emit_seq_chunk(const uint8_t* s, uint64_t seq, uint32_t l_seq, uint32_t j, uint8_t* d) {
    const uint32_t i0 = 8u * j, m = l_seq - i0 < 8u ? l_seq - i0 : 8u;
    const char* const code = "=ACMGRSVTWYHKDBN";
    uint8_t c[8];
    for (uint32_t k = 0; k < m; k += 2) {
        const uint8_t b = s[seq + ((i0 + k) >> 1)];
        c[k] = (uint8_t)code[b >> 4];
        c[k + 1] = (uint8_t)code[b & 15u];               // (of an odd l_seq's last byte: not stored below)
    }
    if (m == 8) memcpy(d + i0, c, 8);
    else for (uint32_t k = 0; k < m; ++k) d[i0 + k] = c[k];
}
MKT_BT_HD inline void bt_emit_qual_chunk(const uint8_t* s, uint64_t qual, uint32_t l_seq, uint32_t j, uint8_t* d) {
    const uint32_t i0 = 8u * j, m = l_seq - i0 < 8u ? l_seq - i0 : 8u;
    if (m == 8) {
        uint64_t q = 0;
        for (uint32_t k = 0; k < 8; ++k) q |= (uint64_t)s[qual + i0 + k] << (8 * k);
        q = ((q & 0x7F7F7F7F7F7F7F7Full) + 0x2121212121212121ull) ^ (q & 0x8080808080808080ull);      // + 33 in every byte, no carry between them
        uint8_t c[8];
        for (uint32_t k = 0; k < 8; ++k) c[k] = (uint8_t)(q >> (8 * k));
        memcpy(d + i0, c, 8);
    } else for (uint32_t k = 0; k < m; ++k) d[i0 + k] = (uint8_t)(s[qual + i0 + k] + 33u);
}
struct BtBody { uint64_t seq, qual, tags, end; uint32_t l_seq; bool has_qual; };
MKT_BT_HD inline BtBody bt_body(const uint8_t* s, uint64_t off) {
    const BtRec r = bt_fixed(s, off);
    BtBody B;
    B.seq = off + kBtFixed + r.l_name + 4ull * r.n_cig;
    B.qual = B.seq + (((uint64_t)r.l_seq + 1) >> 1);
    B.tags = B.qual + r.l_seq;
    B.end = off + 4ull + r.bs;
    B.l_seq = r.l_seq;
    B.has_qual = r.l_seq && s[B.qual] != 0xFF;
    return B;
}
// what stands behind QUAL: the tags and the newline.  Returns the bytes written.
MKT_BT_HD inline uint64_t bt_emit_tags(const uint8_t* s, const BtBody& B, const BtFloats& F, uint64_t fbase, uint8_t* d) {
    uint64_t w = 0, p = B.tags;
    uint32_t nf = 0;
    BtTag T;
    while (p < B.end && bt_tag(s, p, B.end, &T) == BT_OK) {
        d[w++] = '\t'; d[w++] = T.t0; d[w++] = T.t1; d[w++] = ':';
        if (T.type == 'A' || T.type == 'Z' || T.type == 'H' || T.type == 'f' || T.type == 'B') d[w++] = T.type; else d[w++] = 'i';
        d[w++] = ':';
        if (T.type == 'A') d[w++] = s[T.data];
        else if (T.type == 'Z' || T.type == 'H') for (uint32_t k = 0; k < T.count; ++k) d[w++] = s[T.data + k];
        else if (T.type == 'f') {
            if (F.len) for (uint32_t k = 0; k < F.len[fbase + nf]; ++k) d[w++] = F.str[(fbase + nf) * kBtFloatSlot + k];
            ++nf;
        } else if (T.type == 'B') {
            d[w++] = T.sub;
            for (uint32_t k = 0; k < T.count; ++k) {
                d[w++] = ',';
                if (T.sub == 'f') { if (F.len) for (uint32_t x = 0; x < F.len[fbase + nf]; ++x) d[w++] = F.str[(fbase + nf) * kBtFloatSlot + x]; ++nf; }
                else w += bt_put_i(d + w, bt_tag_int(s, T.sub, T.data + (uint64_t)k * T.size));
            }
        } else w += bt_put_i(d + w, bt_tag_int(s, T.type, T.data));
        p = T.next;
    }
    d[w++] = '\n';
    return w;
}

// ---- the header (host) ----------------------------------------------------------------------------------------------------------------
struct BtHeader {
    std::string text;                                   // the l_text bytes as stored
    std::vector<std::string> names;
    std::vector<int32_t> lengths;
    uint64_t end = 0;                                   // the offset of the first record
};
constexpr uint32_t kBtIncomplete = 0xFFFFFFFFu;
// 0: walked (H filled); kBtIncomplete: d[0, n) ends inside the header; else the reason it is refused for.  Reads only below n.
inline uint32_t bt_header(const uint8_t* d, uint64_t n, BtHeader& H) {
    if (n < 4) return (n && memcmp(d, "BAM\1", n)) ? BT_BAD_MAGIC : kBtIncomplete;
    if (memcmp(d, "BAM\1", 4)) return BT_BAD_MAGIC;
    if (n < 8) return kBtIncomplete;
    const int32_t l_text = (int32_t)bt_u32(d, 4);
    if (l_text < 0) return BT_BAD_HEADER;
    uint64_t p = 8ull + (uint32_t)l_text;
    if (p + 4 > n) return kBtIncomplete;
    const int32_t n_ref = (int32_t)bt_u32(d, p);
    if (n_ref < 0) return BT_BAD_HEADER;
    p += 4;
    H.names.clear(); H.lengths.clear();
    for (int32_t k = 0; k < n_ref; ++k) {
        if (p + 4 > n) return kBtIncomplete;
        const int32_t l_name = (int32_t)bt_u32(d, p);
        if (l_name < 1) return BT_BAD_HEADER;
        if (p + 8ull + (uint32_t)l_name > n) return kBtIncomplete;
        if (d[p + 4 + (uint32_t)l_name - 1] != 0) return BT_BAD_HEADER;
        H.names.emplace_back((const char*)d + p + 4);    // up to its first NUL
        H.lengths.push_back((int32_t)bt_u32(d, p + 4 + (uint32_t)l_name));
        p += 8ull + (uint32_t)l_name;
    }
    H.text.assign((const char*)d + 8, (size_t)l_text);
    H.end = p;
    {
        size_t body = H.text.size();
        while (body && H.text[body - 1] == '\0') --body;
        if (H.text.find('\0') < body) return BT_HEADER_NUL;
    }
    if (n_ref > 0) {
        const std::string t = H.text.substr(0, H.text.find('\0'));
        if (t.compare(0, 4, "@SQ\t") && t.find("\n@SQ\t") == std::string::npos) return BT_NO_SQ_LINES;
    }
    return BT_OK;
}
// What `samtools view -H` prints for the stored text: its l_text bytes, NULs at the end included; where the text in front of those NULs
// is not empty and lacks its last newline, one stands in place of the first of them, or behind the text where there is none.
inline std::string bt_header_text(const std::string& stored) {
    size_t body = stored.size();
    while (body && stored[body - 1] == '\0') --body;
    std::string t = stored;
    if (body && stored[body - 1] != '\n') { if (body < t.size()) t[body] = '\n'; else t.push_back('\n'); }
    return t;
}
// "%g" of a float, as the host formats the side list
inline uint32_t bt_format_float(uint32_t bits, uint8_t* out /* kBtFloatSlot */) {
    float f;
    memcpy(&f, &bits, 4);
    char b[32];
    int n = snprintf(b, sizeof b, "%g", (double)f);
    if (n < 0) n = 0;
    if (n > (int)kBtFloatSlot) n = kBtFloatSlot;
    memcpy(out, b, (size_t)n);
    return (uint32_t)n;
}

}  // namespace mkt
