// bamtext_host.cpp -- stand-alone driver of the shared half of the BAM-to-SAM decoder (microcket_amd/csrc/mkt_bamtext.h): the header walk,
// the plausibility test and the chain walk per segment, the resolve step, the validation and length of every record and the routines
// that write its line, serially, in the order the kernels run them.  No GPU, no HIP header.
//
//   bamtext_host <inflated.bam> <out.sam> [segment_bytes [max_record]]
//
// stdout: "ok <records> <text bytes> <segments> <repairs> <float records>\n", the lines in out.sam and the header text in out.sam.hdr;
// or "refused <reason key> <record ordinal> <offset>\n" and no out.sam.  Exit status 0 either way; 2 for a file that cannot be read or
// written.  Every buffer has exactly the size the length routines gave: a write past a line is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../microcket_amd/csrc/mkt_bamtext.h"

using namespace mkt;

static int refused(uint32_t reason, uint64_t rec, uint64_t off) {
    printf("refused %s %llu %llu\n", bt_reason_key(reason), (unsigned long long)rec, (unsigned long long)off);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || argc > 5) return 2;
    const uint64_t seg_bytes = argc > 3 ? strtoull(argv[3], nullptr, 10) : kBtDefaultSegment;
    const uint32_t max_record = argc > 4 ? (uint32_t)strtoul(argv[4], nullptr, 10) : kBtMaxRecord;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    // an exact copy on the heap: a read past the stream is the sanitizer's to find
    const uint64_t n = in.size();
    std::vector<uint8_t> exact(in.begin(), in.end());
    if (!n) return refused(BT_HEADER_TRUNCATED, 0, 0);
    const uint8_t* s = exact.data();
    BtHeader H;
    uint32_t r = bt_header(s, n, H);
    if (r == kBtIncomplete) return refused(BT_HEADER_TRUNCATED, 0, n);
    if (r) return refused(r, 0, 0);
    std::string tab;
    std::vector<uint32_t> noff(H.names.size() + 1, 0);
    for (size_t k = 0; k < H.names.size(); ++k) { tab += H.names[k]; noff[k + 1] = (uint32_t)tab.size(); }
    const BtRefs R = {(const uint8_t*)tab.data(), noff.data(), (int32_t)H.names.size()};
    const uint64_t start = H.end, nseg = (n - start + seg_bytes - 1) / seg_bytes;
    std::vector<BtSeg> seg(nseg);
    for (uint64_t k = 0; k < nseg; ++k) {                // the guess of every segment on its own
        const uint64_t lo = start + k * seg_bytes, hi = lo + seg_bytes;
        uint64_t entry = k ? kBtNone : start;
        for (uint64_t c = lo; k && c < hi && c < n; ++c) if (bt_plausible(s, n, c, R.n_ref, max_record)) { entry = c; break; }
        if (entry != kBtNone) seg[k] = bt_walk(s, n, entry, hi, max_record);
        else { seg[k].entry = seg[k].exit = kBtNone; seg[k].count = 0; seg[k].status = 0; }
    }
    BtIndex X;
    bt_resolve(s, n, start, seg_bytes, nseg, max_record, seg.data(), &X);
    if (X.reason) return refused(X.reason, X.bad_record, X.bad_offset);
    std::vector<uint64_t> rec;
    for (uint64_t k = 0; k < nseg; ++k) {
        uint64_t off = seg[k].entry;
        for (uint32_t i = 0; i < seg[k].count; ++i) { rec.push_back(off); off += 4ull + bt_u32(s, off); }
    }
    if (rec.size() != X.records) return 2;
    std::vector<BtLine> L(rec.size());
    std::vector<uint64_t> fbase(rec.size() + 1, 0);
    BtFloats F = {nullptr, nullptr};
    std::vector<uint8_t> fstr, flen;
    uint64_t frecs = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t i = 0; i < rec.size(); ++i) {
            if ((r = bt_record_len(s, rec[i], R, F, fbase[i], &L[i]))) return refused(r, i, rec[i]);
            fbase[i + 1] = fbase[i] + L[i].floats;
        }
        if (pass || !fbase[rec.size()]) break;
        std::vector<uint32_t> bits(fbase[rec.size()]);
        for (size_t i = 0; i < rec.size(); ++i) if (L[i].floats) { ++frecs; bt_record_floats(s, rec[i], bits.data() + fbase[i]); }
        fstr.assign(bits.size() * kBtFloatSlot, 0); flen.assign(bits.size(), 0);
        for (size_t k = 0; k < bits.size(); ++k) flen[k] = (uint8_t)bt_format_float(bits[k], fstr.data() + k * kBtFloatSlot);
        F.str = fstr.data(); F.len = flen.data();
    }
    if (X.tail != n) return refused(BT_TRUNCATED, X.records, X.tail);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    uint64_t total = 0;
    for (size_t i = 0; i < rec.size(); ++i) {
        std::vector<uint8_t> line(L[i].len);
        uint8_t* d = line.data();
        const BtBody B = bt_body(s, rec[i]);
        const uint32_t sa = L[i].seq_at, nch = (B.l_seq + 7u) >> 3;
        uint8_t* dq = d + sa + (B.l_seq ? B.l_seq : 1u) + 1u;
        for (uint32_t j = nch; j-- > 0;) bt_emit_seq_chunk(s, B.seq, B.l_seq, j, d + sa);      // any order
        if (B.has_qual) for (uint32_t j = 0; j < nch; ++j) bt_emit_qual_chunk(s, B.qual, B.l_seq, j, dq);
        if (bt_emit_head(s, rec[i], R, d) != sa) return 2;
        if (!B.l_seq) d[sa] = '*';
        d[sa + (B.l_seq ? B.l_seq : 1u)] = '\t';
        if (!B.has_qual) dq[0] = '*';
        uint8_t* dt = dq + (B.has_qual ? B.l_seq : 1u);
        if ((uint64_t)(dt - d) + bt_emit_tags(s, B, F, fbase[i], dt) != L[i].len) return 2;
        if (fwrite(d, 1, line.size(), o) != line.size()) return 2;
        total += line.size();
    }
    if (fclose(o)) return 2;
    const std::string ht = bt_header_text(H.text);
    FILE* h = fopen((std::string(argv[2]) + ".hdr").c_str(), "wb");
    if (!h || (ht.size() && fwrite(ht.data(), 1, ht.size(), h) != ht.size()) || fclose(h)) return 2;
    printf("ok %zu %llu %llu %llu %llu\n", rec.size(), (unsigned long long)total, (unsigned long long)nseg, (unsigned long long)X.repairs, (unsigned long long)frecs);
    return 0;
}
