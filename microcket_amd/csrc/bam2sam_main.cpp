// bam2sam_main.cpp -- the `samtools view` of this project: a BAM file inflated (mkt_bgzf_*) and decoded to SAM text (mkt_bamtext_*) on
// the GPU; include/mkt.h has both definitions.
//
//   bam2sam [-h | -H] <in.bam | ->
//
// stdout gets the bytes of `samtools view [-h | -H] in.bam`, so that  bam2sam x.bam | sam2pairs /dev/stdin ...  is the driver's line.
// The file is read in batches of whole BGZF members (the host walks BSIZE; MKT_BAM2SAM_BATCH bytes of the file per batch, 256 MiB by
// default); a batch is inflated on the device, decoded from the device text without a host trip, its lines written, and the record the
// batch ends in is carried into the next.  A file that is refused names the reason, the record's ordinal and its offset in the inflated
// stream on stderr, exit status 3; the lines of the batches before it are already written and stay written.  -H inflates members only
// until the header is complete and decodes no record, so that it prints the header of a file whose records are refused, as samtools does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_bamtext.h"

static int usage(const char* a0) {
    fprintf(stderr, "\nUsage: %s [-h | -H] <in.bam | ->\n\nDecodes a BAM file to SAM text on the GPU; stdout gets what `samtools view [-h | -H]` prints.\n"
                    "  -h  the header in front of the records\n  -H  the header only\n"
                    "The file is read in batches of whole BGZF members.  A file that is refused (exit status 3) names the reason, the record\n"
                    "and its offset in the inflated stream; whole batches already written stay written.\n\n", a0);
    return 2;
}
// the bytes of d[0, n) that are whole BGZF members (a member that does not look like one ends the walk: the reader names the reason)
static size_t whole_members(const unsigned char* d, size_t n) {
    size_t p = 0;
    while (p + 18 <= n) {
        if (d[p] != 0x1f || d[p + 1] != 0x8b || d[p + 2] != 8 || d[p + 3] != 4 || d[p + 10] != 6 || d[p + 11] != 0 || d[p + 12] != 'B' || d[p + 13] != 'C') return n;
        const size_t bsize = (size_t)(d[p + 16] | (d[p + 17] << 8)) + 1;
        if (p + bsize > n) break;
        p += bsize;
    }
    return p;
}

int main(int argc, char* argv[]) {
    int a = 1;
    bool with_header = false, only_header = false;
    if (a < argc && !strcmp(argv[a], "-h")) { with_header = true; ++a; }
    else if (a < argc && !strcmp(argv[a], "-H")) { with_header = only_header = true; ++a; }
    if (argc - a != 1 || (argv[a][0] == '-' && argv[a][1])) return usage(argv[0]);
    const char* in = argv[a];
    const char* e = getenv("MKT_DEVICE");
    const char* eb = getenv("MKT_BAM2SAM_BATCH");
    size_t batch = eb ? (size_t)strtoull(eb, nullptr, 10) : ((size_t)256 << 20);
    if (batch < 65536) batch = 65536;                    // a member has at most 64 KiB
    const int dev = e ? atoi(e) : 0;
    mkt_bgzf* z = nullptr;
    mkt_bamtext* r = nullptr;
    int rc = mkt_bgzf_create(dev, &z);
    if (rc == MKT_OK) rc = mkt_bamtext_create(dev, &r);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU BAM reader: %s\n", mkt_strerror(rc)); mkt_bgzf_destroy(z); return 20; }
    FILE* f = strcmp(in, "-") ? fopen(in, "rb") : stdin;
    if (!f) { fprintf(stderr, "Error: cannot read %s\n", in); mkt_bamtext_destroy(r); mkt_bgzf_destroy(z); return 10; }
    auto done = [&](int code) { if (f && f != stdin) fclose(f); mkt_bamtext_destroy(r); mkt_bgzf_destroy(z); return code; };
    std::vector<unsigned char> pend;
    std::vector<char> out((size_t)32 << 20);
    bool eof = false, header_written = false;
    if (only_header) {                                   // 64 KiB of the file at a time; the header is walked on the host (mkt_bamtext.h)
        std::vector<unsigned char> raw;
        mkt::BtHeader H;
        for (;;) {
            while (!eof && pend.size() < 65536) {
                const size_t have = pend.size();
                pend.resize(65536);
                const size_t got = fread(pend.data() + have, 1, 65536 - have, f);
                pend.resize(have + got);
                if (got == 0) eof = true;
            }
            const size_t cut = eof ? pend.size() : whole_members(pend.data(), pend.size());
            mkt_bgzf_info zi;
            memset(&zi, 0, sizeof zi);
            if (cut) {
                if ((rc = mkt_bgzf_add(z, (const char*)pend.data(), cut)) != MKT_OK || (rc = mkt_bgzf_run(z, nullptr, &zi)) != MKT_OK) {
                    fprintf(stderr, "Error: %s: %s: %s\n", in, mkt_strerror(rc), mkt_bgzf_error(z));
                    return done(rc == MKT_E_FORMAT ? 3 : 21);
                }
                const size_t have = raw.size();
                raw.resize(have + (size_t)zi.text_bytes);
                if (zi.text_bytes && (rc = mkt_bgzf_fetch_text(z, 0, (char*)raw.data() + have, (size_t)zi.text_bytes)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(z)); return done(21); }
                if ((rc = mkt_bgzf_clear(z)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(z)); return done(21); }
                pend.erase(pend.begin(), pend.begin() + (ptrdiff_t)cut);
            }
            const uint32_t hr = raw.empty() ? mkt::kBtIncomplete : mkt::bt_header(raw.data(), raw.size(), H);
            if (hr == mkt::kBtIncomplete && !eof) continue;
            if (hr) {
                const uint32_t why = hr == mkt::kBtIncomplete ? (uint32_t)mkt::BT_HEADER_TRUNCATED : hr;
                fprintf(stderr, "Error: %s: %s: record 0 at %zu: %s [%s]\n", in, mkt_strerror(MKT_E_FORMAT), hr == mkt::kBtIncomplete ? raw.size() : (size_t)0, mkt::bt_reason_text(why), mkt::bt_reason_key(why));
                return done(3);
            }
            const std::string h = mkt::bt_header_text(H.text);
            if (fwrite(h.data(), 1, h.size(), stdout) != h.size() || fflush(stdout)) { fprintf(stderr, "Error: cannot write the output\n"); return done(11); }
            return done(0);
        }
    }
    unsigned long long records = 0, batches = 0, repairs = 0;
    mkt_bamtext_info ti;
    while (!eof) {
        while (!eof && pend.size() < batch) {
            const size_t have = pend.size(), want = batch - have;
            pend.resize(have + want);
            const size_t got = fread(pend.data() + have, 1, want, f);
            pend.resize(have + got);
            if (got < want) eof = true;
        }
        const size_t cut = eof ? pend.size() : whole_members(pend.data(), pend.size());
        if (cut) {
            mkt_bgzf_info zi;
            if ((rc = mkt_bgzf_add(z, (const char*)pend.data(), cut)) != MKT_OK || (rc = mkt_bgzf_run(z, nullptr, &zi)) != MKT_OK) {
                fprintf(stderr, "Error: %s: %s: %s\n", in, mkt_strerror(rc), mkt_bgzf_error(z));
                return done(rc == MKT_E_FORMAT ? 3 : 21);
            }
            const void* d = nullptr;
            uint64_t n = 0;
            if ((rc = mkt_bgzf_device_text(z, &d, &n)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(z)); return done(21); }
            if ((rc = mkt_bamtext_add_device(r, d, n)) != MKT_OK || (rc = mkt_bamtext_run(r, nullptr, &ti)) != MKT_OK) {
                fprintf(stderr, "Error: %s: %s: %s\n", in, mkt_strerror(rc), mkt_bamtext_error(r));
                return done(rc == MKT_E_FORMAT ? 3 : 21);
            }
            if ((rc = mkt_bgzf_clear(z)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(z)); return done(21); }
            pend.erase(pend.begin(), pend.begin() + (ptrdiff_t)cut);
            ++batches; records += ti.records; repairs += ti.repairs;
            if (ti.header_done && !header_written) {
                header_written = true;
                if (with_header) {
                    uint64_t total = 0;
                    if ((rc = mkt_bamtext_fetch_header(r, 0, nullptr, 0, &total)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bamtext_error(r)); return done(21); }
                    std::string h((size_t)total, '\0');
                    if (total && (rc = mkt_bamtext_fetch_header(r, 0, &h[0], (size_t)total, nullptr)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bamtext_error(r)); return done(21); }
                    if (fwrite(h.data(), 1, h.size(), stdout) != h.size()) { fprintf(stderr, "Error: cannot write the output\n"); return done(11); }
                }
            }
            for (uint64_t off = 0; off < ti.text_bytes; off += out.size()) {
                const size_t m = ti.text_bytes - off < out.size() ? (size_t)(ti.text_bytes - off) : out.size();
                if ((rc = mkt_bamtext_fetch_text(r, off, out.data(), m)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bamtext_error(r)); return done(21); }
                if (fwrite(out.data(), 1, m, stdout) != m) { fprintf(stderr, "Error: cannot write the output\n"); return done(11); }
            }
        } else if (!eof && pend.size() >= batch) { fprintf(stderr, "Error: %s: no whole BGZF member in %zu bytes\n", in, pend.size()); return done(3); }
    }
    if ((rc = mkt_bamtext_finish(r, &ti)) != MKT_OK) {
        fprintf(stderr, "Error: %s: %s: %s\n", in, mkt_strerror(rc), mkt_bamtext_error(r));
        (void)fflush(stdout);
        return done(rc == MKT_E_FORMAT ? 3 : 21);
    }
    if (fflush(stdout)) { fprintf(stderr, "Error: cannot write the output\n"); return done(11); }
    fprintf(stderr, "bam2sam: %llu records in %llu batches, %llu index repairs\n", records, batches, repairs);
    return done(0);
}
