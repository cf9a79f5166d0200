// pairsgunzip_main.cpp -- the `bgzip -d -c` of this project: a BGZF file (final.pairs.gz, or any other) inflated on the GPU
// (mkt_bgzf_* of include/mkt.h has the definition).
//
//   pairsgunzip <in.pairs.gz | -> [out | -]
//
// The default output is stdout, so that  pairsgunzip a.pairs.gz | pairscmp - b.pairs  is the pipe the reference's script builds with
// pigz.  A file that is refused (not BGZF, a malformed deflate stream, a wrong CRC-32 or ISIZE) names the reason and the block's file
// offset on stderr and writes nothing.  The compressed bytes and the text are held in GPU memory.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_chunked_file.h"

static int usage(const char* a0) {
    fprintf(stderr, "\nUsage: %s <in.pairs.gz | -> [out | -]\n\nInflates a BGZF file on the GPU; the default output is stdout.\n"
                    "BGZF only (no plain gzip); the compressed bytes and the text are held in GPU memory.\n\n", a0);
    return 2;
}

int main(int argc, char* argv[]) {
    if (argc < 2 || argc > 3 || (argv[1][0] == '-' && argv[1][1])) return usage(argv[0]);
    const char* in = argv[1];
    const char* out = argc == 3 ? argv[2] : "-";
    const char* e = getenv("MKT_DEVICE");
    mkt_bgzf* p = nullptr;
    int rc = mkt_bgzf_create(e ? atoi(e) : 0, &p);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU inflate: %s\n", mkt_strerror(rc)); return 20; }
    std::vector<char> buf((size_t)32 << 20);
    FILE* f = strcmp(in, "-") ? fopen(in, "rb") : stdin;
    if (!f) { fprintf(stderr, "Error: cannot read %s\n", in); mkt_bgzf_destroy(p); return 10; }
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), f)) > 0)
        if ((rc = mkt_bgzf_add(p, buf.data(), got)) != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_bgzf_error(p)); mkt_bgzf_destroy(p); return 21; }
    if (f != stdin) fclose(f);
    mkt_bgzf_info info;
    rc = mkt_bgzf_run(p, nullptr, &info);
    if (rc != MKT_OK) {
        fprintf(stderr, "Error: %s: %s: %s\n", in, mkt_strerror(rc), mkt_bgzf_error(p));
        mkt_bgzf_destroy(p);
        return rc == MKT_E_FORMAT ? 3 : 21;
    }
    const bool to_stdout = !strcmp(out, "-");
    if (to_stdout) {
        for (uint64_t off = 0; off < info.text_bytes; off += buf.size()) {
            const size_t n = info.text_bytes - off < buf.size() ? (size_t)(info.text_bytes - off) : buf.size();
            if ((rc = mkt_bgzf_fetch_text(p, off, buf.data(), n)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(p)); mkt_bgzf_destroy(p); return 21; }
            if (fwrite(buf.data(), 1, n, stdout) != n) { fprintf(stderr, "Error: cannot write the output\n"); mkt_bgzf_destroy(p); return 11; }
        }
        if (fflush(stdout)) { fprintf(stderr, "Error: cannot write the output\n"); mkt_bgzf_destroy(p); return 11; }
    } else {
        mkt::ChunkedFile w(out);
        for (uint64_t off = 0; off < info.text_bytes; off += buf.size()) {
            const size_t n = info.text_bytes - off < buf.size() ? (size_t)(info.text_bytes - off) : buf.size();
            if ((rc = mkt_bgzf_fetch_text(p, off, buf.data(), n)) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_bgzf_error(p)); mkt_bgzf_destroy(p); return 21; }
            if (!w.append(buf.data(), n)) break;
        }
        if (!w.finish()) { fprintf(stderr, "Error: cannot write %s\n", out); mkt_bgzf_destroy(p); return 11; }
    }
    fprintf(stderr, "pairsgunzip: %llu blocks (%llu stored, %llu fixed, %llu dynamic deflate blocks), %llu -> %llu bytes%s\n", (unsigned long long)info.blocks,
            (unsigned long long)info.stored, (unsigned long long)info.fixed, (unsigned long long)info.dynamic, (unsigned long long)info.gz_bytes, (unsigned long long)info.text_bytes,
            info.has_eof ? "" : "; no EOF block");
    mkt_bgzf_destroy(p);
    return 0;
}
