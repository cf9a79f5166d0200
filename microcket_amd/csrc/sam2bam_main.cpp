// sam2bam -- the .sam -> sorted BAM + index tail of the pipeline on the GPU.
//
// Replaces, in the driver (microcket:533-540),
//     cat $samheader $sid.flash.sam $sid.unc.sam | samtools view -@ T --no-PG -b /dev/stdin | samtools sort -@ T -m 4G --no-PG -o $sid.valid.bam /dev/stdin
//     samtools index -@ T $sid.valid.bam
// by
//     sam2bam -o $sid.valid.bam $samheader $sid.flash.sam $sid.unc.sam
// The inputs are read one after the other as ONE SAM stream ("-" = stdin): its leading '@' lines are the header.  The work is
// mkt_bam_* of libmkt_hip.so (include/mkt.h); this file only moves bytes.
//   -o FILE   output BAM ("-" = stdout; then no index is written)        -u        keep the input order (samtools view -b): no sort, no index
//   -l N      0 = stored blocks, 1 = fixed Huffman codes, 2 = per-block codes (default)         -@ N      accepted and ignored (thread count of the tools it replaces)
//   --no-index                                                            -d N      GPU ordinal (default $MKT_DEVICE or 0)
//   -m SIZE   alignment text per sorted run (K/M/G suffixes, as samtools sort -m): runs are sorted on the GPU, spilled to
//             temporary files and merged on the GPU, so the input may be larger than HBM.  Without -m: one pass while the input
//             fits the GPU, runs from where it would not.
//   -T PREFIX temporary files PREFIX.runs / PREFIX.keys (default: beside the output; under $TMPDIR when the output is stdout)
// Exit codes: 0 ok, 2 usage, 10 input cannot be opened, 11 output cannot be opened, 20 no GPU, 21 GPU error, 22 write error
// (a temporary file included), 23 the input is not SAM (message on stderr).
#include <errno.h>
#include <chrono>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mkt.h"

static int usage() {
    fprintf(stderr, "usage: sam2bam [-o out.bam] [-u] [-l 0|1|2] [-m SIZE[K|M|G]] [-T prefix] [-@ threads] [--no-index] [-d device] <in.sam | -> [more.sam ...]\n");
    return 2;
}

// samtools' memory sizes: a number with an optional K, M or G suffix; 0 on anything else
static uint64_t parse_size(const char* s) {
    char* e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(s, &e, 10);
    if (errno || e == s || !(s[0] >= '0' && s[0] <= '9')) return 0;
    uint64_t mul = 1;
    if (*e == 'k' || *e == 'K') { mul = 1ull << 10; ++e; }
    else if (*e == 'm' || *e == 'M') { mul = 1ull << 20; ++e; }
    else if (*e == 'g' || *e == 'G') { mul = 1ull << 30; ++e; }
    if (*e || v > (~0ull >> 1) / mul) return 0;
    return (uint64_t)v * mul;
}
static int code_of(int rc) { return rc == MKT_E_ARG ? 23 : rc == MKT_E_IO ? 22 : 21; }

int main(int argc, char** argv) {
    std::string out = "-", tmp_prefix;
    uint64_t run_bytes = MKT_BAM_RUNS_AUTO;
    std::vector<std::string> in;
    int sorted = 1, level = 2, index = 1, device = getenv("MKT_DEVICE") ? atoi(getenv("MKT_DEVICE")) : 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&](const char* what) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "sam2bam: %s needs a value\n", what); exit(2); } return argv[++i]; };
        if (a == "-o") out = val("-o");
        else if (a == "-u") sorted = 0;
        else if (a == "-l") level = atoi(val("-l"));
        else if (a == "-@") (void)val("-@");
        else if (a == "-d") device = atoi(val("-d"));
        else if (a == "-m") { const char* v = val("-m"); run_bytes = parse_size(v); if (!run_bytes) { fprintf(stderr, "sam2bam: bad -m value %s\n", v); return 2; } }
        else if (a == "-T") tmp_prefix = val("-T");
        else if (a == "--no-index") index = 0;
        else if (a == "--no-PG" || a == "-b") continue;                       // (flags of the commands this replaces)
        else if (a == "-h" || a == "--help") return usage();
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "sam2bam: unknown option %s\n", a.c_str()); return usage(); }
        else in.push_back(a);
    }
    if (in.empty()) return usage();
    const bool verbose = getenv("MKT_VERBOSE") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!verbose) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[sam2bam] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    };
    mkt_bam* b = nullptr;
    int rc = mkt_bam_create(device, &b);
    mark("GPU context");
    if (rc != MKT_OK) { fprintf(stderr, "sam2bam: %s\n", mkt_strerror(rc)); return rc == MKT_E_NO_DEVICE ? 20 : 21; }
    int ofd = -1, out_err = 0;
    auto drop_out = [&]() {                                                   // a partly written output file does not stay behind
        if (ofd > 1) { close(ofd); ofd = -1; (void)unlink(out.c_str()); }
    };
    auto fail = [&](int code, const char* what) { fprintf(stderr, "sam2bam: %s: %s\n", what, mkt_bam_error(b)); drop_out(); mkt_bam_destroy(b); return code; };
    if (tmp_prefix.empty()) {
        if (out != "-") tmp_prefix = out + ".tmp";
        else { const char* td = getenv("TMPDIR"); tmp_prefix = std::string(td && td[0] ? td : "/tmp") + "/sam2bam." + std::to_string((long long)getpid()); }
    }
    rc = mkt_bam_spill(b, run_bytes, tmp_prefix.c_str(), sorted, level);
    if (rc != MKT_OK) return fail(21, "mkt_bam_spill");
    // Input: straight into the library's pinned buffers (two alternate: the copy to the GPU of one runs while the other fills); a
    // regular file is read by a few threads (pread of disjoint slices), a pipe as it comes.
    int io_threads = getenv("MKT_IO_THREADS") ? atoi(getenv("MKT_IO_THREADS")) : 8;
    if (io_threads < 1) io_threads = 1;
    // Output: opened when the first bytes are ready; the pieces of the BAM come in order from mkt_bam_pull
    bool oregular = false;
    off_t obase = 0;
    uint64_t woff = 0;
    auto open_out = [&]() -> bool {
        if (ofd >= 0) return true;
        ofd = out == "-" ? 1 : open(out.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (ofd < 0) { fprintf(stderr, "sam2bam: cannot open %s: %s\n", out.c_str(), strerror(errno)); out_err = 11; return false; }
        struct stat osb;
        // positioned parallel writes only into a regular file we may seek in: stdout redirected with >> (O_APPEND) or handed over at
        // an offset takes the bytes in order, from where it stands
        oregular = fstat(ofd, &osb) == 0 && S_ISREG(osb.st_mode);
        if (oregular && ofd == 1) {
            const int fl = fcntl(ofd, F_GETFL);
            obase = lseek(ofd, 0, SEEK_CUR);
            if (fl < 0 || (fl & O_APPEND) || obase < 0) { oregular = false; obase = 0; }
        }
        return true;
    };
    auto put = [&](const char* src, size_t n) -> bool {
        const uint64_t off = woff;
        bool bad = false;
        if (oregular && n >= ((size_t)8 << 20) && io_threads > 1) {          // a big chunk of a regular file: disjoint slices in parallel
            const size_t slice = ((n + (size_t)io_threads - 1) / (size_t)io_threads + 4095) & ~(size_t)4095;
            std::vector<std::thread> th;
            std::vector<int> badv((size_t)io_threads, 0);
            for (int t = 0; t < io_threads; ++t) {
                const size_t lo = (size_t)t * slice;
                if (lo >= n) break;
                const size_t hi = lo + slice < n ? lo + slice : n;
                th.emplace_back([&, t, lo, hi]() {
                    size_t done = lo;
                    while (done < hi) {
                        const ssize_t k = pwrite(ofd, src + done, hi - done, obase + (off_t)(off + done));
                        if (k < 0) { if (errno == EINTR) continue; badv[(size_t)t] = 1; break; }
                        done += (size_t)k;
                    }
                });
            }
            for (auto& x : th) x.join();
            for (int v : badv) bad = bad || v;
        } else {
            if (oregular && lseek(ofd, obase + (off_t)off, SEEK_SET) < 0) bad = true;
            size_t done = 0;
            while (!bad && done < n) {
                const ssize_t k = write(ofd, src + done, n - done);
                if (k < 0) { if (errno == EINTR) continue; bad = true; break; }
                done += (size_t)k;
            }
        }
        if (bad) { fprintf(stderr, "sam2bam: write error on %s\n", out.c_str()); out_err = 22; return false; }
        woff += n;
        return true;
    };
    auto put_ready = [&]() -> bool {                                        // every piece the library has ready now
        for (;;) {
            const char* src = nullptr;
            size_t n = 0;
            const int prc = mkt_bam_pull(b, &src, &n);
            if (prc != MKT_OK) { fprintf(stderr, "sam2bam: mkt_bam_pull: %s\n", mkt_bam_error(b)); out_err = code_of(prc); return false; }
            if (!n) return true;
            if (!open_out() || !put(src, n)) return false;
        }
    };
    {   // room for everything up front when the sizes are known
        size_t total = 0;
        bool known = true;
        for (const std::string& path : in) { struct stat sb; if (path != "-" && stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) total += (size_t)sb.st_size; else known = false; }
        if (known && total) { rc = mkt_bam_reserve(b, total + 64); if (rc != MKT_OK) return fail(21, "mkt_bam_reserve"); }
    }
    for (const std::string& path : in) {
        const int fd = path == "-" || path == "/dev/stdin" ? 0 : open(path.c_str(), O_RDONLY);
        if (fd < 0) { fprintf(stderr, "sam2bam: cannot open %s: %s\n", path.c_str(), strerror(errno)); drop_out(); mkt_bam_destroy(b); return 10; }
        struct stat sb;
        const bool regular = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
        off_t fpos = 0;
        for (;;) {
            char* win = nullptr;
            size_t cap = 0;
            rc = mkt_bam_window(b, &win, &cap);
            if (rc != MKT_OK) { if (fd) close(fd); return fail(21, "mkt_bam_window"); }
            size_t got = 0;
            bool last = false, bad = false;
            if (regular) {
                const size_t left = sb.st_size > fpos ? (size_t)(sb.st_size - fpos) : 0;
                const size_t want = left < cap ? left : cap;
                const size_t slice = ((want + (size_t)io_threads - 1) / (size_t)io_threads + 4095) & ~(size_t)4095;
                std::vector<std::thread> th;
                std::vector<int> badv((size_t)io_threads, 0);
                for (int t = 0; t < io_threads && slice; ++t) {
                    const size_t lo = (size_t)t * slice;
                    if (lo >= want) break;
                    const size_t hi = lo + slice < want ? lo + slice : want;
                    th.emplace_back([&, t, lo, hi]() {
                        size_t done = lo;
                        while (done < hi) {
                            const ssize_t k = pread(fd, win + done, hi - done, fpos + (off_t)done);
                            if (k <= 0) { if (k < 0 && errno == EINTR) continue; badv[(size_t)t] = 1; break; }
                            done += (size_t)k;
                        }
                    });
                }
                for (auto& x : th) x.join();
                for (int v : badv) bad = bad || v;
                got = want; fpos += (off_t)want; last = fpos >= sb.st_size;
            } else {
                while (got < cap) {
                    const ssize_t k = read(fd, win + got, cap - got);
                    if (k < 0) { if (errno == EINTR) continue; bad = true; break; }
                    if (k == 0) { last = true; break; }
                    got += (size_t)k;
                }
            }
            if (bad) { fprintf(stderr, "sam2bam: read error on %s\n", path.c_str()); if (fd) close(fd); drop_out(); mkt_bam_destroy(b); return 10; }
            if (got) { rc = mkt_bam_commit(b, got); if (rc != MKT_OK) { if (fd) close(fd); return fail(code_of(rc), "mkt_bam_commit"); } }
            if (!sorted && !put_ready()) { if (fd) close(fd); drop_out(); mkt_bam_destroy(b); return out_err; }          // input order with runs: pieces leave as they are ready
            if (last) break;
        }
        if (fd) close(fd);
    }
    mark("read + copy to the GPU");
    uint64_t nrec = 0, nbam = 0, nbai = 0;
    rc = mkt_bam_run(b, sorted, level, &nrec, &nbam, &nbai);
    if (rc != MKT_OK) return fail(code_of(rc), "mkt_bam_run");
    mark("mkt_bam_run");
    if (!put_ready() || !open_out()) { drop_out(); mkt_bam_destroy(b); return out_err; }
    uint64_t st[5] = {0, 0, 0, 0, 0};
    (void)mkt_bam_stats(b, st);
    nbam = woff; nbai = st[4];
    if (sorted && index && out != "-" && !nbai && mkt_bam_note(b)[0]) fprintf(stderr, "sam2bam: WARN: %s\n", mkt_bam_note(b));
    if (verbose) fprintf(stderr, "[sam2bam] runs %llu, temporary bytes %llu, peak device bytes %llu\n", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]);
    if (ofd == 1 && oregular && lseek(ofd, obase + (off_t)nbam, SEEK_SET) < 0) { fprintf(stderr, "sam2bam: write error on %s\n", out.c_str()); mkt_bam_destroy(b); return 22; }
    if (ofd != 1 && close(ofd) != 0) { fprintf(stderr, "sam2bam: write error on %s\n", out.c_str()); mkt_bam_destroy(b); return 22; }
    if (sorted && index && out != "-" && nbai) {
        const std::string ip = out + ".bai";
        FILE* fi = fopen(ip.c_str(), "wb");
        if (!fi) { fprintf(stderr, "sam2bam: cannot open %s: %s\n", ip.c_str(), strerror(errno)); mkt_bam_destroy(b); return 11; }
        const char* ib = nullptr;
        rc = mkt_bam_read(b, 1, 0, nbai, &ib);
        if (rc != MKT_OK) { fclose(fi); return fail(21, "mkt_bam_read"); }
        const bool okw = fwrite(ib, 1, nbai, fi) == nbai;
        if (fclose(fi) != 0 || !okw) { fprintf(stderr, "sam2bam: write error on %s\n", ip.c_str()); mkt_bam_destroy(b); return 22; }
    }
    mark("fetch + write");
    mkt_bam_destroy(b);
    mark("teardown");
    return 0;
}
