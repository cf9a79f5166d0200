// ktrim_main.cpp -- bin/ktrim: drop-in for the driver's adapter and quality trimming step (microcket:371, 405, 413, 430, 444)
//     ktrim -k KIT -t T -o PREFIX -1 R1.fq -2 R2.fq -c | ...
// The reference's argv for its paired-end route.  With -c the interleaved FASTQ of the pairs kept goes to stdout, otherwise to
// PREFIX.read1.fq and PREFIX.read2.fq; PREFIX.trim.log is always written.  Everything is in input order.  The trimming runs on the GPU
// behind mkt_trim_* (include/mkt.h); this file only moves bytes: it reads both inputs piece by piece and hands each piece's output
// to a writer thread, so the output of one segment is written while the next is read and trimmed.
#include <cerrno>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <unistd.h>
#include "../../include/mkt.h"

static void usage() {
    fprintf(stderr, "\nUsage: ktrim [options] -1 <Read1.fq[,more]> -2 <Read2.fq[,more]> -o <out.prefix>\n"
                    "\nPaired-end adapter and quality trimming on the GPU (MI355X build), the argv of Ktrim 1.6.0:\n"
                    "  -1 / -2 files   FASTQ of read 1 / read 2; ',' separates several files, worked off in order; /dev/stdin is accepted\n"
                    "  -o prefix       PREFIX.trim.log, and without -c PREFIX.read1.fq / PREFIX.read2.fq\n"
                    "  -c              interleaved FASTQ to stdout\n"
                    "  -k kit          illumina (default) | nextera | transposase | bgi; wins over -a / -b\n"
                    "  -a / -b seq     adapter of read 1 / read 2 (8 .. 64 letters; -b defaults to -a)\n"
                    "  -s size         minimum read size kept (36; at least 10)     -p phred base (33)     -q minimum quality (20)\n"
                    "  -w window       cycles that must pass in a row (5)            -m mismatch proportion (0.125)\n"
                    "  -t threads      accepted and ignored                          -h / -v  help / version\n"
                    "Not supported: -U (single end), -f, -R, the CLIP kit, .gz inputs (put zcat in front).\n\n");
}
static bool write_all(int fd, const char* p, size_t n) {
    while (n) {
        const ssize_t k = write(fd, p, n);
        if (k < 0) { if (errno == EINTR) continue; return false; }
        p += k; n -= (size_t)k;
    }
    return true;
}
static std::vector<std::string> names(const char* list) {
    std::vector<std::string> v;
    std::string cur;
    for (const char* p = list;; ++p) {
        if (*p == ',' || *p == 0) { if (!cur.empty()) v.push_back(cur); cur.clear(); if (!*p) break; }
        else cur += *p;
    }
    return v;
}
static bool ends_with(const std::string& s, const char* e) { const size_t n = strlen(e); return s.size() >= n && s.compare(s.size() - n, n, e) == 0; }

// one side of the input: the files of a list as one stream (a file that does not end in a newline gets one)
struct Side {
    std::vector<std::string> files;
    size_t next = 0;
    FILE* f = nullptr;
    char last = '\n';
    bool eof = false;
    // up to cap bytes into buf; false on a file that cannot be opened or read
    bool fill(std::vector<char>& buf, size_t cap, size_t* got) {
        *got = 0;
        while (*got < cap && !eof) {
            if (!f) {
                if (next == files.size()) { eof = true; break; }
                f = fopen(files[next++].c_str(), "rb");
                if (!f) return false;
                last = '\n';
            }
            const size_t k = fread(buf.data() + *got, 1, cap - *got, f);
            if (k) { *got += k; last = buf[*got - 1]; continue; }
            if (ferror(f)) return false;
            fclose(f); f = nullptr;
            if (last != '\n') { buf[(*got)++] = '\n'; last = '\n'; }      // (cap leaves room: the buffers are one byte larger)
        }
        return true;
    }
};

// the writer: one piece of output at a time, handed over by the main thread
struct Writer {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> slot[3];
    bool full = false, stop = false, failed = false;
    int fd[3] = {-1, -1, -1};
    void run() {
        std::vector<char> mine[3];
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return full || stop; });
                if (!full) return;
                for (int k = 0; k < 3; ++k) mine[k].swap(slot[k]);
                full = false;
            }
            cv.notify_all();
            for (int k = 0; k < 3; ++k)
                if (fd[k] >= 0 && !mine[k].empty() && !write_all(fd[k], mine[k].data(), mine[k].size())) { std::lock_guard<std::mutex> lk(mu); failed = true; }
            for (int k = 0; k < 3; ++k) mine[k].clear();
        }
    }
};

int main(int argc, char* argv[]) {
    const char *in1 = nullptr, *in2 = nullptr, *prefix = nullptr, *kit = nullptr, *a1 = nullptr, *a2 = nullptr;
    long s = 36, p = 33, q = 20, w = 5;
    double m = 0.125;
    bool to_stdout = false;
    int opt;
    opterr = 0;
    while ((opt = getopt(argc, argv, "1:2:U:f:o:ck:a:b:s:p:q:w:m:t:Rhv")) != -1) {
        switch (opt) {
        case '1': in1 = optarg; break;
        case '2': in2 = optarg; break;
        case 'o': prefix = optarg; break;
        case 'c': to_stdout = true; break;
        case 'k': kit = optarg; break;
        case 'a': a1 = optarg; break;
        case 'b': a2 = optarg; break;
        case 's': s = strtol(optarg, nullptr, 10); break;
        case 'p': p = strtol(optarg, nullptr, 10); break;
        case 'q': q = strtol(optarg, nullptr, 10); break;
        case 'w': w = strtol(optarg, nullptr, 10); break;
        case 'm': m = strtod(optarg, nullptr); break;
        case 't': break;
        case 'h': usage(); return 0;
        case 'v': printf("ktrim (microcket_amd, MI355X build): the paired-end route of Ktrim 1.6.0\n"); return 0;
        case 'U': fprintf(stderr, "Error: -U (single-end data) is not supported by this build\n"); return 15;
        case 'f': fprintf(stderr, "Error: -f (a list file) is not supported by this build; use -1 / -2 with ',' between files\n"); return 15;
        case 'R': fprintf(stderr, "Error: -R is not supported by this build\n"); return 15;
        default: fprintf(stderr, "Error: unrecognized parameter!\n"); usage(); return 2;
        }
    }
    if (optind < argc) { fprintf(stderr, "Error: unrecognized parameter ('%s')!\n", argv[optind]); usage(); return 2; }
    if (!in1) { fprintf(stderr, "Error: No input file specified ('-1' is not set)!\n"); usage(); return 2; }
    if (!in2) { fprintf(stderr, "Error: -2 is not set: single-end data is not supported by this build\n"); return 15; }
    if (!prefix) { fprintf(stderr, "Error: No output file specified ('-o' not set)!\n"); usage(); return 3; }
    if (s < 10) { fprintf(stderr, "Error: invalid min_length! Must be at least 10!\n"); return 11; }
    if (p == 0 || q == 0 || w == 0) { fprintf(stderr, "Error: invalid phred/quality/window parameters!\n"); return 12; }
    if (s < 0 || p < 0 || q < 0 || w < 0 || s > 0x7fffffffL || p > 0x7fffffffL || q > 0x7fffffffL || w > 0x7fffffffL) { fprintf(stderr, "Error: -s, -p, -q and -w take positive numbers\n"); return 1; }
    mkt_trim_opts o;
    mkt_trim_default_opts(&o);
    o.min_size = (uint32_t)s; o.phred = (uint32_t)p; o.min_qual = (uint32_t)q; o.window = (uint32_t)w; o.mismatch = m;
    if (kit) {
        if (!strcmp(kit, "CLIP") || !strcmp(kit, "clip")) { fprintf(stderr, "Error: the CLIP kit is not supported by this build\n"); return 15; }
        if (a1) fprintf(stderr, "Warning: '-k' is set! '-a'/'-b' will be ignored!\n");
        o.kit = kit;
    } else {
        if (a2 && !a1) { fprintf(stderr, "Error: '-b' is set while '-a' is not set!\n"); return 14; }
        o.adapter1 = a1; o.adapter2 = a2;
    }
    char msg[256];
    if (mkt_trim_check(&o, msg, sizeof msg) != MKT_OK) {
        fprintf(stderr, "Error: %s\n", msg);
        return kit ? 13 : (strncmp(msg, "adapter size", 12) == 0 ? 20 : 1);
    }
    Side side[2];
    side[0].files = names(in1); side[1].files = names(in2);
    if (side[0].files.empty() || side[0].files.size() != side[1].files.size()) { fprintf(stderr, "Error: incorrect files!\n"); return 110; }
    for (const Side& sd : side) for (const std::string& f : sd.files)
        if (ends_with(f, ".gz")) { fprintf(stderr, "Error: %s: gzip-compressed input is not supported by this build; put zcat in front\n", f.c_str()); return 15; }
    FILE* flog = fopen((std::string(prefix) + ".trim.log").c_str(), "wb");
    if (!flog) { fprintf(stderr, "Error: cannot write log file!\n"); return 105; }
    Writer wr;
    FILE* fo[2] = {nullptr, nullptr};
    if (to_stdout) wr.fd[MKT_TRIM_INTERLEAVED] = 1;
    else {
        fo[0] = fopen((std::string(prefix) + ".read1.fq").c_str(), "wb");
        fo[1] = fopen((std::string(prefix) + ".read2.fq").c_str(), "wb");
        if (!fo[0] || !fo[1]) { fprintf(stderr, "Error: write file failed!\n"); return 103; }
        wr.fd[MKT_TRIM_READ1] = fileno(fo[0]); wr.fd[MKT_TRIM_READ2] = fileno(fo[1]);
    }
    const char* e = getenv("MKT_DEVICE");
    mkt_trim* t = nullptr;
    int rc = mkt_trim_create(e ? atoi(e) : 0, &t);
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU context: %s\n", mkt_strerror(rc)); return 120; }
    rc = mkt_trim_begin(t, &o);
    if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_trim_error(t)); return 121; }
    std::thread wthread([&] { wr.run(); });
    auto finish = [&](int code) {
        { std::lock_guard<std::mutex> lk(wr.mu); wr.stop = true; }
        wr.cv.notify_all();
        wthread.join();
        return code;
    };
    const size_t piece = (size_t)32 << 20;
    std::vector<char> buf[2] = {std::vector<char>(piece + 1), std::vector<char>(piece + 1)};
    std::vector<char> outb[3];
    uint64_t ob[3];
    for (;;) {
        size_t got[2] = {0, 0};
        for (int k = 0; k < 2; ++k)
            if (!side[k].fill(buf[k], piece, &got[k])) { fprintf(stderr, "Error: open fastq file failed!\n"); return finish(104); }
        const bool last = side[0].eof && side[1].eof;
        rc = mkt_trim_push(t, buf[0].data(), got[0], buf[1].data(), got[1], last ? 1 : 0, ob);
        if (rc != MKT_OK) { fprintf(stderr, "Error: %s: %s\n", mkt_strerror(rc), mkt_trim_error(t)); return finish(121); }
        bool any = false;
        for (int k = 0; k < 3; ++k) {
            outb[k].clear();
            if (wr.fd[k] < 0 || !ob[k]) continue;
            outb[k].resize((size_t)ob[k]);
            if (mkt_trim_fetch(t, k, 0, outb[k].data(), (size_t)ob[k]) != MKT_OK) { fprintf(stderr, "Error: %s\n", mkt_trim_error(t)); return finish(121); }
            any = true;
        }
        if (any) {
            std::unique_lock<std::mutex> lk(wr.mu);
            wr.cv.wait(lk, [&] { return !wr.full; });
            for (int k = 0; k < 3; ++k) wr.slot[k].swap(outb[k]);
            wr.full = true;
            lk.unlock();
            wr.cv.notify_all();
        }
        if (last) break;
    }
    {      // the writer takes the last piece, then stops
        std::unique_lock<std::mutex> lk(wr.mu);
        wr.cv.wait(lk, [&] { return !wr.full; });
    }
    finish(0);
    bool bad = wr.failed;
    for (int k = 0; k < 2; ++k) if (fo[k] && fclose(fo[k]) != 0) bad = true;
    if (bad) { fprintf(stderr, "Error: write file failed!\n"); return 103; }
    uint64_t st[6] = {0, 0, 0, 0, 0, 0};
    mkt_trim_stats(t, &st[0], &st[1], &st[2], &st[3], &st[4], &st[5]);
    static const char* const nm[6] = {"Total", "Dropped", "Aadaptor", "TailHit", "Dimer", "Pass"};
    for (int k = 0; k < 6; ++k) fprintf(flog, "%s\t%llu\n", nm[k], (unsigned long long)st[k]);
    if (fclose(flog) != 0) { fprintf(stderr, "Error: cannot write log file!\n"); return 105; }
    mkt_trim_destroy(t);
    return 0;
}
