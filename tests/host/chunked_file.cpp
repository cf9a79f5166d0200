// chunked_file -- mkt::ChunkedFile (microcket_amd/csrc/mkt_chunked_file.h) with a threshold of 16 bytes, so that the branch the
// executables reach only past 32 MiB runs in every test: a file written in many pieces is the concatenation of what was appended; the
// first piece truncates a longer file that was there and the later ones do not; nothing appended is still an empty file; a path in a
// missing directory reports failure.  argv[1]: a directory to write in.  Prints "ok" and exits 0, or says what went wrong and exits 1.
// tests/test_chunked_file_host.py runs it plain and built with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <string>
#include "../../microcket_amd/csrc/mkt_chunked_file.h"

static int bad = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s\n", __LINE__, #x); ++bad; } } while (0)

static bool slurp(const std::string& fn, std::string& out) {
    out.clear();
    FILE* f = fopen(fn.c_str(), "rb");
    if (!f) return false;
    char buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    fclose(f);
    return true;
}

int main(int argc, char* argv[]) {
    if (argc != 2) { fprintf(stderr, "usage: chunked_file <directory>\n"); return 2; }
    const std::string dir = argv[1];
    std::string got, want;
    {   // many pieces, lines of every length around the threshold, over a longer file that was there before
        const std::string fn = dir + "/many.txt";
        CHECK(mkt::write_file(fn, std::string(5000, '#').data(), 5000));
        mkt::ChunkedFile f(fn, 16);
        size_t pieces = 0;
        for (int k = 0; k < 200; ++k) {
            const std::string line = std::string((size_t)(k % 37), (char)('a' + k % 26)) + "\n";
            want += line;
            if (k % 2) CHECK(f.append(line));
            else { f.text() += line; CHECK(f.wrote()); }
            if (f.text().empty()) ++pieces;
            CHECK(f.text().size() <= 16);                                   // never more than the threshold is kept
            CHECK(slurp(fn, got) && (pieces ? got + f.text() == want : got == std::string(5000, '#')));      // truncated by the first piece only
        }
        CHECK(pieces > 50);
        CHECK(f.finish());
        CHECK(slurp(fn, got) && got == want);
    }
    {   // exactly the threshold is not yet a piece; one byte more is
        const std::string fn = dir + "/edge.txt";
        mkt::ChunkedFile f(fn, 16);
        CHECK(f.append("0123456789abcdef", 16) && f.text().size() == 16 && !slurp(fn, got));
        CHECK(f.append("g", 1) && f.text().empty() && slurp(fn, got) && got == "0123456789abcdefg");
        CHECK(f.finish() && slurp(fn, got) && got == "0123456789abcdefg");
    }
    {   // one piece only: finish() truncates what was there
        const std::string fn = dir + "/one.txt";
        CHECK(mkt::write_file(fn, "a longer file than the new one", 30));
        mkt::ChunkedFile f(fn, 16);
        CHECK(f.append("short\n"));
        CHECK(f.finish() && slurp(fn, got) && got == "short\n");
    }
    {   // nothing appended: an empty file, also over one that was there
        const std::string fn = dir + "/empty.txt", fn2 = dir + "/emptied.txt";
        mkt::ChunkedFile f(fn, 16);
        CHECK(f.finish() && slurp(fn, got) && got.empty());
        CHECK(mkt::write_file(fn2, "old", 3));
        mkt::ChunkedFile g(fn2);                                            // the default threshold
        CHECK(g.finish() && slurp(fn2, got) && got.empty());
    }
    {   // a missing directory: the failure is reported by the piece that meets it, by every call after it, and by finish()
        mkt::ChunkedFile f(dir + "/no/such/dir/x.txt", 16);
        CHECK(f.append("0123456789abcdef", 16));
        CHECK(!f.append("g", 1));
        CHECK(!f.append("h", 1) && !f.wrote());
        CHECK(!f.finish());
        mkt::ChunkedFile g(dir + "/no/such/dir/y.txt", 16);
        CHECK(!g.finish());
        CHECK(!slurp(dir + "/no/such/dir/y.txt", got));
    }
    if (bad) return 1;
    puts("ok");
    return 0;
}
