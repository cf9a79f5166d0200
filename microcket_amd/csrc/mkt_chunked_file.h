// ChunkedFile -- a text file written in pieces, so that a table of any size needs one bounded buffer: append() collects text and writes
// it out once the buffer has passed the threshold; the first piece truncates the file ("wb"), every later one appends ("ab"); finish()
// writes what is left, also when that is nothing (an empty table is still an empty file), and says whether every write went through.
// After a failed write nothing more is written.  Host only, no dependencies: tests/host/chunked_file.cpp drives it with a tiny threshold.
#pragma once
#include <cstddef>
#include <cstdio>
#include <string>
#include <utility>

namespace mkt {

// the whole of [p, p + n) into <fn>, opened with <mode>
inline bool write_file(const std::string& fn, const char* p, size_t n, const char* mode = "wb") {
    FILE* f = fopen(fn.c_str(), mode);
    if (!f) return false;
    const bool ok = (n == 0 || fwrite(p, 1, n, f) == n);
    return (fclose(f) == 0) && ok;
}

class ChunkedFile {
public:
    explicit ChunkedFile(std::string fn, size_t threshold = (size_t)32 << 20) : fn_(std::move(fn)), threshold_(threshold) {}
    std::string& text() { return buf_; }                     // append to it, then call wrote()
    bool wrote() { if (buf_.size() > threshold_) piece(); return ok_; }       // after a line: false once a write has failed
    bool append(const char* p, size_t n) { buf_.append(p, n); return wrote(); }
    bool append(const std::string& s) { return append(s.data(), s.size()); }
    bool finish() { return piece(); }

private:
    bool piece() {
        if (ok_) ok_ = write_file(fn_, buf_.data(), buf_.size(), first_ ? "wb" : "ab");
        first_ = false;
        buf_.clear();
        return ok_;
    }
    std::string fn_, buf_;
    size_t threshold_;
    bool first_ = true, ok_ = true;
};

}  // namespace mkt
