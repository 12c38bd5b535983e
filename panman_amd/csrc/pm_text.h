// pm_text.h -- host-only text plumbing of the extraction drivers (FASTA, VCF, MAF, GFA): the
// sink a driver writes its text through, the growing buffer behind the buffer-returning entry
// points and the cut of whole lines into device batches.  No HIP header: it compiles with a
// plain C++ compiler (tests/text_host_check.cpp).
#pragma once

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace pm {

// Where a driver's text goes, piece by piece in order; false: the write failed (errno says why).
using Sink = std::function<bool(const char*, size_t)>;

inline int digits_of(uint64_t v) {
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

// The text of pm_vcf / pm_maf / pm_gfa: appended through sink(), handed over by release() as a
// NUL-terminated malloc block (the caller's, released with free / pm_free).
class TextCollector {
    char* buf_ = nullptr;
    size_t used_ = 0, cap_ = 0;

    // room for `n` more bytes and the closing NUL; false (errno = ENOMEM): nothing changed
    bool reserve(size_t n) {
        if (used_ + n + 1 <= cap_) return true;
        const size_t want = std::max(used_ + n + 1, cap_ * 2);
        char* grown = static_cast<char*>(std::realloc(buf_, want));
        if (!grown) {
            errno = ENOMEM;
            return false;
        }
        buf_ = grown;
        cap_ = want;
        return true;
    }

public:
    TextCollector() = default;
    TextCollector(const TextCollector&) = delete;
    TextCollector& operator=(const TextCollector&) = delete;
    ~TextCollector() { std::free(buf_); }

    bool append(const char* q, size_t n) {
        if (!reserve(n)) return false;
        if (n) std::memcpy(buf_ + used_, q, n);
        used_ += n;
        return true;
    }
    Sink sink() {
        return [this](const char* q, size_t n) { return append(q, n); };
    }
    // Never null on success, also when nothing was appended; nullptr: out of memory (the text
    // stays with the collector).
    char* release() {
        if (!reserve(0)) return nullptr;
        char* out = buf_;
        out[used_] = 0;
        buf_ = nullptr;
        used_ = cap_ = 0;
        return out;
    }
};

// Items [i0, i1) of one device batch and the sum of their lengths.
struct Batch {
    int64_t i0, i1, bytes;
};

// Consecutive batches over len[0 .. n): a batch always takes its first item, then further items
// while bytes + len[i] <= limit and the batch's weight + weight(i) <= weight_limit (the launch
// grid's bound: workgroups or lines of the batch).
template <class Weight>
std::vector<Batch> cut_batches(const std::vector<int64_t>& len, int64_t limit, Weight weight, int64_t weight_limit) {
    const int64_t n = (int64_t)len.size();
    std::vector<Batch> batches;
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0 + 1, bytes = len[(size_t)i0], w = weight(i0);
        while (i1 < n && bytes + len[(size_t)i1] <= limit && w + weight(i1) <= weight_limit) {
            bytes += len[(size_t)i1];
            w += weight(i1);
            ++i1;
        }
        batches.push_back({i0, i1, bytes});
        i0 = i1;
    }
    return batches;
}

inline std::vector<Batch> cut_batches(const std::vector<int64_t>& len, int64_t limit) {
    return cut_batches(len, limit, [](int64_t) { return (int64_t)0; }, 0);
}

}  // namespace pm
