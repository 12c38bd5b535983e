// The host-only text plumbing (panman_amd/csrc/pm_text.h) under AddressSanitizer, the leak
// checker and UBSan: the text collector behind pm_vcf / pm_maf / pm_gfa and the batch cutter of
// the extraction drivers.  Stand-alone; built and run by tests/test_text_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../panman_amd/csrc/pm_text.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// ---- collector -------------------------------------------------------------------------------

void collector_empty() {
    pm::TextCollector out;
    char* text = out.release();
    CHECK(text != nullptr);
    if (text) CHECK(text[0] == 0);
    std::free(text);
}

void collector_zero_byte_appends() {
    pm::TextCollector out;
    const pm::Sink sink = out.sink();
    CHECK(sink(nullptr, 0));
    CHECK(sink("", 0));
    char* text = out.release();
    CHECK(text != nullptr);
    if (text) CHECK(text[0] == 0);
    std::free(text);
    // ... and between real ones
    pm::TextCollector mixed;
    CHECK(mixed.append("ab", 2) && mixed.append("", 0) && mixed.append("c", 1) && mixed.append(nullptr, 0));
    text = mixed.release();
    CHECK(text && std::strcmp(text, "abc") == 0);
    std::free(text);
}

// The collector keeps room for the text and its NUL and grows to max(used + n + 1, 2 * cap):
// the running total is brought to exactly cap + delta (delta = -1, 0, 1) of every capacity on
// the way up to `stop`, one more byte follows each time, and the text is released at such an edge.
void collector_doubling_edges(int delta, size_t stop) {
    pm::TextCollector out;
    const pm::Sink sink = out.sink();
    std::string want;
    size_t cap = 0;   // the collector's capacity, by its rule
    uint32_t state = 12345u + (uint32_t)delta;
    auto add = [&](size_t n) {
        std::string piece(n, '\0');
        for (char& ch : piece) {
            state = state * 1664525u + 1013904223u;
            ch = (char)('!' + (state >> 24) % 90);
        }
        if (want.size() + n + 1 > cap) cap = std::max(want.size() + n + 1, cap * 2);
        want += piece;
        CHECK(sink(piece.data(), piece.size()));
    };
    auto to_edge = [&]() {
        const size_t target = (size_t)((int64_t)cap + delta);
        if (target > want.size()) add(target - want.size());
    };
    add(3);
    while (cap < stop) {
        to_edge();
        add(1);
    }
    to_edge();
    char* text = out.release();
    CHECK(text != nullptr);
    if (text) {
        CHECK(std::memcmp(text, want.data(), want.size()) == 0);
        CHECK(text[want.size()] == 0);
    }
    std::free(text);
}

void collector_dropped() {   // the leak checker is the assertion
    pm::TextCollector out;
    CHECK(out.append("never released", 14));
    std::string big(100000, 'x');
    CHECK(out.append(big.data(), big.size()));
}

void collector_released_twice() {   // a second release hands out a fresh empty text
    pm::TextCollector out;
    CHECK(out.append("x", 1));
    char* a = out.release();
    char* b = out.release();
    CHECK(a && std::strcmp(a, "x") == 0);
    CHECK(b && b != a && b[0] == 0);
    std::free(a);
    std::free(b);
}

// ---- batch cutter ----------------------------------------------------------------------------

// The drivers' loop as it stood in pm_vcf.cpp, pm_maf.cpp and pm_gfa.cpp before they shared it.
std::vector<pm::Batch> restated(const std::vector<int64_t>& len, int64_t limit, const std::vector<int64_t>* weight,
                                int64_t weight_limit) {
    std::vector<pm::Batch> out;
    const int64_t n = (int64_t)len.size();
    for (int64_t e0 = 0; e0 < n;) {
        int64_t e1 = e0 + 1, bytes = len[(size_t)e0], w = weight ? (*weight)[(size_t)e0] : 0;
        while (e1 < n && bytes + len[(size_t)e1] <= limit && (!weight || w + (*weight)[(size_t)e1] <= weight_limit)) {
            bytes += len[(size_t)e1];
            if (weight) w += (*weight)[(size_t)e1];
            ++e1;
        }
        out.push_back({e0, e1, bytes});
        e0 = e1;
    }
    return out;
}

std::vector<pm::Batch> cut(const std::vector<int64_t>& len, int64_t limit, const std::vector<int64_t>* weight = nullptr,
                           int64_t weight_limit = 0) {
    const std::vector<pm::Batch> got =
        weight ? pm::cut_batches(len, limit, [&](int64_t i) { return (*weight)[(size_t)i]; }, weight_limit)
               : pm::cut_batches(len, limit);
    const std::vector<pm::Batch> want = restated(len, limit, weight, weight_limit);
    CHECK(got.size() == want.size());
    for (size_t k = 0; k < got.size() && k < want.size(); ++k)
        CHECK(got[k].i0 == want[k].i0 && got[k].i1 == want[k].i1 && got[k].bytes == want[k].bytes);
    // non-empty, consecutive, covering [0, n), bytes = the sums
    int64_t at = 0;
    for (const pm::Batch& b : got) {
        CHECK(b.i0 == at && b.i1 > b.i0 && b.i1 <= (int64_t)len.size());
        int64_t sum = 0;
        for (int64_t i = b.i0; i < b.i1 && i < (int64_t)len.size(); ++i) sum += len[(size_t)i];
        CHECK(sum == b.bytes);
        at = b.i1;
    }
    CHECK(at == (int64_t)len.size());
    return got;
}

void cutter_cases() {
    CHECK(cut({}, 4096).empty());
    {   // one item longer than the limit is its own batch
        const auto b = cut({5000}, 4096);
        CHECK(b.size() == 1 && b[0].bytes == 5000);
        const auto c = cut({1, 5000, 1}, 4096);
        CHECK(c.size() == 3);
    }
    {   // exactly the limit stays together, the next byte starts a new batch
        const auto b = cut({1000, 2000, 1096}, 4096);
        CHECK(b.size() == 1 && b[0].bytes == 4096);
        const auto c = cut({1000, 2000, 1096, 1}, 4096);
        CHECK(c.size() == 2 && c[0].i1 == 3 && c[1].bytes == 1);
        const auto d = cut({1000, 2000, 1097}, 4096);
        CHECK(d.size() == 2 && d[0].i1 == 2);
    }
    {
        const auto b = cut({4095, 1, 1, 4096, 4097, 0, 0, 1}, 4096);
        // {4095, 1} {1} {4096} {4097} {0, 0, 1}: a batch takes its first item, then what fits
        CHECK(b.size() == 5);
        if (b.size() == 5) {
            CHECK(b[0].i1 == 2 && b[0].bytes == 4096);
            CHECK(b[1].i1 == 3 && b[1].bytes == 1);
            CHECK(b[2].i1 == 4 && b[2].bytes == 4096);
            CHECK(b[3].i1 == 5 && b[3].bytes == 4097);
            CHECK(b[4].i1 == 8 && b[4].bytes == 1);
        }
    }
    {   // a weight limit that cuts before the byte limit does
        const std::vector<int64_t> len{10, 10, 10, 10, 10, 10, 10}, one(7, 1), mixed{1, 2, 3, 1, 5, 1, 1};
        const auto b = cut(len, 4096, &one, 3);
        CHECK(b.size() == 3 && b[0].i1 == 3 && b[1].i1 == 6 && b[2].i1 == 7);
        const auto c = cut(len, 4096, &mixed, 4);   // {1, 2} {3, 1} {5}: heavier than the limit, alone {1, 1}
        CHECK(c.size() == 4 && c[0].i1 == 2 && c[1].i1 == 4 && c[2].i1 == 5 && c[3].i1 == 7);
        const auto d = cut(len, 25, &one, 3);       // the byte limit first
        CHECK(d.size() == 4 && d[0].i1 == 2);
        const auto e = cut(len, 4096, &one, (int64_t)0x7fffffff);
        CHECK(e.size() == 1 && e[0].bytes == 70);
    }
    {   // zero-length items
        CHECK(cut({0}, 4096).size() == 1);
        CHECK(cut({0, 0, 0, 0}, 4096).size() == 1);
        const auto b = cut({0, 4096, 0, 1, 0}, 4096);
        CHECK(b.size() == 2 && b[0].i1 == 3 && b[1].bytes == 1);
        const auto c = cut({0, 0, 0}, 0);
        CHECK(c.size() == 1 && c[0].bytes == 0);
    }
    // digits_of, the other resident of the header
    CHECK(pm::digits_of(0) == 1 && pm::digits_of(9) == 1 && pm::digits_of(10) == 2 && pm::digits_of(99999) == 5 &&
          pm::digits_of(100000) == 6 && pm::digits_of(UINT64_MAX) == 20);
}

}  // namespace

int main() {
    collector_empty();
    collector_zero_byte_appends();
    for (const int delta : {-1, 0, 1})
        for (const size_t stop : {(size_t)4, (size_t)64, (size_t)1 << 16}) collector_doubling_edges(delta, stop);
    collector_dropped();
    collector_released_twice();
    cutter_cases();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("text host checks ok");
    return 0;
}
