// Host driver for xfg-stark_amd/csrc/trace_layout.hpp (no HIP): the overflow-checked extent, the dense test,
// the gather of a host trace into [7][n] and the strided canonicity key, for every layout of
// tests/trace_layout_cases.py at n = 8 and 64. Built with ASan + UBSan (make build/asan/trace_layout) and run
// directly; a read outside a buffer that ends exactly at its extent is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../xfg-stark_amd/csrc/trace_layout.hpp"

using namespace xfg;
typedef uint64_t u64;

static int failures = 0;
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            failures++;                                            \
        }                                                          \
    } while (0)

struct Case {
    const char* name;
    TraceLayout at;
    u64 offset;  // words in front of cell (0, 0, 0)
};
static std::vector<Case> cases(u64 n, u64 count) {
    return {{"dense", {7 * n, n, 1}, 0},          {"rows7", {7 * n, 1, 7}, 0},
            {"rows8", {8 * n, 1, 8}, 0},          {"rows12+3", {12 * n, 1, 12}, 3},
            {"rows24", {24 * n, 1, 24}, 0},       {"cols_padded", {7 * (n + 8), n + 8, 1}, 0},
            {"batch_inner", {1, n * count, count}, 0}, {"broadcast", {0, n, 1}, 0}};
}
static u64 cell_value(u64 i, u64 c, u64 s) { return (i << 40) | (c << 32) | (s + 1); }  // canonical, all distinct

// the key of a dense trace, restated independently of trace_layout.hpp: the smallest key over the columns' first
// offenders
static u64 dense_key(const std::vector<u64>& tr, u64 n) {
    u64 key = TRACE_KEY_VALID;
    for (unsigned c = 0; c < 7; c++)
        for (u64 s = 0; s < n; s++)
            if (tr[c * n + s] >= TRACE_FIELD_P) {
                const u64 k = trace_key(TRACE_KEY_NONCANONICAL, s, c);
                key = k < key ? k : key;
                break;
            }
    return key;
}

static void test_extent() {
    u64 e = 0;
    const u64 n = 64;
    CHECK(trace_extent(dense_layout(n), 3, n, &e) && e == 3 * 7 * n);
    CHECK(trace_extent(TraceLayout{7 * n, 1, 7}, 3, n, &e) && e == 3 * 7 * n);
    CHECK(trace_extent(TraceLayout{8 * n, 1, 8}, 3, n, &e) && e == 3 * 8 * n - 1);  // no pad behind the last row
    CHECK(trace_extent(TraceLayout{0, 0, 0}, 65535, n, &e) && e == 1);              // all-zero strides: one word
    CHECK(trace_extent(TraceLayout{0, n, 1}, 5, n, &e) && e == 7 * n);
    CHECK(!trace_extent(dense_layout(n), 0, n, &e));
    CHECK(!trace_extent(dense_layout(n), 3, 0, &e));
    CHECK(!trace_extent(TraceLayout{1ULL << 63, n, 1}, 3, n, &e));   // 2 * 2^63 overflows
    CHECK(!trace_extent(TraceLayout{7 * n, 1ULL << 63, 1}, 1, n, &e));
    CHECK(!trace_extent(TraceLayout{7 * n, 1, 1ULL << 63}, 1, n, &e));
    CHECK(!trace_extent(TraceLayout{1ULL << 63, n, 1}, 2, n, &e));   // no overflow, above 2^58
    CHECK(!trace_extent(TraceLayout{1ULL << 50, n, 1}, 65535, n, &e));  // count = 65535 with a huge stride
    CHECK(!trace_extent(TraceLayout{~0ULL, ~0ULL, ~0ULL}, 2, n, &e));
    CHECK(trace_extent(TraceLayout{(1ULL << 58) - 7 * n, n, 1}, 2, n, &e) && e == (1ULL << 58));
    CHECK(!trace_extent(TraceLayout{(1ULL << 58) - 7 * n + 1, n, 1}, 2, n, &e));
    CHECK(is_dense(dense_layout(n), n) && is_dense(TraceLayout{7 * n, n, 1}, n));
    CHECK(!is_dense(TraceLayout{7 * n, 1, 7}, n) && !is_dense(TraceLayout{0, n, 1}, n) && !is_dense(dense_layout(n), 2 * n));
}

static void test_gather_and_key(u64 n) {
    const u64 count = 3;
    for (const Case& k : cases(n, count)) {
        u64 extent = 0;
        CHECK(trace_extent(k.at, count, n, &extent));
        // exactly offset + extent words on the heap: the sanitizer sees any read past the last cell
        std::vector<u64> buf(k.offset + extent, ~0ULL);
        u64* base = buf.data() + k.offset;
        for (u64 i = count; i-- > 0;)  // trace 0 last: with a broadcast layout every trace is trace 0
            for (u64 c = 0; c < 7; c++)
                for (u64 s = 0; s < n; s++) base[k.at.at(i, c, s)] = cell_value(k.at.trace_stride ? i : 0, c, s);
        for (u64 i = 0; i < count; i++) {
            std::vector<u64> got(7 * n, 0), want(7 * n);
            for (u64 c = 0; c < 7; c++)
                for (u64 s = 0; s < n; s++) want[c * n + s] = base[i * k.at.trace_stride + c * k.at.col_stride + s * k.at.row_stride];
            gather_trace(base + i * k.at.trace_stride, k.at, n, got.data());
            CHECK(got == want);
            CHECK(want[0] == cell_value(k.at.trace_stride ? i : 0, 0, 0) && want[6 * n + n - 1] == cell_value(k.at.trace_stride ? i : 0, 6, n - 1));
            CHECK(host_noncanonical_key(base + i * k.at.trace_stride, k.at, n) == TRACE_KEY_VALID);
        }
        // offenders in two columns of one step and in two steps: the first is by step, then by column
        struct Plant {
            u64 c, s;
        };
        const std::vector<std::vector<Plant>> plants = {
            {{5, 3}, {2, 3}}, {{1, n - 1}, {6, 4}}, {{0, 5}, {6, 2}, {3, 2}}, {{6, n - 1}}, {{0, 0}, {6, 0}}};
        for (const auto& plant : plants) {
            std::vector<u64> saved;
            for (const Plant& p : plant) {
                saved.push_back(base[k.at.at(1, p.c, p.s)]);
                base[k.at.at(1, p.c, p.s)] = TRACE_FIELD_P + p.c;
            }
            std::vector<u64> dense(7 * n);
            gather_trace(base + 1 * k.at.trace_stride, k.at, n, dense.data());
            const u64 key = host_noncanonical_key(base + 1 * k.at.trace_stride, k.at, n);
            CHECK(key == dense_key(dense, n) && key != TRACE_KEY_VALID);
            u64 fs = ~0ULL, fc = 0;
            for (const Plant& p : plant)
                if (p.s < fs || (p.s == fs && p.c < fc)) fs = p.s, fc = p.c;
            CHECK(key == trace_key(TRACE_KEY_NONCANONICAL, fs, (unsigned)fc));
            for (size_t j = plant.size(); j-- > 0;) base[k.at.at(1, plant[j].c, plant[j].s)] = saved[j];
        }
    }
}

int main() {
    test_extent();
    test_gather_and_key(8);
    test_gather_and_key(64);
    if (failures) {
        fprintf(stderr, "trace_layout: %d failures\n", failures);
        return 1;
    }
    printf("trace_layout ok\n");
    return 0;
}
