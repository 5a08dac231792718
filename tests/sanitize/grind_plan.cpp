// Stand-alone driver of the proof-of-work search planner (xfg-stark_amd/csrc/grind_plan.hpp), built host-only
// with ASan + UBSan by `make -C xfg-stark_amd sanitize`. It walks grinding factor 0..32 x B = 1..4096 x a few
// compute-unit counts and fails unless
//   * the grid has at least one block and at most min(GRIND_BLOCKS_MAX, 8 per compute unit),
//   * it is no larger than the expected work B 2^grind asks for (one block per 1024 hashes, rounded up),
//   * chunk_log lies in the planner's range and the block size follows from it,
//   * max_nonce = 2^(grind + 8) >= 2^grind, formed without a shift overflow at grind = 32,
//   * the chunks tile [first, max_nonce]: chunk 0 starts at first, each chunk starts one past the previous
//     one's last nonce, the last ends at max_nonce -- for the prover's range (ends and samples of up to 2^32
//     chunks) and, chunk by chunk, for small ranges with odd ends, for every chunk_log a caller may force,
//     up to a range that ends at 2^64 - 1.
// Plans of the shapes the prover meets go to stdout, one per line (tests/test_grind_plan.py reads them).
#include <cstdint>
#include <cstdio>

#include "../../xfg-stark_amd/csrc/grind_plan.hpp"

using namespace xfg;

static int failures = 0;
#define CHECK(c, ...)                              \
    do {                                           \
        if (!(c)) {                                \
            if (failures++ < 20) {                 \
                std::fprintf(stderr, "FAIL %s: ", #c); \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fprintf(stderr, "\n");        \
            }                                      \
        }                                          \
    } while (0)

// chunk c against its neighbours
static void check_chunk(uint64_t first, uint64_t max_nonce, unsigned cl, uint64_t count, uint64_t c) {
    const uint64_t lo = grind_chunk_first(first, c, cl), hi = grind_chunk_last(first, max_nonce, c, cl);
    CHECK(lo >= first && lo <= hi && hi <= max_nonce && hi - lo < (1ULL << cl), "chunk %llu of [%llu, %llu] log %u",
          (unsigned long long)c, (unsigned long long)first, (unsigned long long)max_nonce, cl);
    if (c == 0) CHECK(lo == first, "first chunk of [%llu, ..] log %u", (unsigned long long)first, cl);
    if (c + 1 < count)
        CHECK(hi - lo == (1ULL << cl) - 1 && grind_chunk_first(first, c + 1, cl) == hi + 1, "gap or overlap after chunk %llu log %u",
              (unsigned long long)c, cl);
    else
        CHECK(hi == max_nonce, "last chunk %llu ends at %llu, not %llu", (unsigned long long)c, (unsigned long long)hi,
              (unsigned long long)max_nonce);
}
static void check_tiling(uint64_t first, uint64_t max_nonce, unsigned cl, bool every) {
    const uint64_t count = grind_chunk_count(first, max_nonce, cl);
    if (first > max_nonce) {
        CHECK(count == 0, "empty range has %llu chunks", (unsigned long long)count);
        return;
    }
    CHECK(count >= 1, "no chunk in [%llu, %llu]", (unsigned long long)first, (unsigned long long)max_nonce);
    if (every) {
        for (uint64_t c = 0; c < count; c++) check_chunk(first, max_nonce, cl, count, c);
        return;
    }
    const uint64_t picks[] = {0, 1, 2, count / 3, count / 2, count - 3, count - 2, count - 1};
    for (uint64_t c : picks)
        if (c < count) check_chunk(first, max_nonce, cl, count, c);
}

int main() {
    const unsigned cus_set[] = {1, 64, 256, 304};
    for (unsigned cus : cus_set)
        for (unsigned g = 0; g <= GRIND_MAX; g++)
            for (uint32_t B = 1; B <= 4096; B++) {
                const GrindPlan p = grind_plan(g, B, cus);
                const uint64_t cap = (uint64_t)cus * GRIND_BLOCKS_PER_CU < GRIND_BLOCKS_MAX ? (uint64_t)cus * GRIND_BLOCKS_PER_CU
                                                                                             : GRIND_BLOCKS_MAX;
                CHECK(p.blocks >= 1 && p.blocks <= cap, "blocks %u at g %u B %u cus %u", p.blocks, g, B, cus);
                // (blocks - 1) 1024 < B 2^g, in 128 bits: B 2^g reaches 2^44 here and 2^64 at the ABI's limit
                CHECK((unsigned __int128)(p.blocks - 1) * GRIND_BLOCK * GRIND_LANE_NONCES < ((unsigned __int128)B << g),
                      "grid %u over-scans g %u B %u", p.blocks, g, B);
                CHECK(p.chunk_log >= GRIND_PLAN_CHUNK_LOG_MIN && p.chunk_log <= GRIND_PLAN_CHUNK_LOG_MAX &&
                          p.chunk_log >= GRIND_CHUNK_LOG_MIN && p.chunk_log <= GRIND_CHUNK_LOG_MAX,
                      "chunk_log %u at g %u B %u", p.chunk_log, g, B);
                CHECK(p.block == grind_block_size(p.chunk_log) && p.block >= 64 && p.block <= GRIND_BLOCK && p.block % 64 == 0,
                      "block %u", p.block);
                CHECK(p.max_nonce == grind_max_nonce(g) && p.max_nonce >= (1ULL << g) && p.max_nonce == (1ULL << g) << GRIND_BOUND_LOG,
                      "max_nonce %llu at g %u", (unsigned long long)p.max_nonce, g);
                if (B == 1 || B == 32 || B == 4096) check_tiling(1, p.max_nonce, p.chunk_log, false);
                if (cus == 256 && (B == 1 || B == 5 || B == 32 || B == 64))
                    std::printf("grind=%u B=%u cus=%u : chunk_log=%u blocks=%u block=%u max_nonce=%llu\n", g, B, cus, p.chunk_log,
                                p.blocks, p.block, (unsigned long long)p.max_nonce);
            }
    // the ABI's extremes
    const GrindPlan big = grind_plan(GRIND_MAX, 0xFFFFFFFFu, 256);
    CHECK(big.blocks == GRIND_BLOCKS_MAX && big.chunk_log == GRIND_PLAN_CHUNK_LOG_MAX, "B = 2^32 - 1 at g 32");
    CHECK(grind_plan(0, 1, 0).blocks == 1, "no compute units reported");
    // every chunk of small ranges with odd ends, every chunk_log a caller may force
    const uint64_t firsts[] = {1, 2, 63, 64, 255, 256, 257, (1ULL << 32) - 300, ~0ULL - 70000};
    const uint64_t spans[] = {0, 1, 62, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 65537, 70000};
    for (unsigned cl = GRIND_CHUNK_LOG_MIN; cl <= GRIND_CHUNK_LOG_MAX; cl++) {
        for (uint64_t f : firsts)
            for (uint64_t s : spans) check_tiling(f, f + s, cl, true);
        check_tiling(1, ~0ULL, cl, false);
        check_tiling(~0ULL, ~0ULL, cl, true);
        check_tiling(2, 1, cl, true);  // empty
    }
    CHECK(grind_block_size(6) == 64 && grind_block_size(7) == 128 && grind_block_size(8) == 256 && grind_block_size(16) == 256,
          "block sizes");
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    return 0;
}
