// The proof-of-work search on the device (grind.hip): when the prover uses it, how its nonces are cut
// into chunks, and the launch geometry. Pure functions, no HIP (tests/sanitize/grind_plan.cpp compiles
// this header with a plain host compiler), like ntt_plan.hpp.
//
// The rule. A unit of B proofs at grinding factor g expects W = B 2^g hashes in all.
//   grid      one block of GRIND_BLOCK lanes per GRIND_BLOCK * GRIND_LANE_NONCES expected hashes, so a
//             small search is not over-scanned by lanes that had nothing to find; at least 1, at most
//             min(GRIND_BLOCKS_MAX, GRIND_BLOCKS_PER_CU * CUs) blocks (8 waves per SIMD at 256 CUs)
//   chunk     2^chunk_log nonces, what a block claims at a time. A proof is worked on by about
//             P = max(1, blocks / B) blocks at once, and when its nonce is found up to P chunks are in
//             flight beyond it: chunk_log = g - 2 - ceil(log2 P) keeps that at a quarter of the 2^g
//             hashes the proof expects, within [GRIND_PLAN_CHUNK_LOG_MIN, GRIND_PLAN_CHUNK_LOG_MAX]
//             (one pass of a block; 64 passes: a block checks `best` every fourth pass, and a longer chunk
//             only saves claims, of which a proof at g = 32 already takes only 2^18)
//   bound     max_nonce = 2^(g + GRIND_BOUND_LOG): no nonce above it is tested. A search fails to find
//             a nonce below it with probability (1 - 2^-g)^(2^(g + 8)) ~ e^-256
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XFG_GRIND_HD __host__ __device__
#else
#define XFG_GRIND_HD
#endif

namespace xfg {

// The smallest grinding factor whose nonce the prover searches on the device; below it the host loop
// of plan_queries runs as it always has (the reference's factors 4 and 8 among them).
// Measurement behind the value (DESIGN.md 7 "Grinding on the device", profiles/r09/grind_min_ab.txt): two
// builds differing in this constant alone, ST_HQUERY of 32-proof units at n = 2^16, blowup 8 on one MI355X,
// medians of six units, two runs each. Factor 9: device 0.34 / 0.43 ms, host 0.31 / 0.29 (host ahead);
// 10: 0.28 / 0.37 against 0.42 / 0.42; 11: 0.28 / 0.40 against 0.71 / 0.58; 16: 0.52 / 0.63 against
// 13.5 / 12.9. 10 is the smallest factor at which the device search is not slower.
constexpr unsigned GRIND_DEVICE_MIN = 10;

constexpr unsigned GRIND_MAX = 32;  // ProofOptions::new: grinding factor <= 32
constexpr unsigned GRIND_BLOCK = 256;
constexpr unsigned GRIND_LANE_NONCES = 4;
constexpr unsigned GRIND_BLOCKS_MAX = 2048, GRIND_BLOCKS_PER_CU = 8;
constexpr unsigned GRIND_PLAN_CHUNK_LOG_MIN = 8, GRIND_PLAN_CHUNK_LOG_MAX = 14;
constexpr unsigned GRIND_BOUND_LOG = 8;
// what a caller may force (xfg_debug_grind)
constexpr unsigned GRIND_CHUNK_LOG_MIN = 6, GRIND_CHUNK_LOG_MAX = 16, GRIND_FORCED_BLOCKS_MAX = 4096;

struct GrindPlan {
    unsigned chunk_log, blocks, block;
    uint64_t max_nonce;
};

// the prover's bound: 2^(grind + 8) <= 2^40
XFG_GRIND_HD constexpr uint64_t grind_max_nonce(unsigned grind) { return 1ULL << (grind + GRIND_BOUND_LOG); }
// lanes of a block: a chunk shorter than GRIND_BLOCK is one pass of a smaller block
XFG_GRIND_HD constexpr unsigned grind_block_size(unsigned chunk_log) {
    return chunk_log >= 8 ? GRIND_BLOCK : 1u << chunk_log;
}

// ---- chunks: chunk c of a search over [first, max_nonce] is [first + c 2^chunk_log, ...], the last one
// cut at max_nonce. chunk_log >= 1, so the count fits 64 bits for any range.
XFG_GRIND_HD constexpr uint64_t grind_chunk_count(uint64_t first, uint64_t max_nonce, unsigned chunk_log) {
    return first > max_nonce ? 0 : ((max_nonce - first) >> chunk_log) + 1;
}
// for c < grind_chunk_count: no overflow, (c << chunk_log) <= max_nonce - first
XFG_GRIND_HD constexpr uint64_t grind_chunk_first(uint64_t first, uint64_t c, unsigned chunk_log) {
    return first + (c << chunk_log);
}
XFG_GRIND_HD constexpr uint64_t grind_chunk_last(uint64_t first, uint64_t max_nonce, uint64_t c, unsigned chunk_log) {
    const uint64_t lo = grind_chunk_first(first, c, chunk_log), room = max_nonce - lo, len1 = (1ULL << chunk_log) - 1;
    return lo + (room < len1 ? room : len1);
}

constexpr unsigned grind_ceil_log2(uint64_t x) {
    unsigned r = 0;
    while (r < 63 && (1ULL << r) < x) r++;
    return r;
}

// grind <= GRIND_MAX, B >= 1; cus: compute units of the device (0 is taken as 1)
constexpr GrindPlan grind_plan(unsigned grind, uint32_t B, unsigned cus) {
    constexpr unsigned per_block_log = 10;  // log2(GRIND_BLOCK * GRIND_LANE_NONCES)
    static_assert(GRIND_BLOCK * GRIND_LANE_NONCES == 1u << per_block_log, "per_block_log");
    // ceil(B 2^grind / 2^10) without forming B 2^grind (2^64 at B = 2^32, grind = 32)
    const uint64_t want = grind >= per_block_log ? (uint64_t)B << (grind - per_block_log)
                                                 : (((uint64_t)B << grind) + (1u << per_block_log) - 1) >> per_block_log;
    const uint64_t by_cu = (uint64_t)(cus ? cus : 1) * GRIND_BLOCKS_PER_CU;
    const uint64_t cap = by_cu < GRIND_BLOCKS_MAX ? by_cu : GRIND_BLOCKS_MAX;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > cap ? cap : want));
    const unsigned per_proof = blocks / B ? blocks / B : 1;
    const int cl = (int)grind - 2 - (int)grind_ceil_log2(per_proof);
    const unsigned chunk_log = cl < (int)GRIND_PLAN_CHUNK_LOG_MIN   ? GRIND_PLAN_CHUNK_LOG_MIN
                               : cl > (int)GRIND_PLAN_CHUNK_LOG_MAX ? GRIND_PLAN_CHUNK_LOG_MAX
                                                                    : (unsigned)cl;
    return GrindPlan{chunk_log, blocks, grind_block_size(chunk_log), grind_max_nonce(grind)};
}

}  // namespace xfg
