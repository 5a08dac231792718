// The proof-of-work search of the prover on the device: for each of B transcript seeds the smallest
// nonce whose BLAKE3(seed || nonce_le8) has `grind` trailing zero bits in its first 8 LE bytes (what
// plan_queries' host loop finds one hash at a time). Geometry and chunking: grind_plan.hpp.
#include "dev_coin.hpp"
#include "grind_plan.hpp"
#include "hip_util.hpp"
#include "kernels.hpp"

namespace xfg {

constexpr u64 GRIND_NONE = ~0ULL;  // `best` of a proof without a hit yet; no chunk / no hit in a block

struct GrindArgs {
    const Digest* seeds;  // [B]
    u64* best;            // [B], preset to GRIND_NONE
    u64* next_chunk;      // [B], preset to 0
    u64 first, max_nonce;
    unsigned B, grind, chunk_log;
};

__device__ __forceinline__ u64 grind_load(const u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane tests one nonce per compression (dev_merge_int); a block works on one proof at a time, chunk
// by chunk, and moves to the next proof when its current one is finished. Blocks never wait for each
// other: every word they share (next_chunk, best) is only touched by atomics, and a stale `best` costs a
// scan, never an answer.
//
// Why best[b] ends as the smallest nonce >= first that passes (or stays GRIND_NONE when none <= max_nonce does):
//  - chunks of a proof are claimed in increasing order (atomicAdd on next_chunk[b]), each by one block;
//  - a claimed chunk is either scanned completely, or skipped / left early because best[b] was seen below the
//    nonces still to test in it. Within a chunk a wave tests its nonces in increasing order and stops at its
//    first hit, the block's minimum over the waves goes into best[b] by one atomicMin;
//  - best[b] only decreases, so whatever was seen below a nonce stays below it;
//  - a block stops claiming for a proof only when next_chunk[b] is past the last chunk or best[b] is below
//    the next chunk to claim; both stay true for every later chunk.
//  So every nonce below the final best[b] lies in a chunk that was claimed, was not skipped over (that
//  would need a best[b] below it), and therefore was tested and failed; and the kernel ends only when every
//  claimed chunk has been dealt with, since each block finishes its own. Termination: every pass of the
//  outer loop either consumes one of finitely many chunks or counts one finished proof, and B finished
//  proofs in a row end the block.
__global__ __launch_bounds__(GRIND_BLOCK) void grind_kernel(GrindArgs a) {
    __shared__ u64 sh_chunk;
    __shared__ u64 sh_min[GRIND_BLOCK / 64];
    const unsigned tid = threadIdx.x, nth = blockDim.x;
    const u64 nchunks = grind_chunk_count(a.first, a.max_nonce, a.chunk_log);
    const uint32_t mask = a.grind >= 32 ? 0xFFFFFFFFu : (1u << a.grind) - 1u;  // tz64(w0 | w1 << 32) >= grind, grind <= 32
    unsigned b = blockIdx.x % a.B;
    for (unsigned finished = 0; finished < a.B;) {
        if (tid == 0) {
            u64 c = GRIND_NONE;
            // look before claiming: a finished proof's counter is not driven up by the blocks passing by
            const u64 seen = grind_load(&a.next_chunk[b]);
            if (seen < nchunks && grind_load(&a.best[b]) >= grind_chunk_first(a.first, seen, a.chunk_log)) {
                c = atomicAdd((unsigned long long*)&a.next_chunk[b], 1ULL);
                if (c >= nchunks || grind_load(&a.best[b]) < grind_chunk_first(a.first, c, a.chunk_log)) c = GRIND_NONE;
            }
            sh_chunk = c;
        }
        __syncthreads();
        const u64 c = sh_chunk;
        __syncthreads();  // sh_chunk is free for the next claim
        if (c == GRIND_NONE) {
            finished++;
            b = b + 1 == a.B ? 0 : b + 1;
            continue;
        }
        finished = 0;
        const u64 lo = grind_chunk_first(a.first, c, a.chunk_log);
        const u64 cnt = grind_chunk_last(a.first, a.max_nonce, c, a.chunk_log) - lo + 1;  // <= 2^chunk_log
        const Digest seed = a.seeds[b];
        u64 found = GRIND_NONE;
        for (u64 base = 0; base < cnt; base += nth) {
            // every fourth pass: has another block's hit made the rest of this chunk pointless?
            if (base && ((base / nth) & 3) == 0 && __ballot(grind_load(&a.best[b]) < lo + base)) break;
            const u64 off = base + tid;
            const Digest h = dev_merge_int(seed, lo + off);
            const u64 hits = __ballot(off < cnt && (h.w[0] & mask) == 0);
            if (hits) {  // lanes hold increasing nonces: the wave's first hit is its smallest
                found = lo + base + (tid & ~63u) + (unsigned)(__ffsll((unsigned long long)hits) - 1);
                break;
            }
        }
        if ((tid & 63) == 0) sh_min[tid >> 6] = found;
        __syncthreads();
        if (tid == 0) {
            u64 m = sh_min[0];
            for (unsigned w = 1; w < nth / 64; w++) m = sh_min[w] < m ? sh_min[w] : m;
            if (m != GRIND_NONE) atomicMin((unsigned long long*)&a.best[b], (unsigned long long)m);
        }
    }
}

// best [B] -> out [B] (device-mapped pinned host memory): the nonce, 0 where the range held none
__global__ void grind_collect_kernel(const u64* best, u64* out, unsigned B) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) out[i] = best[i] == GRIND_NONE ? 0 : best[i];
}

void launch_grind(const Digest* seeds, u64* state, u64* out, unsigned B, unsigned grind, u64 first, u64 max_nonce,
                  unsigned chunk_log, unsigned blocks, hipStream_t s) {
    const size_t words = grind_state_words(B) / 2;
    GrindArgs a{seeds, state, state + words, first, max_nonce, B, grind, chunk_log};
    HIPCHK(hipMemsetAsync(a.best, 0xFF, words * 8, s));
    HIPCHK(hipMemsetAsync(a.next_chunk, 0, words * 8, s));
    XFG_LAUNCH(grind_kernel, dim3(blocks), dim3(grind_block_size(chunk_log)), 0, s, a);
    XFG_LAUNCH(grind_collect_kernel, dim3((B + 255) / 256), dim3(256), 0, s, a.best, out, B);
}

}  // namespace xfg
