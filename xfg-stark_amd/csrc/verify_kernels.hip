// Batched verification on the GPU (gfx950): the Merkle openings and the per-query DEEP / FRI /
// remainder checks of many burn proofs at once. The host replays each transcript and lays the work
// out as flat task lists (verifier.cpp plan_proof); see xfg_verify_batch_gpu in verify_batch_gpu.hip.
// Replaces the serial BatchBurnMintVerifier loops of the reference (src/burn_mint_verifier.rs:
// 326-338, 386-408), each of which runs winterfell::verify on the CPU.
#include "dispatch.hpp"
#include "hip_util.hpp"
#include "verifier.hpp"

namespace xfg {

// exclusive prefix count of `f` over the workgroup's 256 threads (4 waves), and the total
__device__ __forceinline__ int block_scan(bool f, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ULL << lane) - 1));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        base += k < w ? wsum[k] : 0;
        total += wsum[k];
    }
    __syncthreads();
    return base + pre;
}

// One batch Merkle opening per workgroup: BatchMerkleProof::get_root (winter-crypto 0.8.3, the
// opening plan_batch_opening emits) recomputed in place. Thread i hashes opened row i (rows sorted
// by leaf index); the distinct leaf pairs take their missing leaf from node vector j (j = the pair's
// position); then, level by level, the entry at position j of the current sorted list merges with
// its right neighbour when that is its sibling, else takes its sibling from vector j; the survivors
// are compacted (block scan) and climb one level. The opening is valid when every vector holds the
// nodes the walk takes (nodes past them are ignored, as winter-crypto 0.8's get_root ignores them:
// verifier.cpp tree_ok, the same walk done serially by the host) and the root equals the commitment;
// else flags[proof] |= bit.
__global__ __launch_bounds__(256) void vtree_kernel(const uint8_t* blob, const VTree* trees, const VTreeLeaf* tleaves,
                                                    const VVec* vecs, u64* flags) {
    __shared__ Digest leaf[512];
    __shared__ Digest dg[2][256];
    __shared__ u64 hx[2][256];
    __shared__ u64 sidx[256];
    __shared__ uint8_t have[512];
    __shared__ int wsum[4];
    __shared__ int bad;
    const VTree T = trees[blockIdx.x];
    const int i = threadIdx.x;
    const u64 L = 1ULL << T.depth;
    if (i == 0) bad = 0;
    // the vector this thread's position consumes from, and how many nodes it has taken
    VVec vec{0, 0, 0};
    if (i < (int)T.nvec) vec = vecs[T.vec0 + i];
    uint32_t used = 0;
    auto take = [&](Digest& out) {
        if (used >= vec.cnt) {
            bad = 1;
            out = Digest{};
            return;
        }
        out = ld_digest(blob + vec.off + 32 * (u64)used);
        used++;
    };
    u64 idx = 0;
    Digest ld{};
    const bool opened = i < (int)T.nidx;
    if (opened) {
        const VTreeLeaf lf = tleaves[T.leaf0 + i];
        idx = lf.index;
        ld = hash_row(blob + lf.row_off, T.words);
        sidx[i] = idx;
    }
    have[i] = 0;
    have[i + 256] = 0;
    __syncthreads();
    // leaf pairs: thread i's pair position = number of pair starts before it (minus one if it is the
    // right leaf of a pair whose left leaf is opened too)
    const bool start = opened && (i == 0 || (sidx[i - 1] >> 1) != (idx >> 1));
    int npairs;
    const int pp = block_scan(start, wsum, npairs) - (opened && !start ? 1 : 0);
    if (opened) {
        leaf[2 * pp + (idx & 1)] = ld;
        have[2 * pp + (idx & 1)] = 1;
        if (start) hx[0][pp] = (L + (idx & ~1ULL)) >> 1;
    }
    if (i == 0 && (int)T.nvec != npairs) bad = 1;
    __syncthreads();
    if (i < npairs) {
        Digest l = leaf[2 * i], r = leaf[2 * i + 1];
        if (!have[2 * i]) take(l);
        if (!have[2 * i + 1]) take(r);
        dg[0][i] = b3_merge(l, r);
    }
    __syncthreads();
    int nn = npairs, cb = 0;
    for (unsigned lvl = 1; lvl < T.depth; lvl++) {
        const bool act = i < nn;
        const u64 h = act ? hx[cb][i] : 0;
        const bool left = act && !(h & 1) && i + 1 < nn && hx[cb][i + 1] == h + 1;
        const bool right = act && (h & 1) && i > 0 && hx[cb][i - 1] == h - 1;
        Digest par{};
        if (act && !right) {  // one merge call site: (own, right neighbour) or (own, vector node) in order
            Digest x = dg[cb][i], y;
            if (left) {
                y = dg[cb][i + 1];
            } else {
                take(y);
                if (h & 1) {
                    const Digest t = x;
                    x = y;
                    y = t;
                }
            }
            par = b3_merge(x, y);
        }
        int total;
        const int m = block_scan(act && !right, wsum, total);
        if (act && !right) {
            hx[cb ^ 1][m] = h >> 1;
            dg[cb ^ 1][m] = par;
        }
        __syncthreads();
        nn = total;
        cb ^= 1;
    }
    __syncthreads();
    if (i == 0) {
        const Digest root = ld_digest(blob + T.root_off);
        bool ok = !bad && nn == 1 && hx[cb][0] == 1;
        for (int w = 0; w < 8; w++) ok = ok && dg[cb][0].w[w] == root.w[w];
        if (!ok) atomicOr((unsigned long long*)&flags[T.proof], (unsigned long long)T.bit);
    }
}

// one thread per (proof, query): query_bits (verify_checks.hpp), its failures set in flags[proof].
// F = 2^LOGF: the folding factor of every proof that has a record in fq[0 .. nq), one of the batch's four
// ranges (launch_verify); Q.proof indexes the whole batch's fp and flags
template <int LOGF>
__global__ __launch_bounds__(64) void vfield_kernel(const uint8_t* blob, const VFieldProof* fp, const VFieldQuery* fq,
                                                    u64 nq, u64* flags) {
    const u64 qi = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const VFieldQuery& Q = fq[qi];
    const u64 bad = query_bits<LOGF>(blob, fp[Q.proof], Q);
    if (bad) atomicOr((unsigned long long*)&flags[Q.proof], (unsigned long long)bad);
}

static unsigned blocks_for(u64 n, unsigned t) { return (unsigned)((n + t - 1) / t); }

void launch_verify(const uint8_t* blob, const VTree* trees, u64 ntrees, const VTreeLeaf* tleaves, const VVec* vecs,
                   const VFieldProof* fp, const VFieldQuery* fq, const FoldRanges& ranges, u64* flags, hipStream_t s) {
    if (ntrees) XFG_LAUNCH(vtree_kernel, dim3((unsigned)ntrees), dim3(256), 0, s, blob, trees, tleaves, vecs, flags);
    for (int r = 0; r < 4; r++) {  // folding factor 2 << r: its instantiation over its own range of records
        const u64 first = ranges.begin[r], nq = ranges.begin[r + 1] - first;
        if (!nq) continue;  // a zero-sized grid is a launch error
        const dim3 g(blocks_for(nq, 64)), b(64);
        with_fold(2 << r, [&](auto LOGF) { XFG_LAUNCH(vfield_kernel<LOGF>, g, b, 0, s, blob, fp, fq + first, nq, flags); });
    }
}

}  // namespace xfg
