// Merkle commitments (RowMatrix::commit_to_rows / MerkleTree::new, FriProver's layer commitments) for
// gfx950: the leaf kernels, the tree levels above them, the transcript step on the root and the
// recomputation of opened rows.
//
// Heap layout per tree: nodes[1] = root, nodes[i] = H(nodes[2i] || nodes[2i+1]), leaf k at L + k
// (MerkleTree::new / build_merkle_nodes, winter-crypto 0.8.3). For the LDE commitments only the
// levels >= log2(beta) + 1 are stored (heap [1, n)): the 2^log2(beta) leaves of LDE row m (one per
// coset, coset-major layout; beta = 2 .. 128) form a register-resident subtree whose top is heap node n + m. The
// few leaves / low nodes a proof opens are recomputed from the LDE by open_rows_kernel. A tree of
// L leaf slots lives in 2 L digests (node stride 2n for an LDE, 2 rows for a FRI layer).
//
// A commitment is a leaf kernel, which also merges each block's nodes a few levels up through LDS,
// then tree_mid / tree_mid4 launches while more than TREE_TOP_MAX nodes are left, then one
// tree_top block per tree. The route, all of it in launch_merkle_lde / launch_merkle_fri / finish_tree:
//   LDE leaves   n >= ROW2_MIN_N and npoly n / 256 < ROW2_MAX_BLOCKS: leaves_row2_kernel, else leaves_row_kernel
//   middle       (count / 512) npoly < MID4_MAX_BLOCKS: tree_mid4_kernel, else tree_mid_kernel
#include "dev_coin.hpp"
#include "dispatch.hpp"
#include "hip_util.hpp"
#include <algorithm>
#include <stdexcept>
#include <type_traits>

namespace xfg {

// ---- routing thresholds
// leaves_row2_kernel (LEAF_LANES lanes per row) serves small launch sets, under one wave per SIMD of
// one-lane-per-row blocks (a lone proof), of trees with at least four whole blocks of rows
constexpr u64 ROW2_MIN_N = 1024, ROW2_MAX_BLOCKS = 1024;
constexpr int LEAF_LANES_LOG = 1;  // 2 lanes per row (4: 42.5 + 40.4 against 31.8 + 27.9 µs, profiles/r06/leaves_small_ab.txt)
// in-block Merkle levels continue while a level keeps >= 64 nodes per block (full waves only); the
// narrower levels go to the kernels above
constexpr int UP_WMIN = 64;
// tree_mid_kernel: 512 nodes in, 64 out per block. (Merging on down to one node per block ran six more
// levels on one part-filled wave each: 13 wave-compressions per block for the work of 8.)
constexpr int TREE_MID_WMIN = 64, TREE_MID_SHRINK = 8;
// tree_mid4_kernel (four lanes per parent) instead, for launch sets under one block per CU
constexpr u64 MID4_MAX_BLOCKS = 256;
// tree_top_kernel takes the last levels from here: 512 nodes = 256 parents of four lanes = 1024 threads
constexpr u64 TREE_TOP_MAX = 512;

// ============================================================================ level helpers
// One Merkle level through LDS: the threads with `have` hold node `slot` of the block's part of a
// level in d; after the barrier thread t < half merges nodes 2t, 2t + 1, keeps the parent in d and
// stores it to dst[t]. The caller places the barrier that frees the LDS for the next level.
__device__ __forceinline__ void lds_level(Digest& d, bool have, int slot, Digest* lds, int half, Digest* dst) {
    const int t = threadIdx.x;
    if (have) lds[slot] = d;
    __syncthreads();
    if (t < half) {
        d = b3_merge(lds[2 * t], lds[2 * t + 1]);
        dst[t] = d;
    }
}
// Block-level continuation of a Merkle level: thread t of a block of T (power of two) threads
// holds the digest of node blockIdx.x * T + t of the level with `count` nodes (heap [count,
// 2 count)). The block merges its T nodes up through LDS, storing every parent, until a level has
// `wmin` nodes per block (lanes of narrower levels would idle): count / T * wmin nodes are left.
__device__ __forceinline__ void block_tree_up(Digest d, Digest* nodes, u64 count, Digest* lds, int wmin) {
    u64 c = count;
    for (int w = blockDim.x; w > wmin; w >>= 1) {
        c >>= 1;
        lds_level(d, true, threadIdx.x, lds, w / 2, nodes + c + (u64)blockIdx.x * (w / 2));
        __syncthreads();
    }
}
// One level at four lanes per parent (b3_merge_quad): quad i of the active ones (whole quads) merges
// src[2i], src[2i + 1] and writes the parent, two words per lane, to lds[i] and dst[i]. src may be the
// LDS of the previous level: every quad has read it before the first barrier.
__device__ __forceinline__ void quad_level(const Digest* src, bool act, int i, int q, Digest* lds, Digest* dst) {
    uint2 o = make_uint2(0, 0);
    if (act) {
        uint32_t m[16];
#pragma unroll
        for (int w = 0; w < 8; w++) {
            m[w] = src[2 * i].w[w];
            m[8 + w] = src[2 * i + 1].w[w];
        }
        o = b3_merge_quad(m, q);
    }
    __syncthreads();
    if (act) {
        lds[i].w[q] = o.x;
        lds[i].w[4 + q] = o.y;
        dst[i].w[q] = o.x;
        dst[i].w[4 + q] = o.y;
    }
    __syncthreads();
}

// ============================================================================ LDE leaves
// One leaf's elements: row[c] = column c of the LDE at coset t, row m. CC (a trace LDE with constant
// columns, NC = 7; columns.hpp ColConst): a column flagged in rc comes from rc and its load is not
// issued; a column shared in rc is read at the same place of proof 0's planes, `back` words before the
// proof's own (one offset, selected per column: wave-uniform where a block serves one proof, per lane in
// the openings). CC = false is the dense read and takes no RowConst (NoConst)
struct NoConst {};
struct RowConstBack : RowConst {
    u64 back;  // words from proof 0's planes to the proof's own: proof * 7 * beta * n
    // the leaf kernels (a block per proof): what the constant columns fix of round 1 of every leaf's hash
    // (blake3.hpp b3_row7_prefix), in scalar registers; pre.ugs = 0 (nothing to resume from) elsewhere
    B3RowPrefix pre;
};
// The blowups whose leaf kernels resume their leaves from the prefix: all but 64. There the two-lane kernel
// goes from 93 to 98 vector registers with it and loses a wave (profiles/r16/kernel_resources.txt), so both
// kernels of that blowup keep the whole hash; 32 and 128 take three registers more and keep their waves.
template <int LOGB>
constexpr bool leaf_prefix_on() { return LOGB != 6; }
template <bool CC>
using RowConstOf = std::conditional_t<CC, RowConstBack, NoConst>;
template <int NC, int LOGB, bool CC>
__device__ __forceinline__ void lde_row(const u64* base, u64 n, u64 m, int t, const RowConstOf<CC>& rc, u64 (&row)[NC]) {
    static_assert(!CC || NC == 7, "constant columns are those of the trace");
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if constexpr (CC) {
            if ((rc.mask >> c) & 1) {
                row[c] = rc.v[c];
                continue;
            }
            row[c] = (base - ((rc.shared >> c) & 1 ? rc.back : 0))[((u64)c * (1 << LOGB) + t) * n + m];
        } else {
            row[c] = base[((u64)c * (1 << LOGB) + t) * n + m];
        }
    }
}

// subtree over the leaves t = T0 .. T0 + 2^LOG - 1 of LDE row m; compile-time recursion keeps
// every intermediate digest in registers.
template <int NC, int LOGB, int LOG, int T0, bool CC>
__device__ __forceinline__ Digest lde_subtree(const u64* base, u64 n, u64 m, const RowConstOf<CC>& rc) {
    if constexpr (LOG == 0) {
        u64 row[NC];
        lde_row<NC, LOGB, CC>(base, n, m, T0, rc, row);
        if constexpr (CC && leaf_prefix_on<LOGB>()) {
            if (rc.pre.ugs) return b3_hash_row7(rc.pre, row);  // wave-uniform; nothing to resume from: the whole hash
        }
        return b3_hash_elems<NC>(row);
    } else {
        Digest l = lde_subtree<NC, LOGB, LOG - 1, T0, CC>(base, n, m, rc);
        Digest r = lde_subtree<NC, LOGB, LOG - 1, T0 + (1 << (LOG - 1)), CC>(base, n, m, rc);
        return b3_merge(l, r);
    }
}

// The same subtree for 2^LOG > 16 leaves (blowup 32, 64, 128), leaves t0 .. t0 + 2^LOG - 1: the levels above
// the 16-leaf subtrees are two-trip loops that stay rolled, one inside the other, so the code is that of one
// unrolled 16-leaf subtree and a thread holds one pending digest per level (unrolled through all seven
// levels the three column counts took minutes to compile). Up to 16 leaves this is lde_subtree itself.
template <int NC, int LOGB, int LOG, bool CC>
__device__ __forceinline__ Digest lde_subtree_wide(const u64* base, u64 n, u64 m, int t0, const RowConstOf<CC>& rc) {
    if constexpr (LOG <= 4) {
        return lde_subtree<NC, LOGB, LOG, 0, CC>(base + (u64)t0 * n, n, m, rc);
    } else {
        Digest l, d;
#pragma unroll 1
        for (int i = 0; i < 2; i++) {
            d = lde_subtree_wide<NC, LOGB, LOG - 1, CC>(base, n, m, t0 + (i << (LOG - 1)), rc);
            if (i == 0) l = d;
        }
        return b3_merge(l, d);
    }
}

// the constant columns of a block's proof (a block per proof: flags and values are read once, wave-uniform)
// back: the words between proof 0's planes and this proof's (RowConstBack)
// PREFIX: with the uniform part of the leaf hash's round 1, computed here once for the thread's whole subtree
// on the wave-uniform values (every word made a scalar)
template <bool CC, bool PREFIX>
__device__ __forceinline__ RowConstOf<CC> block_row_const(const ColConst& cc, int proof, u64 back) {
    if constexpr (CC) {
        RowConstBack rc;
        static_cast<RowConst&>(rc) = row_const_uniform(cc, (u64)proof);
        rc.back = back;
        rc.pre.ugs = 0;
        if constexpr (PREFIX) {
            rc.pre = b3_row7_prefix(rc.v, rc.mask);
#pragma unroll
            for (int w = 0; w < 16; w++) rc.pre.s[w] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rc.pre.s[w]);
            rc.pre.ugs = (unsigned)__builtin_amdgcn_readfirstlane((int)rc.pre.ugs);
        }
        return rc;
    } else {
        return NoConst{};
    }
}

// one LDE row per thread, min(256, n) rows per block: the row's 2^LOGB-leaf subtree (top at heap level
// log2(beta), not stored), then through LDS the row-pair level (heap n/2 + m/2) and one more (n/4 + m/4):
// 256 rows -> 64 nodes per block, n/4 left for the levels above. Against two rows per thread (the
// kernel this one replaced) a thread holds one row and one pending digest per subtree level -- 49-56
// instead of 83-105 VGPRs, 8 instead of 4-5 waves per SIMD -- for the same compressions: the trace
// leaves 3.3 % faster, the composition leaves unchanged (profiles/r05/leaves_row.txt).
// CC: the constant columns of the block's proof stand in for their planes; cc is unused without it
template <int NC, int LOGB, bool CC>
__global__ __launch_bounds__(256) void leaves_row_kernel(const u64* lde, Digest* nodes_all,
                                                         u64 node_stride, int logn, ColConst cc) {
    __shared__ Digest lds[256];
    const u64 n = 1ULL << logn;
    const int proof = blockIdx.y;
    const u64 m = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // grid covers n exactly
    const u64 back = (u64)proof * NC * (1 << LOGB) * n;
    const u64* base = lde + back;
    const RowConstOf<CC> rc = block_row_const<CC, leaf_prefix_on<LOGB>()>(cc, proof, back);
    Digest d = lde_subtree_wide<NC, LOGB, LOGB, CC>(base, n, m, 0, rc);
    block_tree_up(d, nodes_all + (u64)proof * node_stride, n, lds, blockDim.x / 4);
}

// The same levels for small launch sets (a lone proof: one wave per SIMD, each running the row's
// 2 beta - 1 compressions in sequence): 2^LOGL lanes per row, each the subtree of beta / 2^LOGL cosets,
// merged across the lane group (__shfl_xor, every lane of the group merging at every level), then the
// row-pair level and one more through LDS: 256 / 2^LOGL rows -> a quarter as many nodes per block.
// 2^LOGL times the waves, and a chain of beta / 2^LOGL + log2 beta + 2 compressions instead of 2 beta + 1.
template <int LOGB>
constexpr int leaf_lanes_log() { return LOGB < LEAF_LANES_LOG ? LOGB : LEAF_LANES_LOG; }
template <int NC, int LOGB, bool CC>
__global__ __launch_bounds__(256) void leaves_row2_kernel(const u64* lde, Digest* nodes_all,
                                                          u64 node_stride, int logn, ColConst cc) {
    constexpr int LOGL = leaf_lanes_log<LOGB>(), RB = 256 >> LOGL;  // lanes per row (log2), rows per block
    __shared__ Digest lds[RB];
    const u64 n = 1ULL << logn;
    const int proof = blockIdx.y, t = threadIdx.x, h = t & ((1 << LOGL) - 1), rl = t >> LOGL;
    const u64 m = (u64)blockIdx.x * RB + rl;
    const u64 back = (u64)proof * NC * (1 << LOGB) * n;
    const u64* base = lde + back + (u64)h * (1 << (LOGB - LOGL)) * n;
    const RowConstOf<CC> rc = block_row_const<CC, leaf_prefix_on<LOGB>()>(cc, proof, back);
    Digest d = lde_subtree_wide<NC, LOGB, LOGB - LOGL, CC>(base, n, m, 0, rc);
#pragma unroll
    for (int k = 0; k < LOGL; k++) {
        Digest r;
#pragma unroll
        for (int w = 0; w < 8; w++) r.w[w] = __shfl_xor(d.w[w], 1 << k);
        d = (h >> k) & 1 ? b3_merge(r, d) : b3_merge(d, r);
    }
    Digest* nodes = nodes_all + (u64)proof * node_stride;
    lds_level(d, h == 0, rl, lds, RB / 2, nodes + n / 2 + (u64)blockIdx.x * (RB / 2));
    __syncthreads();
    lds_level(d, t < RB / 2, t, lds, RB / 4, nodes + n / 4 + (u64)blockIdx.x * (RB / 4));
}

// openings: recompute the local subtree heaps of selected rows; entry e = proof << logn | m. One
// lane per leaf (coset t of row m, 2^LOGB lanes per entry inside a wave): the leaf, then LOGB
// merge levels with the right child taken from lane l ^ 2^(k-1) -- 1 + LOGB dependent compressions
// per entry instead of the 2^(LOGB+1) - 1 one lane ran in sequence (a lone proof waits on them).
// Every lane of a group merges at every level (no divergence around the shuffles); the lanes with
// t % 2^k == 0 hold level k's nodes and store them to the local heap (slot 1 = top).
// Blowup 128 has more leaves per row than a wave has lanes: there a lane takes the two leaves 2l, 2l + 1
// and their parent (2^LPL leaves per lane, 2^LOGL = 64 lanes per entry), and the shuffles start one level up.
// CC: the constant columns of the entry's proof (which differs from lane group to lane group) stand in
// for their planes
template <int LOGB>
constexpr int open_lanes_log() { return LOGB < 6 ? LOGB : 6; }
template <int NC, int LOGB, bool CC>
__global__ __launch_bounds__(64) void open_rows_kernel(const u64* lde, const u64* entries, u64 count, Digest* out,
                                                       int logn, ColConst cc) {
    constexpr int LOGL = open_lanes_log<LOGB>(), LPL = LOGB - LOGL;
    static_assert(LPL <= 1, "at most two leaves per lane");
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 e = g >> LOGL;
    const int t = (int)(g & ((1 << LOGL) - 1)) << LPL;  // the lane's (first) leaf
    if (e >= count) return;  // whole groups: count is per entry, groups never straddle a wave
    const u64 n = 1ULL << logn, ent = entries[e];
    const u64 proof = ent >> logn, m = ent & (n - 1);
    const u64* base = lde + proof * NC * (1 << LOGB) * n;
    Digest* local = out + e * (2 << LOGB);
    RowConstOf<CC> rc;
    if constexpr (CC) {
        static_cast<RowConst&>(rc) = row_const_lane(cc, proof);
        rc.back = proof * NC * (1 << LOGB) * n;
        rc.pre.ugs = 0;
    }
    u64 row[NC];
    lde_row<NC, LOGB, CC>(base, n, m, t, rc, row);
    Digest d = b3_hash_elems<NC>(row);
    local[(1 << LOGB) + t] = d;
    if constexpr (LPL == 1) {
        lde_row<NC, LOGB, CC>(base, n, m, t + 1, rc, row);
        const Digest d1 = b3_hash_elems<NC>(row);
        local[(1 << LOGB) + t + 1] = d1;
        d = b3_merge(d, d1);
        local[((1 << LOGB) + t) >> 1] = d;
    }
#pragma unroll
    for (int k = LPL + 1; k <= LOGB; k++) {
        Digest r;
#pragma unroll
        for (int w = 0; w < 8; w++) r.w[w] = __shfl_xor(d.w[w], 1 << (k - 1 - LPL));
        d = b3_merge(d, r);
        if ((t & ((1 << k) - 1)) == 0) local[((1 << LOGB) + t) >> k] = d;
    }
}

// The one dispatch of the three kernel families above: f(NC, LOGB, CC) as integral constants
// (dispatch.hpp), for nc in {7, 2, 1} and blowup 2..128; with constant columns the CC instantiations,
// which exist for the seven trace columns alone. Anything else has no kernel: refused, never skipped
// (the ABI entries validate both before anything is launched).
template <class F>
static void with_lde_kernel(int nc, int logbeta, const ColConst& cc, F f) {
    if (cc.flags && nc != 7) throw std::invalid_argument("Merkle kernels: constant columns are those of a 7-column trace LDE");
    if (cc.flags) with_logbeta<7>(logbeta, [&](auto NC, auto LB) { f(NC, LB, std::true_type{}); });
    else with_nc_logbeta(nc, logbeta, [&](auto NC, auto LB) { f(NC, LB, std::false_type{}); });
}

void launch_open_rows(const u64* lde, int nc, const u64* entries, u64 count, Digest* out, int logn, int logbeta,
                      hipStream_t s, const ColConst& cc) {
    if (!count) return;
    const int logl = logbeta < 6 ? logbeta : 6;  // lanes per entry (open_lanes_log)
    dim3 g((unsigned)(((count << logl) + 63) / 64)), b(64);
    with_lde_kernel(nc, logbeta, cc, [&](auto NC, auto LB, auto CC) {
        XFG_LAUNCH((open_rows_kernel<NC, LB, CC>), g, b, 0, s, lde, entries, count, out, logn, cc);
    });
}

// ============================================================================ transcript step
// one wave (all lanes, uniform) of the block that computed proof b's root: reseed with the root,
// then the draws that follow that commitment in Prover::prove
__device__ void coin_root_step(const CoinStep& cs, int b, const Digest& root) {
    const int D = cs.ext, lane = threadIdx.x;
    DevCoin c = cs.coins[b];
    dev_reseed(c, root);
    bool ok;
    if (cs.kind == CoinStep::COEFFS) {  // 7 transition + 8 boundary composition coefficients
        ok = wave_draw_e(c, 15, D, cs.out + (u64)b * 15 * D, D);
    } else {
        u64 a[2] = {0, 0};
        ok = dev_draw_e(c, a, D);
        if (cs.kind == CoinStep::OOD_POINT) {  // z, and z g; z = 0 leaves no DEEP quotient
            if (a[0] == 0 && a[1] == 0) ok = false;
            if (lane == 0)
                for (int k = 0; k < D; k++) {
                    cs.out[(u64)b * 2 * D + k] = a[k];
                    cs.out[(u64)b * 2 * D + D + k] = gl_mul(a[k], cs.g);
                }
        } else if (lane == 0) {  // FRI layer alpha, stored as alpha * 7^-1 for the fold
            const u64 inv7 = 0x249249246DB6DB6EULL;
            for (int k = 0; k < D; k++) cs.out[(u64)b * D + k] = gl_mul(a[k], inv7);
            if (cs.hist)
                for (int k = 0; k < D; k++) cs.hist[(u64)b * D + k] = a[k];
        }
    }
    if (lane == 0) {
        if (!ok) cs.fail[b] = 1;
        cs.coins[b] = c;
        if (cs.root_out) cs.root_out[b] = root;
    }
}

// ============================================================================ levels above the leaf kernel
// last levels (count <= TREE_TOP_MAX): one block per tree, four lanes per node, the levels
// through LDS; then the transcript step `cs` on the root
__global__ __launch_bounds__(1024) void tree_top_kernel(Digest* nodes_all, u64 node_stride, u64 count, CoinStep cs) {
    __shared__ Digest lds[256];
    Digest* nodes = nodes_all + (u64)blockIdx.x * node_stride;
    const int tid = threadIdx.x, i = tid >> 2, q = tid & 3;
    for (u64 c = count; c > 1; c >>= 1) {
        const u64 half = c >> 1;
        quad_level(c == count ? nodes + c : lds, i < (int)half, i, q, lds, nodes + half);
    }
    if (cs.kind != CoinStep::NONE && tid < 64) coin_root_step(cs, blockIdx.x, count > 1 ? lds[0] : nodes[1]);
}
// middle levels: a block merges 512 consecutive nodes of level `count` (two per thread, coalesced)
// and continues through LDS while a level keeps full waves, writing every parent: 64 nodes per block,
// count / TREE_MID_SHRINK remain.
__global__ __launch_bounds__(256) void tree_mid_kernel(Digest* nodes_all, u64 node_stride, u64 count) {
    __shared__ Digest lds[256];
    Digest* nodes = nodes_all + (u64)blockIdx.y * node_stride;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    const Digest d = b3_merge(nodes[count + 2 * i], nodes[count + 2 * i + 1]);
    nodes[count / 2 + i] = d;
    block_tree_up(d, nodes, count / 2, lds, TREE_MID_WMIN);
}
// the same three levels for small launch sets (under one block per CU: a lone proof's trees), four lanes
// per parent (b3_merge_quad): 128 nodes in, 16 out per block, each level's latency about half
__global__ __launch_bounds__(256) void tree_mid4_kernel(Digest* nodes_all, u64 node_stride, u64 count) {
    __shared__ Digest lds[64];
    Digest* nodes = nodes_all + (u64)blockIdx.y * node_stride;
    const int tid = threadIdx.x, i = tid >> 2, q = tid & 3;
    u64 c = count, first = (u64)blockIdx.x * 64;  // level being merged; this block's first parent in it
    for (int w = 64; w >= 16; w >>= 1, c >>= 1, first >>= 1)
        quad_level(w == 64 ? nodes + c + 2 * first : lds, i < w, i, q, lds, nodes + c / 2 + first);
}
// completes the tree above level `count` (nodes [count, 2 count) present) up to the root, then runs
// the transcript step `cs` on it
static void finish_tree(Digest* nodes, u64 node_stride, u64 count, int npoly, hipStream_t s, const CoinStep& cs) {
    while (count > TREE_TOP_MAX) {
        if ((count / 512) * (u64)npoly < MID4_MAX_BLOCKS)
            XFG_LAUNCH(tree_mid4_kernel, dim3((unsigned)(count / 128), npoly), dim3(256), 0, s, nodes, node_stride, count);
        else
            XFG_LAUNCH(tree_mid_kernel, dim3((unsigned)(count / 512), npoly), dim3(256), 0, s, nodes, node_stride, count);
        count /= TREE_MID_SHRINK;
    }
    if (count > 1 || cs.kind != CoinStep::NONE) {
        int threads = (int)(2 * count);  // four lanes per node of the widest level
        threads = threads < 64 ? 64 : threads;
        XFG_LAUNCH(tree_top_kernel, dim3(npoly), dim3(threads), 0, s, nodes, node_stride, count, cs);
    }
}

void launch_merkle_lde(const u64* lde, int nc, Digest* nodes, int npoly, int logn, int logbeta, hipStream_t s,
                       const CoinStep& cs, const ColConst& cc) {
    const u64 n = 1ULL << logn, node_stride = 2 * n;
    const bool row2 = n >= ROW2_MIN_N && (u64)npoly * (n / 256) < ROW2_MAX_BLOCKS;  // under one wave per SIMD
    const int logl = logbeta < LEAF_LANES_LOG ? logbeta : LEAF_LANES_LOG;
    const unsigned T = (unsigned)std::min<u64>(256, n);
    const dim3 g(row2 ? (unsigned)(n >> (8 - logl)) : (unsigned)(n / T), npoly), b(row2 ? 256 : T);
    with_lde_kernel(nc, logbeta, cc, [&](auto NC, auto LB, auto CC) {
        if (row2) XFG_LAUNCH((leaves_row2_kernel<NC, LB, CC>), g, b, 0, s, lde, nodes, node_stride, logn, cc);
        else XFG_LAUNCH((leaves_row_kernel<NC, LB, CC>), g, b, 0, s, lde, nodes, node_stride, logn, cc);
    });
    finish_tree(nodes, node_stride, n / 4, npoly, s, cs);  // both leaf kernels: the row level and two more
}

// FRI layer leaves (hash_values::<H, E, F> over transpose_slice rows, F = 2^LOGF the folding factor):
// leaf i = H(values at natural indices i + k*rows, k < F), 16 to 256 bytes. All leaves are stored
// (layers are N/F and smaller).
// E-valued layers are D coordinate planes `comp_stride` elements apart (per proof: D planes)
template <int D, int LOGF>
__global__ __launch_bounds__(256) void fri_leaves_kernel(const u64* vals, u64 val_stride, u64 comp_stride,
                                                         int coset_major, int logn, int logbeta, u64 rows,
                                                         Digest* nodes_all, u64 node_stride, int wmin) {
    __shared__ Digest lds[256];
    constexpr int NF = 1 << LOGF;
    const int proof = blockIdx.y;
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // grid covers rows exactly
    const u64* base = vals + (u64)proof * val_stride;
    u64 v[NF * D];
#pragma unroll
    for (int k = 0; k < NF; k++)
#pragma unroll
        for (int c = 0; c < D; c++)
            v[k * D + c] = layer_at(base + c * comp_stride, coset_major, logn, logbeta, i + (u64)k * rows);
    Digest d = b3_hash_elems<NF * D>(v);
    Digest* nodes = nodes_all + (u64)proof * node_stride;
    nodes[rows + i] = d;
    block_tree_up(d, nodes, rows, lds, wmin);
}
void launch_merkle_fri(const u64* vals, u64 val_stride, u64 comp_stride, bool coset_major, int logn, int logbeta,
                       u64 rows, Digest* nodes, int npoly, int ext, int fold, hipStream_t s, const CoinStep& cs) {
    const u64 T = std::min<u64>(256, rows), node_stride = 2 * rows;
    const int wmin = (int)std::min<u64>(T, UP_WMIN);
    dim3 g((unsigned)(rows / T), npoly);
    with_ext(ext, [&](auto D) {  // ext in {1, 2}, fold in {2, 4, 8, 16}: anything else is refused
        with_fold(fold, [&](auto LOGF) {
            XFG_LAUNCH((fri_leaves_kernel<D, LOGF>), g, dim3((unsigned)T), 0, s, vals, val_stride, comp_stride,
                       coset_major ? 1 : 0, logn, logbeta, rows, nodes, node_stride, wmin);
        });
    });
    finish_tree(nodes, node_stride, rows / T * wmin, npoly, s, cs);
}

}  // namespace xfg
