// Launch wrappers for the burn-proof STARK kernels (gfx950). Every wrapper enqueues on the given
// stream and never synchronises; batch dimension = number of independent proofs. A wrapper throws
// std::invalid_argument for an ext outside {1, 2}, a fold outside {2, 4, 8, 16} or an LDE shape without a kernel
// (dispatch.hpp), and HipError naming the kernel when the runtime refuses a launch (hip_util.hpp XFG_LAUNCH).
#pragma once
#include <hip/hip_runtime.h>
#include "gl.hpp"
#include "air.hpp"
#include "blake3.hpp"
#include "ntt_plan.hpp"
#include "trace_layout.hpp"
#include "burn_record.hpp"
#include "columns.hpp"

namespace xfg {

// per-proof DEEP parameters, every value an element of E (2 coordinates; the second is 0 without
// a field extension): trace coefficients a_i, composition coefficient, OOD points and the
// constant terms c1 = sum a_i T_i(z) + gamma H(z), c2 = sum a_i T_i(z g)
struct DeepParams {
    u64 a[7][2];
    u64 gamma[2];
    u64 z[2], zg[2], zinv[2], zginv[2];
    u64 c1[2], c2[2];
    u64 pad[2];
};

// precomputed four-step twiddles (tables.hip build_fourstep): fwd[logn][logbeta] holds
// 7^j2 w_N^(j2 (t + beta k1)) at [t][k1][j2], inv[logn] holds w_n^-(j2 k1) / n at [k1][j2];
// nullptr -> the kernels form them as running products. Which of the two a forward size gets:
// table_kind (ntt_plan.hpp).
// forward sizes past FOURSTEP_MAX_LOG (configs[4]: 2^20 x 16 = 2^24 points, where a full table would
// be 128 MB) get no beta n table, only the per-size pass tables as one contiguous block,
// pass_fwd[logn][logbeta]: w_R^i, w_C^i and the coset pre-factors (R + C + beta R entries); at
// R = C = 1024 also the per-coset [r][k] and [t][j2] factors and the coset-independent [k1][j2]
// four-step table (8 MiB, ntt_pass_a_r1024); other sizes keep running-product four-step twiddles
struct FourStep {
    const u64* fwd[FOURSTEP_MAX_LOG + 1][5] = {};
    const u64* inv[FOURSTEP_MAX_LOG + 1] = {};
    const u64* pass_fwd[PASS_MAX_LOG + 1][5] = {};
};
struct Tables {
    const u64* tw;     // tw[e] = w_{2^LM}^e, e < 2^LM
    int LM;
    const u64* pow7;   // 7^j,  j < 2^LM
    const u64* ipow7;  // 7^-j, j < 2^LM
    const FourStep* fs;  // host-side table registry (never dereferenced on the device)
};
// w_{2^k}^e from the master table, or its inverse
__device__ __forceinline__ u64 tw_get(const Tables& T, int k, u64 e, bool inv) {
    const u64 M = 1ULL << T.LM, idx = (e << (T.LM - k)) & (M - 1);
    return T.tw[inv ? (M - idx) & (M - 1) : idx];
}

// ---- NTT (four-step, natural order in/out) ----
// forward LDE: coef[poly][n] -> out[poly][beta][n] (coset-major: out[p][t][m] = P(7 w_N^(t + beta m)))
// skip [npoly] (device, or nullptr): polynomials with a non-zero byte are not transformed and their
// planes of out are left untouched (the consumers of a trace LDE take such a column from a ColConst;
// launch_const_fill can write the planes).
// beta = 2..16 is one transform; 32, 64 and 128 (N <= 2^24) run as beta / 16 blowup-16 transforms of twisted
// coefficients whose planes land in the same layout (lde_plan, ntt_plan.hpp). scratch: npoly * beta * n words;
// T.tw must reach N entries and T.fs hold the tables of (logn, min(logbeta, 4)) (ensure_fourstep)
void launch_lde(const u64* coef, u64 coef_stride, u64* out, u64* scratch, int npoly, int logn, int logbeta,
                const Tables& T, hipStream_t s, const unsigned char* skip = nullptr);
// inverse: evals[poly][n] at 7^off7 * w_n^i -> coefficients (first `keep` written, stride out_stride)
void launch_interpolate(const u64* evals, u64 in_stride, u64* out, u64 out_stride, u64* scratch, int npoly, int logn,
                        bool off7, u64 keep, const Tables& T, hipStream_t s, const unsigned char* skip = nullptr);

// ---- device-side Fiat-Shamir (winter-crypto DefaultRandomCoin<Blake3_256>, as host_common.hpp Coin).
// Each transcript step runs in the kernel that produces its input, one proof per block; the host
// replays the same steps from the roots and the OOD frame afterwards. fail[b] = 1 when a draw was
// rejected 1000 times in a row or z = 0.
struct DevCoin {
    Digest seed;
    u64 counter;
    u64 pad;
};
// step run on a Merkle root by launch_merkle_lde / launch_merkle_fri: reseed with the root, then
//   COEFFS (trace root): the 15 composition coefficients -> out = coeffs [B][15][D]
//   OOD_POINT (composition root): z -> out = zpts [B][2][D] = (z, z g)
//   FRI_ALPHA (FRI layer root): alpha -> out = alpha7 [B][D] = alpha * 7^-1
struct CoinStep {
    enum Kind : int { NONE = 0, COEFFS = 1, OOD_POINT = 2, FRI_ALPHA = 3 };
    int kind = NONE;
    int ext = 1;
    DevCoin* coins = nullptr;
    int* fail = nullptr;
    u64* out = nullptr;
    u64 g = 0;                  // OOD_POINT: the trace domain generator
    Digest* root_out = nullptr;  // root of proof b also stored at root_out[b] (one contiguous D2H)
    u64* hist = nullptr;         // FRI_ALPHA: the raw alpha of proof b also stored at hist[b][D]
};
// step run by launch_ood on the OOD frame (when coins is set): reseed with hash(trace frame) and
// hash(H(z)), draw a_0..a_6 and gamma, and form the DEEP parameters dp [B] from zpts [B][2][D]
struct DeepCoinStep {
    DevCoin* coins = nullptr;
    int* fail = nullptr;
    const u64* zpts = nullptr;
    DeepParams* dp = nullptr;
    u64 ginv = 0;  // g^-1
};

// ---- burn records (burn_record.hip) ----
// The head of the chain of a unit whose statements are packed records in device memory: for record b < B,
// air_out[b] = its AIR constants (validation does not stop the marshalling: an invalid record's slot runs through
// the chain like any other), coin_out[b] = its transcript's coin as Coin::init leaves it (seed = BLAKE3 of ctx ||
// the 12 public inputs, counter 0), status_out[b] = record_status. One wave per record; the records are only read
struct CoinContext {
    u64 e[8];  // Context::to_elements (host_common.hpp context_elements)
};
void launch_burn_marshal(const xfg_burn_record* records, int B, const CoinContext& ctx, AirConst* air_out,
                         DevCoin* coin_out, int* status_out, hipStream_t s);
// Keccak-256 of `count` single-block messages msgs [count][136], lens[i] <= 135 -> out [count][32] (out 8-byte
// aligned), by the record kernel's permutation
void launch_keccak256(const uint8_t* msgs, const u32* lens, int count, uint8_t* out, hipStream_t s);

// ---- Merkle (merkle.hip; heap layout: nodes[1] = root, nodes[L + i] = leaf i) ----
// A commitment is one call: the leaves, every level above them up to the root, then the transcript
// step `cs` on the root. Which kernels run, and the level each stops at, is merkle.hip's business.
// LDE commitment of npoly trees over lde [npoly][nc][beta][n] (coset-major): nodes [npoly][2n], of which
// the levels from the row pairs up are stored (heap [1, n)); the subtree over the beta leaves of row m
// tops out at heap node n + m and stays in registers. nc in {1, 2, 7}, beta a power of two in 2..128: any
// other pair throws std::invalid_argument. cc (nc = 7 only; a trace LDE): the planes of its flagged columns are not read
void launch_merkle_lde(const u64* lde, int nc, Digest* nodes, int npoly, int logn, int logbeta, hipStream_t s,
                       const CoinStep& cs = CoinStep{}, const ColConst& cc = ColConst{});
// recompute the local subtree heap (2 * beta digests, slot 1 = top, leaf t at beta + t) of LDE
// rows entries[e] = proof << logn | m, for Merkle openings
void launch_open_rows(const u64* lde, int nc, const u64* entries, u64 count, Digest* out, int logn, int logbeta,
                      hipStream_t s, const ColConst& cc = ColConst{});
// FRI layer commitment: leaf i = values at natural indices i + k*rows, k < fold (coset-major source when
// coset_major, else natural); nodes [npoly][2 rows], every level stored (leaves at nodes[rows + i]).
// fold in {2, 4, 8, 16}, ext in {1, 2}: anything else throws std::invalid_argument
void launch_merkle_fri(const u64* vals, u64 val_stride, u64 comp_stride, bool coset_major, int logn, int logbeta,
                       u64 rows, Digest* nodes, int npoly, int ext, int fold, hipStream_t s,
                       const CoinStep& cs = CoinStep{});

// ---- AIR ----
// Trace::validate on the device (trace_check_kernel): keys[proof] = the smallest key of what the trace
// [npoly][7][n] violates, TRACE_KEY_VALID (all ones) when nothing. A key is kind << 62 | step << 3 | index,
// so that their order is the order of the report: a cell >= p first (index = column; such a cell is also
// replaced by its canonical value, so `trace` is the lane's copy), then the assertions by number
// (0..6 = columns 0..6 at step 0, 7 = column 4 at step n - 1; step-major order is number order), then
// the transition constraints by step and number 0..6 (steps 0..n-2). with_air = false: the canonicity
// test alone. Sets keys with a memset on s first; npoly <= 65535
// (TRACE_KEY_VALID, the kinds and trace_key itself: trace_layout.hpp, which the host shares)
static_assert(TRACE_FIELD_P == P, "trace_layout.hpp restates the field's prime");
void launch_trace_check(u64* trace, const AirConst* air, u64* keys, int logn, int npoly, bool with_air, hipStream_t s);
// The check on one row, the one statement of the reporting order: the key of what step s of a trace of n steps
// violates first, TRACE_KEY_VALID when nothing. cur: the row's seven cells, canonical; bad: bit c set where
// cell c was >= p as it was loaded (reported before anything else, the lowest column first); nxt4: the
// canonical cell [4][s + 1], read below the last step only. AIR = false: the canonicity test alone.
// Called by trace_check_kernel (a trace in the lane's buffer) and trace_ingest_probe_kernel (columns.hip: the
// caller's buffer in any layout)
template <bool AIR>
__device__ __forceinline__ u64 trace_row_key(const AirConst& A, const u64 (&cur)[7], unsigned bad, u64 nxt4, u64 s, u64 n) {
    if (bad) return trace_key(TRACE_KEY_NONCANONICAL, s, (unsigned)__builtin_ctz(bad));
    u64 key = TRACE_KEY_VALID;
    if constexpr (AIR) {
        if (s + 1 < n) {
            u64 r[7];
            air_transition(A, cur, nxt4, r);
#pragma unroll
            for (int c = 6; c >= 0; c--)
                if (r[c] != 0) key = trace_key(TRACE_KEY_TRANSITION, s, (unsigned)c);
        } else if (cur[4] != AIR_LAST_STATE) {
            key = trace_key(TRACE_KEY_ASSERTION, s, 7);
        }
        if (s == 0) {  // after the rest: an assertion precedes every transition, and number 7 when n = 1
            u64 v0[7];
            air_step0_values(A, v0);
#pragma unroll
            for (int c = 6; c >= 0; c--)
                if (cur[c] != v0[c]) key = trace_key(TRACE_KEY_ASSERTION, 0, (unsigned)c);
        }
    }
    return key;
}
// the rows' keys reduced to a minimum over the wave with shuffles (every lane of the wave takes part); only a
// wave that found something issues an atomicMin on the proof's word, so a valid trace issues none
__device__ __forceinline__ void trace_key_commit(u64 key, u64* word) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const u32 lo = __shfl_xor((u32)key, m, 64), hi = __shfl_xor((u32)(key >> 32), m, 64);
        const u64 o = (u64)lo | ((u64)hi << 32);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != TRACE_KEY_VALID) atomicMin((unsigned long long*)word, (unsigned long long)key);
}
// composition evaluations over the CE domain 7*<w_2n> (natural order) from the trace LDE
// div = constraint divisor table [3][2][n] from ce_divisor_table()
// ext = extension degree D: coeffs [B][15][D], ce planes [B][D][2n]; cc: as for launch_merkle_lde
// uni [B] (required with cc.flags): the terms of the constraint sums that a proof's constant columns make the
// same at every point (air.hpp CeUniform), written here by a one-thread-per-proof kernel ahead of the evaluation
void launch_constraint_eval(const u64* lde, const AirConst* air, const u64* coeffs, const u64* div, u64* ce, int logn,
                            int logbeta, int npoly, int ext, hipStream_t s, const ColConst& cc = ColConst{},
                            CeUniform* uni = nullptr);

// ---- OOD / DEEP ----
// partial: [B][ood_partial_count(logn)][15] per-block sums, kept for launch_deep
// ext = D: zpts [B][2][D], hcoef planes [B][D][n], partial [B][count][15][D], ood [B][15][D]
// cc (both; flags set): coef is the trace's coefficients [B][7][n] whose flagged columns' planes hold
// nothing -- a constant column is its value, a shared one proof 0's plane; without it every plane is read
void launch_ood(const u64* coef, const u64* hcoef, const u64* zpts, u64* partial, u64* ood, int logn, int npoly,
                int ext, hipStream_t s, const DeepCoinStep& dc = DeepCoinStep{}, const ColConst& cc = ColConst{});
u64 ood_partial_count(int logn);
// carry: [B][ood_partial_count(logn)][2][D]; deep planes [B][D][n]
void launch_deep(const u64* coef, const u64* hcoef, const DeepParams* dp, const u64* partial, u64* carry, u64* deep,
                 int logn, int npoly, int ext, hipStream_t s, const ColConst& cc = ColConst{});

// ---- FRI ----
// FRI layer value at natural index K of a layer stored coset-major (layer 0) or natural
__device__ __forceinline__ u64 layer_at(const u64* base, bool coset_major, int logn, int logbeta, u64 K) {
    if (!coset_major) return base[K];
    u64 t = K & ((1ULL << logbeta) - 1), m = K >> logbeta;
    return base[(t << logn) + m];
}
// alpha7 [B][D] = alpha * 7^-1; E values as D planes comp_stride apart; out planes [B][D][out_stride];
// rows = 2^logD / fold, fold in {2, 4, 8, 16} (any other throws std::invalid_argument)
void launch_fri_fold(const u64* vals, u64 val_stride, u64 comp_stride, bool coset_major, int logn, int logbeta,
                     u64 rows, int logD, const u64* alpha7, u64* out, u64 out_stride, const Tables& T, int npoly,
                     int ext, int fold, hipStream_t s);

// ---- openings ----
// several gathers in one launch: segment k copies src[k][idx[first[k] + j]] to dst[k][j],
// j < first[k + 1] - first[k], as u64 or as Digest (digest[k]).
// Segment cc_seg (-1: none) reads a trace LDE whose flagged planes hold nothing: an index whose plane
// idx >> cc_shift (cc_shift = logn + logbeta, the plane = proof * 7 + column) is constant yields cc's value,
// and one whose plane is shared is read from the same column's plane of proof 0
struct GatherSet {
    static constexpr int MAX = 24;
    int nseg = 0;
    const void* src[MAX];
    void* dst[MAX];
    int digest[MAX];
    u64 first[MAX + 1] = {0};
    int cc_seg = -1, cc_shift = 0;
    ColConst cc;
};
void launch_gather_set(const GatherSet& g, const u64* idx, hipStream_t s);

// contiguous device regions packed end to end into one block (segment k: words[k] 32-bit words
// from src[k] to dst + off[k] words); dst may be device-mapped pinned host memory
struct PackSet {
    static constexpr int MAX = 12;
    int nseg = 0;
    const void* src[MAX];
    u64 off[MAX], words[MAX];
};
void launch_pack(const PackSet& p, void* dst, hipStream_t s);

// ---- proof-of-work search (grind.hip) ----
// out[b] (may be device-mapped pinned host memory) = the smallest nonce in [first, max_nonce] for which
// BLAKE3(seeds[b] || nonce_le8) has >= grind (<= 32) trailing zero bits in its first 8 LE bytes, 0 where
// there is none. state: grind_state_words(B) words of device memory, set here (two memsets on s).
// chunk_log, blocks: grind_plan (grind_plan.hpp) or forced; the block size follows from chunk_log
constexpr size_t grind_state_words(size_t B) { return 2 * ((B + 1) & ~(size_t)1); }  // best, next_chunk: 16 B multiples
void launch_grind(const Digest* seeds, u64* state, u64* out, unsigned B, unsigned grind, u64 first, u64 max_nonce,
                  unsigned chunk_log, unsigned blocks, hipStream_t s);

}  // namespace xfg
