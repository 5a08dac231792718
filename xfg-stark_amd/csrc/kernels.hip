// HIP kernels (CDNA4 / gfx950) for the XFG burn-proof STARK hot path.
//
// Replaces, inside Winterfell 0.8.3 `Prover::prove` as bound by the reference
// (src/burn_mint_air.rs:479-531, called at src/burn_mint_prover.rs:124-126):
//   - DefaultConstraintEvaluator with XfgBurnMintAir::evaluate_transition (:335-378) and the
//     8 assertions (:380-395), batch-inverted divisors
//   - CompositionPoly / DeepCompositionPoly: OOD evaluation, coefficient-domain DEEP combine with
//     synthetic division expressed as a weighted suffix scan
//   - FriProver::build_layers: fold by 2, 4, 8 or 16 (apply_drp)
// and the gathers / packing of the openings and the replay block. The LDE is ntt.hip; the Merkle
// commitments (trace, composition, FRI layers) and the transcript step on their roots are merkle.hip;
// the device transcript itself is dev_coin.hpp (here: the DEEP draws, deep_coin_block).
// All arithmetic is 64-bit Goldilocks integer work: HBM/VALU bound, no MFMA.
#include "dev_coin.hpp"
#include "dispatch.hpp"
#include "field_dft.hpp"
#include "hip_util.hpp"
#include <algorithm>
#include <stdexcept>

namespace xfg {

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m, int w) {
    u32 lo = __shfl_xor((u32)v, m, w), hi = __shfl_xor((u32)(v >> 32), m, w);
    return (u64)lo | ((u64)hi << 32);
}

// ============================================================================ AIR
// The AIR itself (the constraints on one row, the step-0 values, which columns a constraint reads and the
// split of the sums by constant columns) is air.hpp; writing a generated trace is columns.hip.
struct CeArgs {
    const u64* lde;
    const AirConst* air;
    const u64* coeffs;
    const u64* div;  // [3][2][n]: (x - g^(n-1))/(x^n - 1), 1/(x - 1), 1/(x - g^(n-1)) by (parity, m)
    u64* ce;
    int logn, logbeta;
    ColConst cc;  // CC instantiations: the trace's constant columns, whose LDE planes hold nothing
    const CeUniform* uni;  // CC: [proof] the terms those columns make the same at every point (ce_uniform_kernel)
};
// The part of a proof's constraint sums that its constant columns fix (air.hpp ce_uniform_of), one thread per
// proof, between the coefficient draw on the trace root and the evaluation: the constraints whose columns
// are all constant, the assertion terms of the constant columns. The evaluation starts its sums from these
template <int D>
__global__ __launch_bounds__(64) void ce_uniform_kernel(const AirConst* air, const u64* coeffs, ColConst cc,
                                                        CeUniform* uni, int npoly) {
    const int proof = blockIdx.x * blockDim.x + threadIdx.x;
    if (proof >= npoly) return;
    const RowConst rc = row_const_lane(cc, (u64)proof);
    uni[proof] = ce_uniform_of<D>(air[proof], coeffs + (u64)proof * 15 * D, rc.mask, rc.v);
}
// One thread per constraint-evaluation point i = 2m + par of the CE domain 7*<w_2n>
// (ce_to_lde_blowup = beta/2: CE point i is LDE row i*beta/2, i.e. coset t = par*beta/2, row m).
// Threads walk m fastest inside one parity so the coset-major LDE reads are coalesced.
// The divisor inverses are data independent and come from a per-(n, beta) table.
// D = extension degree of the composition coefficients (1: FieldExtension::None, 2: Quadratic);
// the evaluations are written as D coordinate planes ce[proof][c][nce].
// CC: the frame's cells of a constant column (the next row's column 4 among them) are the column's value,
// read once per block (the block's proof is blockIdx.y) in place of their loads, and those of a shared
// column come from proof 0's planes (a.lde itself); the AIR stays generic. The sums start from the proof's
// uniform part (a.uni) and a term in it is neither formed nor added: its mask bit is clear, the same in
// every lane of the block, so the branches around the terms are scalar.
template <int D, bool CC>
__global__ __launch_bounds__(256) void constraint_eval_kernel(CeArgs a) {
    using F = FE<D>;
    const u64 n = 1ULL << a.logn, nce = 2 * n;
    const int proof = blockIdx.y;
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // grid covers nce exactly
    const u64 par = g >> a.logn, m = g & (n - 1), i = 2 * m + par;
    const AirConst& A = a.air[proof];
    const u64* co = a.coeffs + (u64)proof * 15 * D;
    const u64 beta = 1ULL << a.logbeta;
    const u64* lde = a.lde + (u64)proof * 7 * beta * n;
    const u64 t = par * (beta / 2), mn = (m + 1) & (n - 1);
    u64 cur[7], nxt4;
    if constexpr (CC) {
        const RowConst rc = row_const_uniform(a.cc, (u64)proof);
#pragma unroll
        for (int c = 0; c < 7; c++) {
            if ((rc.mask >> c) & 1) cur[c] = rc.v[c];
            else cur[c] = rc.plane(c, lde, a.lde)[(((u64)c << a.logbeta) + t) * n + m];
        }
        if ((rc.mask >> 4) & 1) nxt4 = rc.v[4];
        else nxt4 = rc.plane(4, lde, a.lde)[((4ULL << a.logbeta) + t) * n + mn];
    } else {
#pragma unroll
        for (int c = 0; c < 7; c++) cur[c] = lde[(((u64)c << a.logbeta) + t) * n + m];
        nxt4 = lde[((4ULL << a.logbeta) + t) * n + mn];
    }
    // divisor inverses loaded with the frame (not next to the multiplies that use them)
    const u64 di = par * n + m;
    const u64 dv0 = a.div[di], dv1 = a.div[nce + di], dv2 = a.div[2 * nce + di];
    F tr, b0, b1;
    if constexpr (CC) {
        const CeUniform& U = a.uni[proof];
        const unsigned tr_live = __builtin_amdgcn_readfirstlane(U.tr_live);
        const unsigned as_live = __builtin_amdgcn_readfirstlane(U.as_live);
        ce_live_sums<D>(U, tr_live, as_live, co, A, cur, nxt4, tr, b0, b1);
    } else {
        u64 r[7];
        air_transition(A, cur, nxt4, r);
        tr = F::zero();
#pragma unroll
        for (int c = 0; c < 7; c++) tr = fe_add(tr, fe_mulb(F::load(co + c * D), r[c]));
        // assertions (src/burn_mint_air.rs:380-395): step 0 on columns 0..6, step n-1 on column 4
        u64 v0[7];
        air_step0_values(A, v0);
        b0 = F::zero();
#pragma unroll
        for (int c = 0; c < 7; c++) b0 = fe_add(b0, fe_mulb(F::load(co + (7 + c) * D), gl_sub(cur[c], v0[c])));
        b1 = fe_mulb(F::load(co + 14 * D), gl_sub(cur[4], AIR_LAST_STATE));
    }
    F val = fe_mulb(tr, dv0);
    val = fe_add(val, fe_mulb(b0, dv1));
    val = fe_add(val, fe_mulb(b1, dv2));
#pragma unroll
    for (int c = 0; c < D; c++) a.ce[((u64)proof * D + c) * nce + i] = val.c(c);
}
void launch_constraint_eval(const u64* lde, const AirConst* air, const u64* coeffs, const u64* div, u64* ce, int logn,
                            int logbeta, int npoly, int ext, hipStream_t s, const ColConst& cc, CeUniform* uni) {
    if (cc.flags && !uni) throw std::invalid_argument("constraint evaluation: constant columns need the uniform-part buffer");
    CeArgs a;
    a.lde = lde; a.air = air; a.coeffs = coeffs; a.div = div; a.ce = ce; a.logn = logn; a.logbeta = logbeta;
    a.cc = cc;
    a.uni = uni;
    u64 nce = 2ULL << logn;
    int threads = nce < 256 ? (int)nce : 256;
    dim3 g((unsigned)(nce / threads), npoly);
    with_ext(ext, [&](auto D) {
        with_bool(cc.flags != nullptr, [&](auto CC) {
            if constexpr (CC)
                XFG_LAUNCH(ce_uniform_kernel<D>, dim3((unsigned)((npoly + 63) / 64)), dim3(64), 0, s, air, coeffs, cc, uni,
                           npoly);
            XFG_LAUNCH((constraint_eval_kernel<D, CC>), g, dim3(threads), 0, s, a);
        });
    });
}

// Trace::validate (winter-air 0.8) on the device: one thread per step reads its row (seven coalesced
// 8-byte streams, no LDS) and, for the column-4 constraint alone, cell [4][step + 1] of the next row;
// it checks the assertions that fall on its step and, below the last step (Winterfell's one transition
// exemption), the seven transition expressions. What it finds first in Winterfell's reporting order
// becomes a key (trace_key, kernels.hpp); the keys are reduced to a minimum over the wave with shuffles
// and only a wave that found something issues an atomicMin on the proof's word, so a valid trace issues
// none. keys[proof] was set to all ones by the launch wrapper.
// A cell >= p is reported before anything else and replaced by its canonical value in `trace` (the
// lane's copy, never the caller's buffer), so that the chain behind the check runs on field elements;
// the thread of step - 1 may read that cell before or after the store, and what it then reports is
// below the non-canonical key either way.
// AIR = false: the canonicity test alone (device-resident traces proven without validation)
template <bool AIR>
__global__ __launch_bounds__(256) void trace_check_kernel(u64* trace, const AirConst* air, u64* keys, int logn) {
    const u64 n = 1ULL << logn;
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const int proof = blockIdx.y;
    u64 key = TRACE_KEY_VALID;
    if (s < n) {  // no early return: every lane of the wave takes part in the shuffles
        u64* tr = trace + (u64)proof * 7 * n;
        u64 cur[7];
#pragma unroll
        for (int c = 0; c < 7; c++) cur[c] = tr[(u64)c * n + s];
        u64 nxt4 = 0;
        if (AIR && s + 1 < n) nxt4 = tr[4 * n + s + 1];
        unsigned bad = 0;
#pragma unroll
        for (int c = 0; c < 7; c++) {
            if (cur[c] >= P) {
                bad |= 1u << c;
                cur[c] -= P;
                tr[(u64)c * n + s] = cur[c];
            }
        }
        if (nxt4 >= P) nxt4 -= P;
        key = trace_row_key<AIR>(air[proof], cur, bad, nxt4, s, n);
    }
    trace_key_commit(key, keys + proof);
}
void launch_trace_check(u64* trace, const AirConst* air, u64* keys, int logn, int npoly, bool with_air, hipStream_t s) {
    const u64 n = 1ULL << logn;
    HIPCHK(hipMemsetAsync(keys, 0xFF, (size_t)npoly * 8, s));  // TRACE_KEY_VALID
    dim3 g((unsigned)((n + 255) / 256), npoly);
    with_bool(with_air, [&](auto AIR) { XFG_LAUNCH(trace_check_kernel<AIR>, g, dim3(256), 0, s, trace, air, keys, logn); });
}

// ============================================================================ OOD
// Blocks own CHUNK = T * OOD_R consecutive coefficients (T = min(256, n / OOD_R) threads, thread t
// takes j = base + r T + t: coalesced). Per block the 15 partial sums
//   sum_{j in block} T_c[j] z^j, sum T_c[j] (zg)^j (c < 7), sum H[j] z^j
// are stored in `partial` [proof][block][15]: ood_final adds them up, and the DEEP quotient reuses
// them as its per-block carries (no second pass over the coefficients for the block sums).
#define OOD_R 8
static inline int ood_threads(u64 n) { return (int)std::min<u64>(256, n / OOD_R); }

template <int D>
__device__ __forceinline__ FE<D> fe_pow(FE<D> b, u64 e) {
    FE<D> r = FE<D>::zero();
    r.a = 1;
    while (e) {
        if (e & 1) r = fe_mul(r, b);
        b = fe_mul(b, b);
        e >>= 1;
    }
    return r;
}
template <int D>
__device__ __forceinline__ FE<D> fe_plane(const u64* planes, u64 plane_stride, u64 j) {  // coordinates from planes
    FE<D> v;
    v.a = planes[j];
    if constexpr (D == 2) v.b = planes[plane_stride + j];
    return v;
}

// zpts [proof][2][D] = (z, z g); coef [proof][7][n] (base); hcoef [proof][D][n];
// partial [proof][block][15][D]
// CC (the trace's coefficients behind a ColConst: the planes of its flagged columns hold nothing). A
// constant column's polynomial is the constant v, so both of its frame entries are v: block 0's partials
// are (v, 0) and every other block's 0, which is what the dense sums of (v, 0, ..., 0) come to, and the
// column takes no load and no multiply. A shared column is read from proof 0's coefficients (coef itself)
template <int D, bool CC>
__global__ __launch_bounds__(256) void ood_kernel(const u64* coef, const u64* hcoef, const u64* zpts, u64* partial,
                                                  int logn, ColConst colc) {
    using F = FE<D>;
    __shared__ u64 zb[4][D];
    __shared__ u64 red[4][15][D];
    const u64 n = 1ULL << logn;
    const int proof = blockIdx.y, t = threadIdx.x, T = blockDim.x;
    const u64 base = (u64)blockIdx.x * T * OOD_R;
    const F z = F::load(zpts + (u64)proof * 2 * D), zg = F::load(zpts + (u64)proof * 2 * D + D);
    for (int k = t; k < 4; k += T)  // the block's four start powers on four threads (a lone proof waits on them)
        fe_pow(k & 1 ? zg : z, k < 2 ? base : (u64)T).store(zb[k]);
    __syncthreads();
    F pz = fe_mul(F::load(zb[0]), fe_pow(z, (u64)t)), pzg = fe_mul(F::load(zb[1]), fe_pow(zg, (u64)t));
    const F zT = F::load(zb[2]), zgT = F::load(zb[3]);
    const u64* co = coef + (u64)proof * 7 * n;
    const u64* h = hcoef + (u64)proof * D * n;
    F acc[15];
#pragma unroll
    for (int q = 0; q < 15; q++) acc[q] = F::zero();
    // the 8 (7 columns + H) values of index j + T are loaded before the products of index j run:
    // a load next to its multiply would be waited for one at a time (the field primitives are asm
    // statements the scheduler does not move loads across)
    // CC: the proof's flags are wave-uniform (a block per proof), so the branches around a constant
    // column's loads and products are scalar; live(c) is a compile-time true without CC
    RowConst rc = {};
    if constexpr (CC) rc = row_const_uniform(colc, (u64)proof);
    auto live = [&](int c) { return !CC || !((rc.mask >> c) & 1); };
    auto col = [&](int c) { return (CC ? rc.plane(c, co, coef) : co) + (u64)c * n; };
    u64 cur[7] = {}, nxt[7] = {};
    F hc, hn;
    {
        const u64 j = base + t;
#pragma unroll
        for (int c = 0; c < 7; c++)
            if (live(c)) cur[c] = col(c)[j];
        hc = fe_plane<D>(h, n, j);
    }
#pragma unroll
    for (int r = 0; r < OOD_R; r++) {
        if (r + 1 < OOD_R) {
            const u64 j = base + (u64)(r + 1) * T + t;
#pragma unroll
            for (int c = 0; c < 7; c++)
                if (live(c)) nxt[c] = col(c)[j];
            hn = fe_plane<D>(h, n, j);
        }
#pragma unroll
        for (int c = 0; c < 7; c++) {
            if (!live(c)) continue;
            acc[2 * c] = fe_add(acc[2 * c], fe_mulb(pz, cur[c]));
            acc[2 * c + 1] = fe_add(acc[2 * c + 1], fe_mulb(pzg, cur[c]));
        }
        acc[14] = fe_add(acc[14], fe_mul(hc, pz));
        pz = fe_mul(pz, zT);
        pzg = fe_mul(pzg, zgT);
        if (r + 1 < OOD_R) {  // (the last iteration loaded nothing)
#pragma unroll
            for (int c = 0; c < 7; c++) cur[c] = nxt[c];
            hc = hn;
        }
    }
    // wave reduction, then across the (up to 4) waves
    const int W = T < 64 ? T : 64;
    for (int m = W / 2; m > 0; m >>= 1) {
#pragma unroll
        for (int q = 0; q < 15; q++) {
            acc[q].a = gl_add(acc[q].a, shfl_xor_u64(acc[q].a, m, W));
            if constexpr (D == 2) acc[q].b = gl_add(acc[q].b, shfl_xor_u64(acc[q].b, m, W));
        }
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 15; q++) acc[q].store(red[t >> 6][q]);
    }
    __syncthreads();
    for (int qc = t; qc < 15 * D; qc += T) {  // T may be below 15 D for short traces
        const int q = qc / D, cc = qc % D;
        u64 v = red[0][q][cc];
        for (int w = 1; w < (T + 63) / 64; w++) v = gl_add(v, red[w][q][cc]);
        if constexpr (CC) {  // both frame entries of a constant column: v in block 0's partial, 0 elsewhere
#pragma unroll
            for (int c = 0; c < 7; c++)
                if ((q >> 1) == c && q < 14 && ((rc.mask >> c) & 1)) v = (blockIdx.x == 0 && cc == 0) ? rc.v[c] : 0;
        }
        partial[((u64)proof * gridDim.x + blockIdx.x) * 15 * D + qc] = v;
    }
}
// DEEP coefficients (Prover::prove after the OOD frame), 128 threads for proof b with the frame o[15 D]
// in LDS: wave 0 runs the transcript (reseed with the two element hashes, the 8 draws), wave 1
// meanwhile inverts z (1 / (z g) = (1 / z) g^-1: one inversion)
__device__ void deep_coin_block(const DeepCoinStep& dc, int b, const u64* o, int D) {
    __shared__ u64 ab[8][2];  // a_0..a_6, gamma
    __shared__ E2 zinv;
    __shared__ int ok_s;
    const u64* zb = dc.zpts + (u64)b * 2 * D;
    const E2 z{zb[0], D == 2 ? zb[1] : 0}, zg{zb[D], D == 2 ? zb[D + 1] : 0};
    const bool zz = z.a == 0 && z.b == 0;  // z g == 0 <=> z == 0
    if (threadIdx.x < 64) {
        DevCoin c = dc.coins[b];
        dev_reseed(c, dev_hash_elems(o, 14 * D));  // [T_c(z), T_c(zg)] x 7, coordinates interleaved
        dev_reseed(c, dev_hash_elems(o + 14 * D, D));  // H(z)
        const bool ok = wave_draw_e(c, 8, D, &ab[0][0], 2);
        if (threadIdx.x == 0) {
            dc.coins[b] = c;
            ok_s = ok;
        }
    } else if (threadIdx.x == 64) {
        zinv = zz ? E2{0, 0} : e2_inv(z);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    DeepParams P = {};
    for (int k = 0; k < 7; k++)
        for (int d = 0; d < D; d++) P.a[k][d] = ab[k][d];
    for (int d = 0; d < D; d++) P.gamma[d] = ab[7][d];
    auto put = [](u64* d, E2 v) { d[0] = v.a; d[1] = v.b; };
    auto ood_e = [&](int q) { return E2{o[q * D], D == 2 ? o[q * D + 1] : 0}; };
    put(P.z, z);
    put(P.zg, zg);
    put(P.zinv, zinv);
    put(P.zginv, e2_mulb(zinv, dc.ginv));
    E2 c1 = e2_mul(E2{P.gamma[0], P.gamma[1]}, ood_e(14)), c2{0, 0};
    for (int k = 0; k < 7; k++) {
        const E2 a{P.a[k][0], P.a[k][1]};
        c1 = e2_add(c1, e2_mul(a, ood_e(2 * k)));
        c2 = e2_add(c2, e2_mul(a, ood_e(2 * k + 1)));
    }
    put(P.c1, c1);
    put(P.c2, c2);
    dc.dp[b] = P;
    if (!ok_s || zz) dc.fail[b] = 1;
}
// OOD block partials -> the frame ood[proof][15][D]; then the DEEP draws when dc.coins is set
// The nblk partials of each of the 15 D values are summed by S threads (the most that fit the block), each
// loading 8 partials before it adds them: one thread per value walking all nblk with a load before
// each (asm) add waited for every load in turn -- nblk = 32 round trips at 2^16, 512 at 2^20.
__global__ __launch_bounds__(128) void ood_final_kernel(const u64* partial, int nblk, int d, u64* ood, DeepCoinStep dc) {
    __shared__ u64 o[30];
    __shared__ u64 red[8][30];
    const int proof = blockIdx.x, t = threadIdx.x, nq = 15 * d;
    int S = 1;
    while (nq * S * 2 <= (int)blockDim.x && S < 8) S <<= 1;
    const int q = t % nq, k = t / nq;
    if (k < S) {
        const u64* pp = partial + (u64)proof * nblk * nq + q;
        u64 s = 0;
        for (int b0 = k; b0 < nblk; b0 += 8 * S) {
            u64 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int b = b0 + u * S;
                v[u] = b < nblk ? pp[(u64)b * nq] : 0;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) s = gl_add(s, v[u]);
        }
        red[k][q] = s;
    }
    __syncthreads();
    if (t < nq) {
        u64 s = red[0][t];
        for (int j = 1; j < S; j++) s = gl_add(s, red[j][t]);
        ood[(u64)proof * nq + t] = s;
        o[t] = s;
    }
    if (!dc.coins) return;
    __syncthreads();
    deep_coin_block(dc, proof, o, d);
}
void launch_ood(const u64* coef, const u64* hcoef, const u64* zpts, u64* partial, u64* ood, int logn, int npoly,
                int ext, hipStream_t s, const DeepCoinStep& dc, const ColConst& cc) {
    const u64 n = 1ULL << logn;
    const int T = ood_threads(n), nblk = (int)(n / ((u64)T * OOD_R));
    const dim3 g(nblk, npoly), b(T);
    with_ext(ext, [&](auto D) {
        with_bool(cc.flags != nullptr, [&](auto CC) {
            XFG_LAUNCH((ood_kernel<D, CC>), g, b, 0, s, coef, hcoef, zpts, partial, logn, cc);
        });
    });
    XFG_LAUNCH(ood_final_kernel, dim3(npoly), dim3(dc.coins ? 128 : 64), 0, s, partial, nblk, ext, ood, dc);
}
u64 ood_partial_count(int logn) {
    const u64 n = 1ULL << logn;
    return n / ((u64)ood_threads(n) * OOD_R);
}

// ============================================================================ DEEP
// DEEP quotient in coefficient form: P1_j = sum a_c T_c[j] + gamma H[j] - [j==0] c1,
// P2_j = sum a_c T_c[j] - [j==0] c2; d_k = q1_k + q2_k with the synthetic-division recurrences
//   q1_k = P1_{k+1} + z q1_{k+1},  q2_k = P2_{k+1} + zg q2_{k+1},  q_{n-1} = 0.
// Same block chunking as the OOD kernel. Block b's entry carry q_e (e = last index of the block)
// is z^-(e+1) * sum_{j > e} P_j z^j, a weighted suffix sum of the OOD block partials
// (deep_carry_kernel). Inside a block every thread owns OOD_R consecutive indices: a backward
// Horner pass gives its chunk map Q_out = L + z^R Q_in, a suffix scan over threads with the
// uniform multiplier z^R gives each thread's Q_in, and a second backward pass writes d_k.
// All of it in E (extension degree D): coefficients, z and the output planes deep[proof][c][n].
template <int D>
__global__ __launch_bounds__(1024) void deep_carry_kernel(const u64* partial, const DeepParams* dp, u64* carry,
                                                          int nblk, int logch) {
    using F = FE<D>;
    __shared__ u64 S1[1024][D], S2[1024][D];
    const int proof = blockIdx.x, b = threadIdx.x;
    const DeepParams& P = dp[proof];
    F b1 = F::zero(), b2 = F::zero();
    if (b < nblk) {
        const u64* pp = partial + ((u64)proof * nblk + b) * 15 * D;
        F t1 = F::zero(), t2 = F::zero();
#pragma unroll
        for (int c = 0; c < 7; c++) {
            const F a = F::load(P.a[c]);
            t1 = fe_add(t1, fe_mul(a, F::load(pp + 2 * c * D)));
            t2 = fe_add(t2, fe_mul(a, F::load(pp + (2 * c + 1) * D)));
        }
        b1 = fe_add(t1, fe_mul(F::load(P.gamma), F::load(pp + 14 * D)));
        b2 = t2;
        if (b == 0) {
            b1 = fe_sub(b1, F::load(P.c1));
            b2 = fe_sub(b2, F::load(P.c2));
        }
    }
    b1.store(S1[b]);
    b2.store(S2[b]);
    __syncthreads();
    for (int off = 1; off < (int)blockDim.x; off <<= 1) {  // inclusive suffix sums
        F v1 = F::load(S1[b]), v2 = F::load(S2[b]);
        if (b + off < (int)blockDim.x) {
            v1 = fe_add(v1, F::load(S1[b + off]));
            v2 = fe_add(v2, F::load(S2[b + off]));
        }
        __syncthreads();
        v1.store(S1[b]);
        v2.store(S2[b]);
        __syncthreads();
    }
    if (b < nblk) {
        const u64 e = (u64)(b + 1) << logch;  // carry into block b: z^-e * sum over blocks after b
        const F x1 = b + 1 < nblk ? F::load(S1[b + 1]) : F::zero();
        const F x2 = b + 1 < nblk ? F::load(S2[b + 1]) : F::zero();
        fe_mul(x1, fe_pow(F::load(P.zinv), e)).store(carry + (((u64)proof * nblk + b) * 2) * D);
        fe_mul(x2, fe_pow(F::load(P.zginv), e)).store(carry + (((u64)proof * nblk + b) * 2 + 1) * D);
    }
}
__device__ __forceinline__ int dpad(int i) { return i + i / OOD_R; }  // chunk stride R+1: no bank pile-up
// CC (as ood_kernel): a constant column's coefficients are (v, 0, ..., 0), so it appears in P1_j, P2_j at
// j = 0 alone, as a_c v, added there (every field addition returns the canonical value, so the order of
// the terms changes no bit); c1, c2 and the DeepParams are what they were. A shared column is read
// from proof 0's coefficients (coef itself)
template <int D, bool CC>
__global__ __launch_bounds__(256) void deep_final_kernel(const u64* coef, const u64* hcoef, const DeepParams* dp,
                                                         const u64* carry, u64* deep, int logn, ColConst colc) {
    using F = FE<D>;
    constexpr int R = OOD_R, CHMAX = 256 * OOD_R, PADN = CHMAX + CHMAX / R;
    __shared__ u64 s1[D][PADN], s2[D][PADN];
    __shared__ u64 S1[256][D], S2[256][D];
    const u64 n = 1ULL << logn;
    const int proof = blockIdx.y, t = threadIdx.x, T = blockDim.x;
    const u64 base = (u64)blockIdx.x * T * R;
    const DeepParams& P = dp[proof];
    const F z = F::load(P.z), zg = F::load(P.zg), gam = F::load(P.gamma);
    F ac[7];
#pragma unroll
    for (int c = 0; c < 7; c++) ac[c] = F::load(P.a[c]);
    const u64* co = coef + (u64)proof * 7 * n;
    const u64* h = hcoef + (u64)proof * D * n;
    auto lds_ld = [&](u64 (*arr)[PADN], int k) {
        F v;
        v.a = arr[0][k];
        if constexpr (D == 2) v.b = arr[1][k];
        return v;
    };
    auto lds_st = [&](u64 (*arr)[PADN], int k, F v) {
        arr[0][k] = v.a;
        if constexpr (D == 2) arr[1][k] = v.b;
    };
    RowConst rc = {};
    if constexpr (CC) rc = row_const_uniform(colc, (u64)proof);
    // 1. P1, P2 (coalesced reads) into LDS
#pragma unroll 2
    for (int r = 0; r < R; r++) {
        const int li = r * T + t;
        const u64 j = base + li;
        F sacc = F::zero();
#pragma unroll
        for (int c = 0; c < 7; c++) {
            if constexpr (CC) {
                if ((rc.mask >> c) & 1) continue;  // wave-uniform
                sacc = fe_add(sacc, fe_mulb(ac[c], rc.plane(c, co, coef)[(u64)c * n + j]));
            } else {
                sacc = fe_add(sacc, fe_mulb(ac[c], co[(u64)c * n + j]));
            }
        }
        if constexpr (CC) {
            if (j == 0) {
#pragma unroll
                for (int c = 0; c < 7; c++)
                    if ((rc.mask >> c) & 1) sacc = fe_add(sacc, fe_mulb(ac[c], rc.v[c]));
            }
        }
        F p1 = fe_add(sacc, fe_mul(gam, fe_plane<D>(h, n, j))), p2 = sacc;
        if (j == 0) {
            p1 = fe_sub(p1, F::load(P.c1));
            p2 = fe_sub(p2, F::load(P.c2));
        }
        lds_st(s1, dpad(li), p1);
        lds_st(s2, dpad(li), p2);
    }
    __syncthreads();
    // 2. chunk maps: L = sum_i z^i P_{a+i}
    const int a = t * R;
    F L1 = F::zero(), L2 = F::zero();
#pragma unroll
    for (int i = R - 1; i >= 0; i--) {
        L1 = fe_add(lds_ld(s1, dpad(a + i)), fe_mul(z, L1));
        L2 = fe_add(lds_ld(s2, dpad(a + i)), fe_mul(zg, L2));
    }
    // 3. suffix scan over threads, multiplier w = z^R; the block carry enters through the last thread
    F w1 = z, w2 = zg;
#pragma unroll
    for (int i = 1; i < R; i <<= 1) {
        w1 = fe_mul(w1, w1);
        w2 = fe_mul(w2, w2);
    }
    const F cin1 = F::load(carry + (((u64)proof * gridDim.x + blockIdx.x) * 2) * D);
    const F cin2 = F::load(carry + (((u64)proof * gridDim.x + blockIdx.x) * 2 + 1) * D);
    if (t == T - 1) {
        L1 = fe_add(L1, fe_mul(w1, cin1));
        L2 = fe_add(L2, fe_mul(w2, cin2));
    }
    L1.store(S1[t]);
    L2.store(S2[t]);
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        F v1 = F::load(S1[t]), v2 = F::load(S2[t]);
        if (t + off < T) {
            v1 = fe_add(v1, fe_mul(w1, F::load(S1[t + off])));
            v2 = fe_add(v2, fe_mul(w2, F::load(S2[t + off])));
        }
        __syncthreads();
        v1.store(S1[t]);
        v2.store(S2[t]);
        __syncthreads();
        w1 = fe_mul(w1, w1);
        w2 = fe_mul(w2, w2);
    }
    F q1 = t + 1 < T ? F::load(S1[t + 1]) : cin1, q2 = t + 1 < T ? F::load(S2[t + 1]) : cin2;
    // 4. backward pass over the chunk: d_k = q1_k + q2_k, then step to k - 1
#pragma unroll
    for (int i = R - 1; i >= 0; i--) {
        const int k = dpad(a + i);
        const F p1 = lds_ld(s1, k), p2 = lds_ld(s2, k);
        lds_st(s1, k, fe_add(q1, q2));
        q1 = fe_add(p1, fe_mul(z, q1));
        q2 = fe_add(p2, fe_mul(zg, q2));
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < D; c++) {
        u64* out = deep + ((u64)proof * D + c) * n + base;
#pragma unroll
        for (int r = 0; r < R; r++) out[r * T + t] = s1[c][dpad(r * T + t)];
    }
}
void launch_deep(const u64* coef, const u64* hcoef, const DeepParams* dp, const u64* partial, u64* carry, u64* deep,
                 int logn, int npoly, int ext, hipStream_t s, const ColConst& cc) {
    const u64 n = 1ULL << logn;
    const int T = ood_threads(n), nblk = (int)(n / ((u64)T * OOD_R));
    int logch = 0;
    while ((1ULL << logch) < (u64)T * OOD_R) logch++;
    int ct = 64;
    while (ct < nblk) ct <<= 1;  // nblk <= 1024 (n <= 2^21, 2048 coefficients per block)
    const dim3 g(nblk, npoly), b(T);
    with_ext(ext, [&](auto D) {
        XFG_LAUNCH(deep_carry_kernel<D>, dim3(npoly), dim3(ct), 0, s, partial, dp, carry, nblk, logch);
        with_bool(cc.flags != nullptr, [&](auto CC) {
            XFG_LAUNCH((deep_final_kernel<D, CC>), g, b, 0, s, coef, hcoef, dp, carry, deep, logn, cc);
        });
    });
}

// ============================================================================ FRI fold
// apply_drp for folding factor F = 2^LOGF (2, 4, 8, 16) with Winterfell's constant domain offset 7 on
// every layer: row i = {v_k at 7 w_D^i zeta^k}, zeta = w_D^rows = w_F;
// c = iDFT_F(v)/F ; result = sum_j c_j (alpha / (7 w_D^i))^j
struct FoldArgs {
    const u64* vals;
    u64 val_stride, comp_stride;
    int coset_major, logn, logbeta;
    u64 rows;
    int logD;
    const u64* alpha7;  // [proof][D]: alpha * 7^-1
    u64* out;           // [proof][D][rows]
    u64 out_stride;
    Tables T;
};
template <int D, int LOGF>
__global__ __launch_bounds__(256) void fri_fold_kernel(FoldArgs a) {
    using F = FE<D>;
    constexpr int NF = 1 << LOGF;
    const int proof = blockIdx.y;
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.rows) return;
    const u64* base = a.vals + (u64)proof * a.val_stride;
    // the size-F inverse DFT per coordinate (base-field twiddles w_F^-k = powers of two for every
    // F <= 16: shifts), natural order in and out, outputs canonicalised for the Horner adds
    u64 c[D][NF];
#pragma unroll
    for (int k = 0; k < NF; k++) {
        const u64 K = i + (u64)k * a.rows;
        c[0][k] = layer_at(base, a.coset_major, a.logn, a.logbeta, K);
        if constexpr (D == 2) c[1][k] = layer_at(base + a.comp_stride, a.coset_major, a.logn, a.logbeta, K);
    }
    F v[NF];
#pragma unroll
    for (int d = 0; d < D; d++) {
        dft_reg<LOGF, true>(c[d]);
#pragma unroll
        for (int k = 0; k < NF; k++) {
            if (d == 0) v[k].a = canon(c[d][k]);
            if constexpr (D == 2) if (d == 1) v[k].b = canon(c[d][k]);
        }
    }
    // y = alpha * 7^-1 * w_D^-i ; Horner
    const F y = fe_mulb(F::load(a.alpha7 + (u64)proof * D), tw_get(a.T, a.logD, i, true));
    F r = v[NF - 1];
#pragma unroll
    for (int j = NF - 2; j >= 0; j--) r = fe_add(fe_mul(r, y), v[j]);
    // 1/F = 2^-LOGF = 2^(192 - LOGF) = -2^(96 - LOGF)
#pragma unroll
    for (int d = 0; d < D; d++) {
        const u64 x = gl_neg(mul_pow2<96 - LOGF>(r.c(d)));
        if (d == 0) r.a = x;
        if constexpr (D == 2) if (d == 1) r.b = x;
    }
#pragma unroll
    for (int c = 0; c < D; c++) a.out[((u64)proof * D + c) * a.out_stride + i] = r.c(c);
}
void launch_fri_fold(const u64* vals, u64 val_stride, u64 comp_stride, bool coset_major, int logn, int logbeta,
                     u64 rows, int logD, const u64* alpha7, u64* out, u64 out_stride, const Tables& T, int npoly,
                     int ext, int fold, hipStream_t s) {
    FoldArgs a;
    a.vals = vals; a.val_stride = val_stride; a.comp_stride = comp_stride; a.coset_major = coset_major ? 1 : 0;
    a.logn = logn; a.logbeta = logbeta; a.rows = rows; a.logD = logD; a.alpha7 = alpha7; a.out = out;
    a.out_stride = out_stride;
    a.T = T;
    int threads = rows < 256 ? (int)rows : 256;
    dim3 g((unsigned)((rows + threads - 1) / threads), npoly);
    with_ext(ext, [&](auto D) {
        with_fold(fold, [&](auto LOGF) { XFG_LAUNCH((fri_fold_kernel<D, LOGF>), g, dim3(threads), 0, s, a); });
    });
}

// ============================================================================ gathers
// all of a unit's opening gathers in one launch: thread i of the grid serves element i - first[k] of
// segment k (the segments are laid end to end in index order; at most GatherSet::MAX of them).
// An element of segment cc_seg whose plane is a constant column is the column's value, and one whose
// plane is a shared column is read at the same place of proof 0's plane (plane = proof * 7 + column):
// those planes of the trace LDE are not written
__global__ void gather_set_kernel(GatherSet g, const u64* idx) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.first[g.nseg]) return;
    int k = 0;
    while (i >= g.first[k + 1]) k++;
    const u64 src = idx[i];
    if (g.digest[k]) {
        const Digest* s = (const Digest*)g.src[k];
        ((Digest*)g.dst[k])[i - g.first[k]] = s[src];
    } else {
        u64 v;
        const u64 plane = src >> g.cc_shift;
        const unsigned f = k == g.cc_seg ? g.cc.flags[plane] : 0u;
        if (f & COL_CONST) v = g.cc.vals[plane * g.cc.val_stride];
        else if (f & COL_SHARED) v = ((const u64*)g.src[k])[src - ((plane - plane % 7) << g.cc_shift)];  // proof 0's plane
        else v = ((const u64*)g.src[k])[src];
        ((u64*)g.dst[k])[i - g.first[k]] = v;
    }
}
void launch_gather_set(const GatherSet& g, const u64* idx, hipStream_t s) {
    const u64 total = g.first[g.nseg];
    if (!total) return;
    XFG_LAUNCH(gather_set_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, idx);
}

// one segment per blockIdx.y, grid-stride over its words
__global__ void pack_kernel(PackSet p, u32* dst) {
    const int k = blockIdx.y;
    const u32* src = (const u32*)p.src[k];
    u32* out = dst + p.off[k];
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < p.words[k]; i += (u64)gridDim.x * blockDim.x)
        out[i] = src[i];
}
void launch_pack(const PackSet& p, void* dst, hipStream_t s) {
    u64 most = 0;
    for (int k = 0; k < p.nseg; k++) most = std::max(most, p.words[k]);
    if (!most) return;
    const unsigned bx = (unsigned)std::min<u64>(32, (most + 255) / 256);
    XFG_LAUNCH(pack_kernel, dim3(bx, p.nseg), dim3(256), 0, s, p, (u32*)dst);
}

}  // namespace xfg
