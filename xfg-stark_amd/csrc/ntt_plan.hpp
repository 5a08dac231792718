// What the four-step NTT launches for a given shape, and where its tables and LDS regions lie: pure
// functions, no HIP (tests/sanitize/ntt_plan.cpp compiles this header with a plain host compiler).
// ntt.hip launches what ntt_plan() returns; its kernels and the table generators (tables.hip) take
// every offset from the layout types here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define XFG_HD __host__ __device__
#else
#define XFG_HD
#endif

namespace xfg {

// split n = R * C: evenly below 2^18, C = 2R from 2^18 on except 2^20 (faster at 2^18; see
// scripts/ntt_split.py; at 2^24 the splits C = 512 / 2048 / 4096 measured slower than 1024)
constexpr void ntt_split(int logn, int& logR, int& logC) {
    if (logn >= 18) {
        logC = logn == 20 ? 10 : logn / 2 + 1;  // 2^20: R = C = 1024, both passes wide-tiled (3 % faster)
    } else {
        logC = logn - logn / 2;
    }
    logR = logn - logC;
}

// LDS tile: row `seq` of length S at seq * PITCH; element i at i + (i >> P), one pad word per 2^P
// elements, P = log2 elements per thread (4 or 5). The pad word makes the stride-2^P stores of a
// full-radix first step (lanes along a row, 2^P contiguous outputs each) conflict-free: 16 lanes
// land on 16 different 8-byte bank pairs. The pitch does the same for lanes walking across rows:
// a 16-lane group spans 2^L rows and 16 / 2^L consecutive elements, so the pitch must be an odd
// multiple of 16 / 2^L mod 16 (radix 16: odd; radix 32 with 8-row tiles, pass B at n = 2^20: 2 mod
// 4 -- the odd pitch there cost 2-way conflicts on every last-step read, and the pad per 16 on
// every first-step write, 14.8 M conflict cycles per configs[4] trace LDE).
// L = log2 of the tile's row count (the kernel's maximum; a smaller tile only uses fewer rows).
XFG_HD constexpr int row_pitch(int S, int P = 4, int L = 4) {
    return P == 4 ? S + S / 16 + 1 : S + (S >> P) + ((L >= 4 || L <= 0) ? 1 : (16 >> L));
}
// Pitch of a 32-bit exchange tile (pass_dft_split). Its writes and ds_read_b32 / ds_read2_b32 reads
// bank on (a / 4) mod 32 per 32-lane half, where a row-fast half-wave spans 2^L rows of the tile and
// 32 / 2^L consecutive groups, so a row pitch of 32 / 2^L (mod 32) spreads the rows over distinct bank
// groups. Radix 32 (P = 5): S + S / 32 + 32 / 2^L (the 64-bit pitch, 2 mod 32 at 8 rows, was 2-way
// conflicted on pass A's first-step writes and both passes' second-step reads: 22 M conflict cycles
// per configs[4] trace LDE). Radix 16 keeps row_pitch.
XFG_HD constexpr int split_pitch(int S, int P, int L) {
    return P == 5 ? S + (S >> 5) + ((32 >> L) & 31) : row_pitch(S, P, L);
}

// ---------------------------------------------------------------- LDS layout of a pass block
// Offsets in 8-byte words from the start of dynamic LDS; the tile is always at 0. `tw` is the pass's
// twiddle table (ltw, or the per-coset [r][k] table comb), `pre` the coset pre-factors behind it (pre,
// or ntt_pass_a_r1024's pre2). The host launches with `bytes`.
struct LdsLayout {
    int tw, pre, bytes;
};
XFG_HD constexpr int min_int(int a, int b) { return a < b ? a : b; }
// ntt_pass_a<LOGR, *, LOGT, LOGE>, ntt_pass_a_cos, ntt_pass_a_cos2: 64-bit tile of 2^logTC columns
// (logTC = min(logC, LOGT + LOGE - LOGR)), w_R [R], pre-factors [R] unless they are read from L2 (preg)
XFG_HD constexpr LdsLayout lds_pass_a(int logR, int logT, int logE, int logC, bool preg) {
    const int full = logT + logE - logR, R = 1 << logR;
    const int tile = (1 << min_int(logC, full)) * row_pitch(R, logE, full);
    return {tile, tile + R, (tile + (preg ? 1 : 2) * R) * 8};
}
// ntt_pass_b<LOGC, *, LOGT, LOGE>, ntt_pass_b_pers: 64-bit tile of 2^min(logR, LOGT + LOGE - LOGC) rows, w_C [C]
XFG_HD constexpr LdsLayout lds_pass_b(int logC, int logT, int logE, int logR) {
    const int full = logT + logE - logC, C = 1 << logC;
    const int tile = (1 << min_int(logR, full)) * row_pitch(C, logE, full);
    return {tile, tile + C, (tile + C) * 8};
}
// ntt_pass_b_tq: the same tile in 32-bit halves (pass_dft_split), [r][k] twiddles [C]. Here alone tw and
// pre count 4-byte words: the tile of a single row has an odd number of them.
XFG_HD constexpr LdsLayout lds_pass_b_tq(int logC, int logT, int logE, int logR) {
    const int full = logT + logE - logC, C = 1 << logC;
    const int tile = (1 << min_int(logR, full)) * row_pitch(C, logE, full);
    return {tile, tile + 2 * C, tile * 4 + C * 8};
}
// ntt_pass_a_r1024 / ntt_pass_b_r1024: 8 x 1024 tile in 32-bit halves, rounded up to 8 bytes; pass A:
// comb [1024], pre2 [32][8]; pass B: w_C [1024]
XFG_HD constexpr LdsLayout lds_r1024(bool pass_b) {
    const int tile = (8 * split_pitch(1024, 5, 3) + 1) / 2;
    return {tile, tile + 1024, (tile + 1024 + (pass_b ? 0 : 256)) * 8};
}

// ---------------------------------------------------------------- pass tables
// One contiguous block per (size, direction, blowup), alone or behind a four-step table:
//   wR() w_R^(+-i) [R], wC() w_C^(+-i) [C]; the inverse tables (logbeta = -1) end here
//   pre(t)        coset pre-factors 7^(C i) w_(beta R)^(t i)    [beta][R]
// R = 256, beta >= 4 (ntt_pass_a_cos2):
//   comb(t)       [r][k] = w_R^(r k) 7^(C r) w_(beta R)^(t r)    [beta][16][16]
//   cos2_scal()   [c][r] = 7^(16 C r) w_(16 beta)^(c r)          [beta / 4][16]
// R = C = 1024 (ntt_pass_a_r1024):
//   comb(t)       [r][k] = w_1024^(r k) g_t^r                    [beta][32][32]
//   r1024_seed(t) [j2] = 7^j2 w_N^(j2 t)                         [beta][C]
//   r1024_t4()    [k1][j2] = w_n^(j2 k1)                         [R][C]
// The per-coset offsets come in the index's type (the largest block, R = C = 1024 at blowup 16, has 1.1 M
// entries: a kernel may keep them in 32 bits).
struct PassTableLayout {
    int logR, logC, logbeta;
    XFG_HD constexpr bool fwd() const { return logbeta >= 0; }
    XFG_HD constexpr bool has_cos2() const { return logR == 8 && logbeta >= 2; }
    XFG_HD constexpr bool has_r1024() const { return fwd() && logR == 10 && logC == 10; }
    XFG_HD constexpr int R() const { return 1 << logR; }
    XFG_HD constexpr int C() const { return 1 << logC; }
    XFG_HD constexpr int wR() const { return 0; }
    XFG_HD constexpr int wC() const { return R(); }
    template <class T>
    XFG_HD constexpr T pre(T t) const { return (T)R() + (T)C() + t * R(); }
    template <class T>
    XFG_HD constexpr T comb(T t) const { return pre((T)1 << logbeta) + t * R(); }
    XFG_HD constexpr uint64_t cos2_scal() const { return comb(1ULL << logbeta); }
    template <class T>
    XFG_HD constexpr T r1024_seed(T t) const { return comb((T)1 << logbeta) + t * C(); }
    XFG_HD constexpr uint64_t r1024_t4() const { return r1024_seed(1ULL << logbeta); }
    XFG_HD constexpr uint64_t total() const {
        return !fwd()        ? (uint64_t)(R() + C())
               : has_r1024() ? r1024_t4() + ((uint64_t)R() << logC)
               : has_cos2()  ? cos2_scal() + (16ULL << (logbeta - 2))
                             : pre(1ULL << logbeta);
    }
};
XFG_HD constexpr PassTableLayout pass_table_layout(int logn, int logbeta) {
    int logR = 0, logC = 0;
    ntt_split(logn, logR, logC);
    return {logR, logC, logbeta};
}
// entries of the four-step table proper ([t][k1][j2], or [k1][j2] for the inverse, logbeta = -1); the
// pass tables follow it
XFG_HD constexpr uint64_t fourstep_main(int logn, int logbeta) { return 1ULL << (logn + (logbeta > 0 ? logbeta : 0)); }
// entries of the pass tables alone, and of a four-step table with its pass tables
constexpr uint64_t pass_tables_size(int logn, int logbeta) { return pass_table_layout(logn, logbeta).total(); }
constexpr uint64_t fourstep_size(int logn, int logbeta) { return fourstep_main(logn, logbeta) + pass_tables_size(logn, logbeta); }

// ---------------------------------------------------------------- which table a forward LDE uses
// Up to 2^FOURSTEP_MAX_LOG points: the full four-step table (pass tables appended). Past it (configs[4]:
// 2^20 x 16, where a full table would be 128 MB and measured slower): the pass tables alone.
constexpr int FOURSTEP_MAX_LOG = 22;
constexpr int PASS_MAX_LOG = 24;
enum class TableKind { none, fourstep, pass_only };
constexpr TableKind table_kind(int logn, int logbeta) {
    if (logn < 0 || logbeta < 0 || logbeta > 4 || logn > PASS_MAX_LOG) return TableKind::none;
    return logn + logbeta <= FOURSTEP_MAX_LOG ? TableKind::fourstep : TableKind::pass_only;
}

// ---------------------------------------------------------------- the kernels
// Every instantiation ntt.hip may launch, once: X(kernel, symbol, LOGS, INV, LOGT, LOGE) with LOGS the
// pass's DFT size (R for pass A, C for pass B), 2^LOGT threads, 2^LOGE elements per thread.
// (tests/sanitize/ntt_plan.cpp: every plan's keys are here, and every entry here is planned by some shape)
#define XFG_NTT_A(X, S, INV, T, E) X(pass_a, (ntt_pass_a<S, INV, T, E>), S, INV, T, E)
#define XFG_NTT_B(X, S, INV, T, E) X(pass_b, (ntt_pass_b<S, INV, T, E>), S, INV, T, E)
#define XFG_NTT_BOTH(M, X, S, T, E) M(X, S, false, T, E) M(X, S, true, T, E)
#define XFG_NTT_KERNELS(X)                                                                                     \
    XFG_NTT_BOTH(XFG_NTT_A, X, 1, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 2, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 3, 8, 4) \
    XFG_NTT_BOTH(XFG_NTT_A, X, 4, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 5, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 6, 8, 4) \
    XFG_NTT_BOTH(XFG_NTT_A, X, 7, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 8, 8, 4) XFG_NTT_BOTH(XFG_NTT_A, X, 9, 8, 5) \
    XFG_NTT_A(X, 10, false, 8, 5) XFG_NTT_A(X, 10, true, 9, 5)                                                 \
    XFG_NTT_BOTH(XFG_NTT_B, X, 2, 8, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 3, 8, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 4, 8, 4) \
    XFG_NTT_BOTH(XFG_NTT_B, X, 5, 8, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 6, 8, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 7, 8, 4) \
    XFG_NTT_BOTH(XFG_NTT_B, X, 8, 8, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 9, 8, 5) XFG_NTT_BOTH(XFG_NTT_B, X, 10, 8, 5) \
    XFG_NTT_BOTH(XFG_NTT_B, X, 11, 10, 4) XFG_NTT_BOTH(XFG_NTT_B, X, 12, 8, 4)                                 \
    X(pass_a_cos, (ntt_pass_a_cos<8>), 8, false, 8, 4)                                                         \
    X(pass_a_cos2, (ntt_pass_a_cos2), 8, false, 8, 4)                                                          \
    X(pass_a_r1024, (ntt_pass_a_r1024), 10, false, 8, 5)                                                       \
    X(pass_b_r1024, (ntt_pass_b_r1024), 10, false, 8, 5)                                                       \
    X(pass_b_tq, (ntt_pass_b_tq<8, 8, 4>), 8, false, 8, 4)                                                     \
    X(pass_b_pers, (ntt_pass_b_pers<10, 8, 5, 2>), 10, false, 8, 5)

enum class NttKernel : int { pass_a, pass_a_cos, pass_a_cos2, pass_a_r1024, pass_b, pass_b_r1024, pass_b_tq, pass_b_pers };
struct NttKey {
    NttKernel kernel;
    int logS, logT, logE;
    bool inv;
    constexpr bool operator==(const NttKey& o) const {
        return kernel == o.kernel && logS == o.logS && logT == o.logT && logE == o.logE && inv == o.inv;
    }
};
struct NttPass {
    NttKey key;
    unsigned gx, gy, block;
    size_t lds;
};
struct NttPlan {
    bool ok;  // false: no kernel for this shape, nothing may be launched
    int logR, logC;
    NttPass a, b;
    int xcd, tq_b, preg;  // NttArgs flags
    int ntx, ntiles;      // ntt_pass_b_pers: row tiles per (poly, coset), tiles in all
};

// Pass shapes (the alternatives named there measured slower):
// * radix-32 steps (32 elements per thread) for pass sizes 2^9 and 2^10: 16 x 32 and 32 x 32 instead of
//   2 x 16 x 16 and 4 x 16 x 16, one general-twiddle step fewer. Pass A then takes 16 columns per tile
//   (2^(logR - 1) threads), except the forward R = 1024 pass with pass tables: 256 threads x 8 columns,
//   coset pre-factors read from L2 (preg: 76 KiB of LDS, two blocks per CU). Pass B: 256 threads, 8192
//   elements, two blocks per CU.
// * C = 2048 runs 1024-thread radix-16 tiles (16384 elements) so that a tile holds 8 rows.
// * everything else: 256 threads x 16 elements.
// has_t4 / has_pt: the four-step table / the pass tables exist (has_t4 implies has_pt); cus: compute
// units, for the persistent pass B's grid.
constexpr NttPlan ntt_plan(int logn, int logbeta, bool inverse, int npoly, bool has_t4, bool has_pt, int cus) {
    NttPlan p{};
    if (logn < 1 || logn > 30 || npoly < 1 || (!inverse && (logbeta < 0 || logbeta > 4 || !has_pt))) return p;
    ntt_split(logn, p.logR, p.logC);
    const int logR = p.logR, logC = p.logC, R = 1 << logR, C = 1 << logC;
    const int eA = (logR >= 9 && logR <= 10 && logC >= 4) ? 5 : 4;
    const int eB = (logC >= 9 && logC <= 10 && logR >= 3) ? 5 : 4;
    p.preg = (!inverse && has_pt && eA == 5 && logR == 10) ? 1 : 0;
    const int ltA = eA == 5 ? (p.preg ? 8 : logR - 1) : 8;
    const int ltB = (eB == 4 && logC == 11 && logR >= 4) ? 10 : 8;
    if (ltA + eA < logR || ltB + eB < logC) return p;  // a tile would not hold one column / row
    const int logTC = min_int(logC, ltA + eA - logR), logTR = min_int(logR, ltB + eB - logC);
    const unsigned ncos = inverse ? 1u : (1u << logbeta), planes = (unsigned)npoly * ncos;
    // XCD-contiguous block order where a tile row of the scattered writes is narrower than a 128 B
    // line: pass A stores 2^logTC consecutive words per row, pass B 2^logTR (xcd_block)
    p.xcd = (logTC < 4 ? 1 : 0) | (logTR < 4 ? 2 : 0) | (p.preg ? 4 : 0);
    p.a = {{NttKernel::pass_a, logR, ltA, eA, inverse}, (unsigned)(C >> logTC), planes, 1u << ltA,
           (size_t)lds_pass_a(logR, ltA, eA, logC, p.preg).bytes};
    p.b = {{NttKernel::pass_b, logC, ltB, eB, inverse}, (unsigned)(R >> logTR), planes, 1u << ltB,
           (size_t)lds_pass_b(logC, ltB, eB, logR).bytes};
    if (!inverse && !has_t4 && logR == 10 && logC == 10) {
        // past the four-step tables at n = 2^20 (configs[4]): the dedicated R = C = 1024 passes
        p.a = {{NttKernel::pass_a_r1024, 10, 8, 5, false}, (unsigned)(C >> 3), planes, 256, (size_t)lds_r1024(false).bytes};
        p.b = {{NttKernel::pass_b_r1024, 10, 8, 5, false}, (unsigned)(R >> 3), planes, 256, (size_t)lds_r1024(true).bytes};
    } else if (!inverse) {
        // pass A: all cosets of a column tile in one block where the four-step table exists (R = 256):
        // ntt_pass_a_cos2 for beta >= 4, ntt_pass_a_cos at beta = 2; pass B then applies the four-step
        // twiddles as it loads (tq_b). Only for launch sets of >= 512 such blocks (two per CU): a smaller
        // set leaves CUs idle while each block walks its beta cosets, and one block per (tile, poly, coset)
        // finishes sooner (2^16 x 8: 28 polynomials 110 against 107 us, 32 polynomials 119 against 122;
        // profiles/r06/lde_small.txt)
        if (has_t4 && logR == 8 && (uint64_t)npoly * (C >> logTC) >= 512) {
            p.tq_b = 1;
            p.a.key.kernel = logbeta >= 2 ? NttKernel::pass_a_cos2 : NttKernel::pass_a_cos;
            p.a.gy = (unsigned)npoly;
        }
        if (logC == 10 && eB == 5 && !p.tq_b) {
            // past the four-step tables: persistent pass B (prefetches the next tile during this one)
            p.ntx = R >> logTR;
            p.ntiles = p.ntx * (int)planes;
            const int want = (2 * cus < p.ntiles ? 2 * cus : p.ntiles) & ~7;
            p.b.key.kernel = NttKernel::pass_b_pers;
            p.b.gx = (unsigned)(want > 8 ? want : 8);
            p.b.gy = 1;
        } else if (logC == 8 && p.tq_b) {
            // the tabled LDE's pass B with the 32-bit split exchange (pass_dft_split): 19.5 instead of 37 KiB
            // of LDS per block, 6 instead of 4 waves per SIMD (919-942 vs 946-961 us per 64-proof launch set)
            p.b.key.kernel = NttKernel::pass_b_tq;
            p.b.lds = (size_t)lds_pass_b_tq(logC, ltB, eB, logR).bytes;
        }
    }
    // a pass of size 1 does not exist, nor any kernel that XFG_NTT_KERNELS does not list
    bool fa = false, fb = false;
#define XFG_NTT_FIND(K, SYM, S, INV, T, E)                           \
    fa = fa || p.a.key == NttKey{NttKernel::K, S, T, E, INV};         \
    fb = fb || p.b.key == NttKey{NttKernel::K, S, T, E, INV};
    XFG_NTT_KERNELS(XFG_NTT_FIND)
#undef XFG_NTT_FIND
    p.ok = fa && fb;
    return p;
}

// whether a size has kernels at all (with the tables ensure_fourstep builds for it; any launch-set size)
constexpr bool ntt_supported(int logn, int logbeta, bool inverse) {
    const TableKind k = table_kind(logn, logbeta);
    const bool t4 = inverse ? (logn >= 3 && logn <= FOURSTEP_MAX_LOG) : k == TableKind::fourstep;
    return ntt_plan(logn, logbeta, inverse, 1, t4, inverse ? t4 : k != TableKind::none, 256).ok;
}

// ---------------------------------------------------------------- blowup 32, 64, 128: composed LDEs
// A blowup beta > 16 is g = beta / 16 blowup-16 transforms. With N = beta n and w_(16 n) = w_N^g, the
// blowup-16 LDE of the twisted coefficients c_j w_N^(u j) evaluates P at 7 w_N^(u + g (t' + 16 m)): its coset
// t' is the natural coset t = u + g t' of the blowup-beta LDE (lde_coset). Sub-transform u therefore writes
// its 16 planes g n words apart starting at plane u (NttArgs::out_plane), which leaves the output in the
// same coset-major layout [poly][t][m], t < beta, that every consumer of a direct LDE reads.
// Scratch (words, from the start of the caller's buffer): the pass intermediate of one sub-transform
// [npoly][16][n], shared by the g of them, then the twisted coefficients of u = 1 .. g - 1 [g - 1][npoly][n]
// (u = 0 reads the caller's coefficients); (15 + g) npoly n words in all, within the beta npoly n every
// caller sizes its LDE scratch to.
constexpr int LDE_DIRECT_MAX_LOGBETA = 4, LDE_MAX_LOGBETA = 7;
constexpr int LDE_COMPOSED_MAX_LOG = 24;  // log2 of the largest composed LDE (the largest LDE of any kind)
struct LdePlan {
    bool ok;              // false: nothing may be launched
    int sub_logbeta;      // log2 blowup of each sub-transform
    int groups;           // g sub-transforms (1: the direct LDE, nothing is twisted)
    uint64_t out_plane;   // words between a sub-transform's consecutive output planes: g n
    uint64_t twist_off;   // first word of the twisted coefficients in the scratch buffer
    uint64_t scratch_words;
};
constexpr LdePlan lde_plan(int logn, int logbeta, int npoly) {
    LdePlan p{};
    if (logn < 1 || logn > 30 || logbeta < 0 || npoly < 1) return p;
    const uint64_t n = 1ULL << logn, np = (uint64_t)npoly;
    if (logbeta <= LDE_DIRECT_MAX_LOGBETA) return {true, logbeta, 1, n, np << (logn + logbeta), np << (logn + logbeta)};
    if (logbeta > LDE_MAX_LOGBETA || logn + logbeta > LDE_COMPOSED_MAX_LOG) return p;
    if (!ntt_supported(logn, LDE_DIRECT_MAX_LOGBETA, false)) return p;
    const int g = 1 << (logbeta - LDE_DIRECT_MAX_LOGBETA);
    const uint64_t y = np << (logn + LDE_DIRECT_MAX_LOGBETA);
    return {true, LDE_DIRECT_MAX_LOGBETA, g, (uint64_t)g << logn, y, y + (uint64_t)(g - 1) * np * n};
}
// log2 blowup of the tables a forward LDE runs on (those of its sub-transforms)
constexpr int lde_table_logbeta(int logbeta) { return logbeta > LDE_DIRECT_MAX_LOGBETA ? LDE_DIRECT_MAX_LOGBETA : logbeta; }
// natural coset of plane t' of sub-transform u
constexpr int lde_coset(const LdePlan& p, int u, int tsub) { return u + p.groups * tsub; }
// whether a forward LDE of this shape can run at all (direct or composed)
constexpr bool lde_supported(int logn, int logbeta) {
    return logbeta <= LDE_DIRECT_MAX_LOGBETA ? ntt_supported(logn, logbeta, false) : lde_plan(logn, logbeta, 1).ok;
}

}  // namespace xfg
