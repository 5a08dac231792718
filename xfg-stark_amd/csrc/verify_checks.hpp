// The verification plan's records and the checks both of its executors run, host and device: the
// kernels of verify_kernels.hip and the serial loop of verifier.cpp (verify_queries_host). No HIP
// runtime calls, no std containers. `blob` is one proof's bytes on the host and all planned proofs'
// bytes end to end on the device; every offset in a record is a blob offset (verifier.cpp plan_proof).
#pragma once
#include "blake3.hpp"
#include "gl.hpp"

namespace xfg {

// FRI layers: N <= 2^25 folded by two down to a last layer of at least 8 is 22
constexpr int VMAXL = 24;
// flags[proof] (64 bits): 0..23 FRI layer l folding, 32..55 FRI layer l commitment,
// 61 constraint commitment, 62 trace commitment, 63 remainder folding
constexpr u64 VF_TRACE = 1ULL << 62, VF_CONSTRAINT = 1ULL << 61, VF_REMAINDER = 1ULL << 63;
constexpr int VF_LAYER_COMMIT = 32;
struct VTree {
    u64 root_off;           // blob offset of the commitment the root must equal
    uint32_t leaf0, nidx;   // opened leaves: tleaves[leaf0 .. leaf0 + nidx), sorted by index
    uint32_t vec0, nvec;    // node vectors: vecs[vec0 .. vec0 + nvec), in the proof's order
    uint32_t words, depth;  // u64 words per leaf (1, 2, 4, 7, 8, 16 or 32); log2 leaves
    uint32_t proof, pad;
    u64 bit;                // on failure: flags[proof] |= bit
};
struct VTreeLeaf {
    u64 index;    // leaf index
    u64 row_off;  // blob offset of the opened row
};
struct VVec {
    u64 off;  // blob offset of the vector's first digest
    uint32_t cnt, pad;
};
struct VFieldProof {
    E2 z, zg, hz, gam, dc[7], ood[14];
    E2 falpha[VMAXL];
    u64 rem_off;
    uint32_t rem_len, nl, de, logN;  // nl: the planned layers (all of them unless the structure breaks)
};
struct VFieldQuery {
    uint32_t proof, pad;
    u64 pos, trace_off, cons_off;
    u64 row_off[VMAXL];  // layer l: blob offset of the opened row of `fold` E values
};

// proof bytes are not 8-aligned inside the blob: assemble words from bytes
__host__ __device__ __forceinline__ u64 ld_u64(const uint8_t* p) {
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) v |= (u64)p[i] << (8 * i);
    return v;
}
__host__ __device__ __forceinline__ E2 ld_e(const uint8_t* p, int de) {
    return de == 2 ? E2{ld_u64(p), ld_u64(p + 8)} : E2{ld_u64(p), 0};
}
__host__ __device__ __forceinline__ Digest ld_digest(const uint8_t* p) {
    Digest d;
#pragma unroll
    for (int w = 0; w < 8; w++)
        d.w[w] = (uint32_t)p[4 * w] | ((uint32_t)p[4 * w + 1] << 8) | ((uint32_t)p[4 * w + 2] << 16) |
                 ((uint32_t)p[4 * w + 3] << 24);
    return d;
}

template <int K>
__host__ __device__ __forceinline__ Digest hash_words(const uint8_t* p) {
    u64 v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ld_u64(p + 8 * k);
    return b3_hash_elems<K>(v);
}
// leaf of an opened row of `words` elements (static, not inline: with the inline hint vtree_kernel
// comes out with other register counts)
static __host__ __device__ Digest hash_row(const uint8_t* p, uint32_t words) {
    switch (words) {  // trace row 7, constraint value 1 / 2, FRI row 2, 4, 8, 16 or 32 (fold x extension degree)
        case 1: return hash_words<1>(p);
        case 2: return hash_words<2>(p);
        case 4: return hash_words<4>(p);
        case 7: return hash_words<7>(p);
        case 8: return hash_words<8>(p);
        case 16: return hash_words<16>(p);
        default: return hash_words<32>(p);
    }
}

// FRI apply_drp of one row of F = 2^LOGF values (domain offset 7): interpolate them on the coset
// x * <w_F> (the size-F inverse DFT scaled by 1 / F, per coordinate: base-field weights) and evaluate
// at alpha
template <int LOGF>
__host__ __device__ E2 fold_row(const E2* v, u64 x, E2 alpha) {
    constexpr int F = 1 << LOGF;
    const u64 winv = gl_inv(gl_root(LOGF)), invf = gl_inv((u64)F);
    E2 c[F];
    for (int k = 0; k < F; k++) {
        E2 s{0, 0};
        u64 wk = gl_pow(winv, (u64)k), p = 1;
        for (int j = 0; j < F; j++) {
            s = e2_add(s, e2_mulb(v[j], p));
            p = gl_mul(p, wk);
        }
        c[k] = e2_mulb(s, invf);
    }
    const E2 t = e2_mulb(alpha, gl_inv(x));
    E2 r{0, 0};
    for (int k = F - 1; k >= 0; k--) r = e2_add(e2_mul(r, t), c[k]);
    return r;
}

// One query of one proof: the DEEP value at the query point, then every planned FRI layer's opened
// value against the running fold, then the remainder polynomial. Returns the failed checks as flag
// bits (bit l: layer l folding, VF_REMAINDER: remainder). F = 2^LOGF: the proof's folding factor
template <int LOGF>
__host__ __device__ __forceinline__ u64 query_bits(const uint8_t* blob, const VFieldProof& P, const VFieldQuery& Q) {
    const int de = (int)P.de;
    const u64 N = 1ULL << P.logN;
    E2 x = e2(gl_mul(GEN, gl_pow(gl_root(P.logN), Q.pos)));
    E2 s1{0, 0}, s2{0, 0};
    for (int c = 0; c < 7; c++) {
        const E2 tx = e2(ld_u64(blob + Q.trace_off + 8 * c));
        s1 = e2_add(s1, e2_mul(P.dc[c], e2_sub(tx, P.ood[2 * c])));
        s2 = e2_add(s2, e2_mul(P.dc[c], e2_sub(tx, P.ood[2 * c + 1])));
    }
    const E2 izx = e2_inv(e2_sub(x, P.z)), izgx = e2_inv(e2_sub(x, P.zg));
    E2 ev = e2_add(e2_mul(s1, izx), e2_mul(s2, izgx));
    ev = e2_add(ev, e2_mul(e2_mul(P.gam, e2_sub(ld_e(blob + Q.cons_off, de), P.hz)), izx));
    u64 D = N, p = Q.pos;
    u64 bad = 0;
    constexpr int F = 1 << LOGF;
    for (uint32_t l = 0; l < P.nl; l++) {
        const u64 rows = D / F, i = p & (rows - 1), k = p / rows;
        const uint8_t* row = blob + Q.row_off[l];
        E2 v[F];
        for (int j = 0; j < F; j++) v[j] = ld_e(row + 8 * de * j, de);
        if (!e2_eq(v[k], ev)) bad |= 1ULL << l;
        int logD = 0;
        while ((1ULL << logD) < D) logD++;
        ev = fold_row<LOGF>(v, gl_mul(GEN, gl_pow(gl_root(logD), i)), P.falpha[l]);
        p = i;
        D = rows;
    }
    int logD = 0;
    while ((1ULL << logD) < D) logD++;
    const E2 xr = e2(gl_mul(GEN, gl_pow(gl_root(logD), p)));
    E2 r{0, 0};
    for (uint32_t k = P.rem_len; k-- > 0;) r = e2_add(e2_mul(r, xr), ld_e(blob + P.rem_off + 8 * de * k, de));
    if (!e2_eq(r, ev)) bad |= VF_REMAINDER;
    return bad;
}
// the host's choice of instantiation: logf = log2 of the folding factor, 1..4 (check_options)
inline u64 query_bits(const uint8_t* blob, const VFieldProof& P, const VFieldQuery& Q, unsigned logf) {
    switch (logf) {
        case 1: return query_bits<1>(blob, P, Q);
        case 2: return query_bits<2>(blob, P, Q);
        case 3: return query_bits<3>(blob, P, Q);
        default: return query_bits<4>(blob, P, Q);
    }
}

}  // namespace xfg
