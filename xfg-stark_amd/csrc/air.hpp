// XfgBurnMintAir on one row (reference src/burn_mint_air.rs:335-395): the seven transition constraints, the
// values asserted at step 0, which columns each constraint reads, and the split of the constraint sums of a
// proof whose trace has constant columns into the part that is the same at every point and the rest.
// Nothing else knows the constraints. Host-compilable (tests/sanitize/leaf_prefix.cpp).
#pragma once
#include "gl.hpp"

namespace xfg {

// per-proof AIR constants (reference src/burn_mint_air.rs:54-71 order + Keccak constants)
struct AirConst {
    u64 pub[12];
    u64 nullifier;
    u64 commitment;
    u64 pad[2];
};

constexpr u64 AIR_LAST_STATE = 3;  // the value asserted on column 4 at step n - 1

// transition constraint K of XfgBurnMintAir::evaluate_transition on one row: cur = the row's seven cells,
// nxt4 = column 4 of the next row (the only neighbour the AIR reads)
template <int K>
__host__ __device__ __forceinline__ u64 air_constraint(const AirConst& A, const u64 (&cur)[7], u64 nxt4) {
    static_assert(K >= 0 && K < 7, "seven transition constraints");
    if constexpr (K == 0) {
        const u64 std_burn = 8000000ULL, large_burn = 8000000000ULL;
        return gl_mul(gl_sub(cur[0], std_burn), gl_sub(cur[0], large_burn));
    } else if constexpr (K == 1) {
        return gl_sub(cur[1], cur[0]);
    } else if constexpr (K == 2) {
        return gl_sub(cur[2], A.pub[2] & 0xFFFFFFFFULL);
    } else if constexpr (K == 3) {
        return gl_sub(cur[3], A.pub[3] & 0xFFFFFFFFULL);
    } else if constexpr (K == 4) {
        const u64 d = gl_sub(nxt4, cur[4]);
        return gl_mul(d, gl_sub(d, 1));
    } else if constexpr (K == 5) {
        return gl_sub(cur[5], A.nullifier);
    } else {
        return gl_sub(cur[6], A.commitment);
    }
}
// the columns constraint k reads: bit c = column c of the current row, bit 8 + c = column c of the next row
__host__ __device__ constexpr unsigned air_constraint_reads(int k) {
    constexpr unsigned READS[7] = {0x01, 0x03, 0x04, 0x08, 0x10 | (0x10 << 8), 0x20, 0x40};
    return READS[k];
}
// all seven. Shared by the constraint evaluator (rows of the LDE) and the trace check (rows of the trace itself)
__host__ __device__ __forceinline__ void air_transition(const AirConst& A, const u64 (&cur)[7], u64 nxt4, u64 (&r)[7]) {
    r[0] = air_constraint<0>(A, cur, nxt4);
    r[1] = air_constraint<1>(A, cur, nxt4);
    r[2] = air_constraint<2>(A, cur, nxt4);
    r[3] = air_constraint<3>(A, cur, nxt4);
    r[4] = air_constraint<4>(A, cur, nxt4);
    r[5] = air_constraint<5>(A, cur, nxt4);
    r[6] = air_constraint<6>(A, cur, nxt4);
}
// the values asserted at step 0 on columns 0..6 (src/burn_mint_air.rs:380-395); the eighth assertion is
// column 4 == AIR_LAST_STATE at step n - 1
__host__ __device__ __forceinline__ void air_step0_values(const AirConst& A, u64 (&v0)[7]) {
    v0[0] = A.pub[0]; v0[1] = A.pub[1]; v0[2] = A.pub[2]; v0[3] = A.pub[3];
    v0[4] = 0; v0[5] = A.nullifier; v0[6] = A.commitment;
}

// ---- row generators: (AirConst, logn, row) -> the seven cells of that row of a proof's trace. The kernels that
// classify the columns of a generated trace and write it (trace_probe_kernel, trace_gen_kernel) are templates
// over one and learn nothing about its columns but the values it returns.
// The burn proof's execution trace (src/burn_mint_air.rs:442-476): the step-0 values in every row, and the
// state column = floor(4 step / n)
struct BurnRowGen {
    __host__ __device__ __forceinline__ void operator()(const AirConst& A, int logn, u64 row, u64 (&r)[7]) const {
        air_step0_values(A, r);
        r[4] = (4 * row) >> logn;
    }
};
// a synthetic trace for xfg_debug_trace_probe, one pattern per column. v = the proof's pub[c], f(row) = 3 row + c:
// 0 v, 1 f (every proof the same, not constant), 2 f + v, 3 v but v + 1 at row[c], 4 f but f + 1 at row[c] of the
// proof whose pub[7] is `proof`
struct SynthRowGen {
    u32 kind[7];
    u64 row[7], proof;
    __host__ __device__ __forceinline__ void operator()(const AirConst& A, int, u64 i, u64 (&r)[7]) const {
        for (int c = 0; c < 7; c++) {
            const u64 v = A.pub[c], f = 3 * i + c, hit = i == row[c] ? 1 : 0;
            const u32 k = kind[c];
            r[c] = k == 0 ? v : k == 1 ? f : k == 2 ? f + v : k == 3 ? v + hit : f + (A.pub[7] == proof ? hit : 0);
        }
    }
};

// ---- the constraint sums of a proof with constant trace columns (bit c of const_mask: column c holds one
// value v[c] in every row, hence at every point of its LDE). Constraint k is the same at every point when
// every column it reads is constant, and so is the assertion term co[7 + c] (T_c(x) - v0_c) of a constant
// column c, and the last-step term of column 4 when column 4 is. Those terms are summed once per proof
// (ce_uniform_of); a point adds the terms left (ce_live_sums). Every field addition returns the canonical
// value, so the split changes no bit of a sum.
__host__ __device__ constexpr unsigned air_uniform_constraints(unsigned const_mask) {
    unsigned u = 0;
    for (int k = 0; k < 7; k++) {
        const unsigned reads = air_constraint_reads(k), cols = (reads | (reads >> 8)) & 0x7Fu;
        if ((cols & ~const_mask) == 0) u |= 1u << k;
    }
    return u;
}
// one proof's uniform part, coordinates of E (the second is 0 in the base field). tr_live: the constraints
// left to the points; as_live: the columns whose step-0 assertion term is (bit 4: and the last-step term)
struct CeUniform {
    u64 tr[2], b0[2], b1[2];
    unsigned tr_live, as_live;
};
// co: the proof's 15 composition coefficients [15][D]; v[c]: the value of constant column c (others unread)
template <int D, int K = 0>
__host__ __device__ __forceinline__ void ce_add_constraints(FE<D>& tr, unsigned which, const u64* co, const AirConst& A,
                                                            const u64 (&cur)[7], u64 nxt4) {
    if constexpr (K < 7) {
        if ((which >> K) & 1) tr = fe_add(tr, fe_mulb(FE<D>::load(co + K * D), air_constraint<K>(A, cur, nxt4)));
        ce_add_constraints<D, K + 1>(tr, which, co, A, cur, nxt4);
    }
}
template <int D>
__host__ __device__ __forceinline__ void ce_add_assertions(FE<D>& b0, unsigned which, const u64* co, const AirConst& A,
                                                           const u64 (&cur)[7]) {
    u64 v0[7];
    air_step0_values(A, v0);
#pragma unroll
    for (int c = 0; c < 7; c++)
        if ((which >> c) & 1) b0 = fe_add(b0, fe_mulb(FE<D>::load(co + (7 + c) * D), gl_sub(cur[c], v0[c])));
}
template <int D>
__host__ __device__ __forceinline__ FE<D> ce_last_step_term(const u64* co, u64 cur4) {
    return fe_mulb(FE<D>::load(co + 14 * D), gl_sub(cur4, AIR_LAST_STATE));
}
template <int D>
__host__ __device__ inline CeUniform ce_uniform_of(const AirConst& A, const u64* co, unsigned const_mask, const u64 (&v)[7]) {
    const unsigned cm = const_mask & 0x7Fu, ut = air_uniform_constraints(cm);
    u64 cur[7];
    for (int c = 0; c < 7; c++) cur[c] = (cm >> c) & 1 ? v[c] : 0;
    FE<D> tr = FE<D>::zero(), b0 = FE<D>::zero(), b1 = FE<D>::zero();
    ce_add_constraints<D>(tr, ut, co, A, cur, cur[4]);  // a constant column 4: the next row's cell is v[4] too
    ce_add_assertions<D>(b0, cm, co, A, cur);
    if ((cm >> 4) & 1) b1 = ce_last_step_term<D>(co, cur[4]);
    CeUniform U = {};
    U.tr[0] = tr.c(0); U.b0[0] = b0.c(0); U.b1[0] = b1.c(0);
    if constexpr (D == 2) { U.tr[1] = tr.c(1); U.b0[1] = b0.c(1); U.b1[1] = b1.c(1); }
    U.tr_live = 0x7Fu & ~ut;
    U.as_live = 0x7Fu & ~cm;
    return U;
}
// a point's three sums from the proof's uniform part: cur[c] of a constant column is its value
template <int D>
__host__ __device__ __forceinline__ void ce_live_sums(const CeUniform& U, unsigned tr_live, unsigned as_live, const u64* co,
                                                      const AirConst& A, const u64 (&cur)[7], u64 nxt4, FE<D>& tr,
                                                      FE<D>& b0, FE<D>& b1) {
    tr = FE<D>::load(U.tr);
    b0 = FE<D>::load(U.b0);
    b1 = FE<D>::load(U.b1);
    ce_add_constraints<D>(tr, tr_live, co, A, cur, nxt4);
    ce_add_assertions<D>(b0, as_live, co, A, cur);
    if ((as_live >> 4) & 1) b1 = ce_last_step_term<D>(co, cur[4]);
}

}  // namespace xfg
