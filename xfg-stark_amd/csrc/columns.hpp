// The classes of a trace's columns (live, constant, shared): the launches that find them (columns.hip) and a
// flagged column as the consumers of the trace's planes read it (ColConst, RowConst). Included by kernels.hpp.
#pragma once
#include "air.hpp"
#include "trace_layout.hpp"

namespace xfg {

// constant columns: flags[col] = COL_CONST where cols[col][0..n) holds one value in every row, else 0
// (flags: ncols bytes, the allocation padded to whole 32-bit words; detection blocks cover
// CONST_DETECT_SPAN rows each).
// period > 0 (a unit of ncols / period traces of `period` columns each, more than one trace): the same
// pass also compares column col >= period with column col % period of trace 0, element for element,
// and flags[col] = COL_SHARED where they are equal and the column is not constant (a constant column
// stays constant); trace 0's columns are never shared. The allocation then holds const_flag_bytes(ncols):
// the pass keeps a second byte per column behind the flags.
// vals (or nullptr): vals[col] = cols[col][0], the value of the column where it is constant
constexpr int CONST_DETECT_SPAN = 1024, CONST_FILL_SPAN = 4096;
constexpr unsigned char COL_CONST = 1, COL_SHARED = 2;
__host__ __device__ constexpr size_t detect_same_off(size_t ncols) { return (ncols + 3) & ~(size_t)3; }
constexpr size_t const_flag_bytes(size_t ncols) { return 2 * detect_same_off(ncols); }
// a flag byte as a class: 0 live, 1 constant, 2 the same as the unit's first trace's column
__host__ __device__ constexpr int col_class(unsigned char f) { return (f & COL_CONST) ? 1 : ((f & COL_SHARED) ? 2 : 0); }
void launch_const_detect(const u64* cols, int ncols, int logn, unsigned char* flags, hipStream_t s, int period = 0,
                         u64* vals = nullptr);
// the same flags and vals for a unit of B generated traces of seven columns (period 7), from the rows as the
// generator returns them and without a trace in memory: what launch_const_detect finds in the trace that
// launch_trace_gen would write dense, byte for byte. synth: the synthetic generator (host; debug), else the burn AIR's
void launch_trace_probe(const AirConst* air, int B, int logn, unsigned char* flags, u64* vals, hipStream_t s,
                        const SynthRowGen* synth = nullptr);
// the generated traces [B][7][n], live columns only: flags [B * 7] are the classified bytes
// (launch_trace_probe), and the plane of a column flagged COL_CONST or COL_SHARED is not written
void launch_trace_gen(const AirConst* air, int B, int logn, const unsigned char* flags, u64* trace, hipStream_t s,
                      const SynthRowGen* synth = nullptr);
// ---- a unit of B traces that lie in the caller's device memory in any layout (trace_layout.hpp): read in
// place, never copied. base is the unit's cell (0, 0, 0); the kernels only read it.
struct StridedRows {
    const u64* base;
    TraceLayout at;
    // rows of one block are one contiguous run of words: the block stages the run in LDS with coalesced loads
    // (the tile form of the two kernels) instead of loading seven cells row_stride words apart per thread
    bool tiled() const { return at.col_stride == 1 && at.row_stride >= 7 && at.row_stride <= INGEST_TILE_MAX_PITCH; }
    static constexpr u64 INGEST_TILE_MAX_PITCH = 16;
};
// One pass over the source for what the copy, launch_trace_check and launch_const_detect produce of a trace
// in the lane's buffer: keys [B] as launch_trace_check leaves them (with_air as there; set by a memset on s
// first), flags [B * 7] and vals [B * 7] as launch_const_detect(period 7) leaves them, both found on the
// canonical values of the cells (a cell >= p counts as its value - p, which is what the check would have put
// into the lane's copy). B <= 65535
void launch_trace_ingest_probe(const StridedRows& src, const AirConst* air, int B, int logn, bool with_air, u64* keys,
                               unsigned char* flags, u64* vals, hipStream_t s);
// the canonical cells of the live columns into trace [B][7][n]; the plane of a column flagged COL_CONST or
// COL_SHARED is not written (flags: the classified bytes of launch_trace_ingest_probe), as by launch_trace_gen
void launch_trace_ingest_write(const StridedRows& src, int B, int logn, const unsigned char* flags, u64* trace,
                               hipStream_t s);
// what the NTTs would have produced for the flagged columns, v = src[col * src_stride]:
// coef[col] = (v, 0, ..., 0) and lde[col][t][m] = v (coset-major planes); coef or lde may be nullptr.
// Outside the prover's chain (its readers take a ColConst): xfg_debug_lde_skip and xfg_debug_interpolate_skip
void launch_const_fill(const unsigned char* flags, const u64* src, u64 src_stride, u64* coef, u64* lde, int ncols,
                       int logn, int logbeta, hipStream_t s);

// The flagged columns as the consumers of the trace's planes take them (the LDE [B][7][beta][n] and the
// coefficients [B][7][n]): neither plane of a flagged column is ever written (launch_trace_lde). Every
// element of a constant column's LDE plane is the column's value; a shared column's planes are those of
// the same column of proof 0, which lie in proof 0's slot of the same buffer.
//   flags  [B * 7] the detection's bytes (COL_CONST, COL_SHARED; device, 4-byte aligned, the allocation
//          padded to whole 32-bit words); nullptr: dense, every plane is read
//   vals   the value of column c of proof b lies at vals[(b * 7 + c) * val_stride]
struct ColConst {
    const unsigned char* flags = nullptr;
    const u64* vals = nullptr;
    u64 val_stride = 0;
};
// one proof's flagged columns in registers: bit c of mask (constant) and v[c] where it is set; bit c of
// shared (never set beside the same bit of mask): the column is read from proof 0's planes
struct RowConst {
    unsigned mask, shared;
    u64 v[7];
    // base[i] of the proof's own planes, or of proof 0's for a shared column: one select between the
    // two bases (both wave-uniform in a kernel that runs a block per proof), not a pointer per column
    __device__ __forceinline__ const u64* plane(int c, const u64* own, const u64* first) const {
        return (shared >> c) & 1 ? first : own;
    }
};
// the seven flag bytes of a proof, o = proof * 7, out of two or three aligned 32-bit loads: byte c = flags[o + c]
__device__ __forceinline__ u64 row_flag_bytes(const unsigned char* flags, u64 o) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(flags) + (o >> 2);
    const unsigned r = (unsigned)(o & 3);
    u64 bytes = ((u64)w[0] | ((u64)w[1] << 32)) >> (8 * r);  // flags o .. o + 7 - r
    if (r >= 2) bytes |= (u64)w[2] << (64 - 8 * r);           // o + 8 - r .. (inside the padded allocation)
    return bytes;
}
// for a proof that is the same in every lane (a block per proof): the seven flags come out of two or
// three aligned 32-bit loads and the values of 64-bit ones at wave-uniform addresses (scalar loads),
// and mask and values are made wave-uniform for the branches that leave the flagged loads out
__device__ __forceinline__ RowConst row_const_uniform(const ColConst& cc, u64 proof) {
    const u64 o = proof * 7;
    const u64 bytes = row_flag_bytes(cc.flags, o);
    RowConst rc;
    rc.mask = rc.shared = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        const unsigned f = (unsigned)(bytes >> (8 * c)) & 0xFF;
        rc.mask |= (f & COL_CONST ? 1u : 0u) << c;
        rc.shared |= ((f & (COL_CONST | COL_SHARED)) == COL_SHARED ? 1u : 0u) << c;
    }
    rc.mask = __builtin_amdgcn_readfirstlane(rc.mask);
    rc.shared = __builtin_amdgcn_readfirstlane(rc.shared);
#pragma unroll
    for (int c = 0; c < 7; c++) {
        rc.v[c] = 0;
        if ((rc.mask >> c) & 1) {
            const u64 v = cc.vals[(o + c) * cc.val_stride];
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
            rc.v[c] = (u64)lo | ((u64)hi << 32);
        }
    }
    return rc;
}
// for a proof that differs from lane to lane (the openings): plain loads. The seven words at vals are
// loaded whatever the flags say (an unflagged column's is its coefficient 0, never used), so that they
// are in flight beside the flags and not behind them: a lone proof waits on this chain
__device__ __forceinline__ RowConst row_const_lane(const ColConst& cc, u64 proof) {
    RowConst rc;
    rc.mask = rc.shared = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        rc.v[c] = cc.vals[(proof * 7 + c) * cc.val_stride];
        const unsigned f = cc.flags[proof * 7 + c];
        rc.mask |= (f & COL_CONST ? 1u : 0u) << c;
        rc.shared |= ((f & (COL_CONST | COL_SHARED)) == COL_SHARED ? 1u : 0u) << c;
    }
    return rc;
}

}  // namespace xfg
