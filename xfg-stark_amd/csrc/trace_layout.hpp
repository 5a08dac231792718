// Where the cells of a batch of caller-supplied traces lie (xfg_trace_layout), and what the host does with a
// layout: the overflow-checked extent, the dense test, the canonicity key of a host trace read through the
// strides, and the gather of one host trace into the dense [7][n] of the lanes' staging. The keys of the
// trace check are defined here too, for the host and the kernels alike (kernels.hpp includes this header).
// Pure functions, no HIP (tests/sanitize/trace_layout.cpp compiles this header with a plain host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define XFG_HD __host__ __device__
#else
#define XFG_HD
#endif

namespace xfg {

// ---- the trace check's word: kind << 62 | step << 3 | index, so that the order of the keys is the order of
// the report (kernels.hpp, launch_trace_check); all ones when the trace violates nothing
constexpr uint64_t TRACE_KEY_VALID = ~0ULL;
enum : unsigned { TRACE_KEY_NONCANONICAL = 0, TRACE_KEY_ASSERTION = 1, TRACE_KEY_TRANSITION = 2 };
XFG_HD constexpr uint64_t trace_key(unsigned kind, uint64_t step, unsigned index) {
    return ((uint64_t)kind << 62) | (step << 3) | index;
}
constexpr uint64_t TRACE_FIELD_P = 0xFFFFFFFF00000001ULL;  // the Goldilocks prime (gl.hpp P)

// cell (trace i, column c, step s) of a batch lies at word i * trace_stride + c * col_stride + s * row_stride.
// Any values: 0 is a broadcast, cells may overlap (they are only read)
struct TraceLayout {
    uint64_t trace_stride, col_stride, row_stride;
    XFG_HD constexpr uint64_t at(uint64_t i, uint64_t c, uint64_t s) const {
        return i * trace_stride + c * col_stride + s * row_stride;
    }
};
constexpr TraceLayout dense_layout(uint64_t n) { return TraceLayout{7 * n, n, 1}; }
constexpr bool is_dense(const TraceLayout& L, uint64_t n) {
    return L.trace_stride == 7 * n && L.col_stride == n && L.row_stride == 1;
}

// the words from the first cell to the last one of `count` traces of n steps, both included:
// (count - 1) trace_stride + 6 col_stride + (n - 1) row_stride + 1. False when count or n is 0, when a
// product or the sum overflows 64 bits, or when the extent is above TRACE_EXTENT_MAX (2^58 words: byte
// offsets then fit 61 bits)
constexpr uint64_t TRACE_EXTENT_MAX = 1ULL << 58;
inline bool trace_extent(const TraceLayout& L, uint64_t count, uint64_t n, uint64_t* extent) {
    if (count == 0 || n == 0) return false;
    uint64_t a = 0, b = 0, c = 0, sum = 1;
    if (__builtin_mul_overflow(count - 1, L.trace_stride, &a) || __builtin_mul_overflow((uint64_t)6, L.col_stride, &b) ||
        __builtin_mul_overflow(n - 1, L.row_stride, &c))
        return false;
    if (__builtin_add_overflow(sum, a, &sum) || __builtin_add_overflow(sum, b, &sum) || __builtin_add_overflow(sum, c, &sum))
        return false;
    if (sum > TRACE_EXTENT_MAX) return false;
    *extent = sum;
    return true;
}

// the key of the first cell >= p of one host trace (tr: its cell (0, 0)) in the check kernel's order, step
// then column; TRACE_KEY_VALID when every cell is canonical. Whole columns are scanned one after the other when
// their cells are neighbours (the smallest key over the columns' first offenders), rows otherwise: the same key
inline uint64_t host_noncanonical_key(const uint64_t* tr, const TraceLayout& L, uint64_t n) {
    uint64_t key = TRACE_KEY_VALID;
    if (L.row_stride == 1) {
        for (unsigned c = 0; c < 7; c++) {
            const uint64_t* col = tr + c * L.col_stride;
            for (uint64_t s = 0; s < n; s++)
                if (col[s] >= TRACE_FIELD_P) {
                    const uint64_t k = trace_key(TRACE_KEY_NONCANONICAL, s, c);
                    key = k < key ? k : key;
                    break;
                }
        }
        return key;
    }
    for (uint64_t s = 0; s < n; s++)
        for (unsigned c = 0; c < 7; c++)
            if (tr[L.at(0, c, s)] >= TRACE_FIELD_P) return trace_key(TRACE_KEY_NONCANONICAL, s, c);
    return key;
}

// one host trace (tr: its cell (0, 0)) into the dense dst [7][n]
inline void gather_trace(const uint64_t* tr, const TraceLayout& L, uint64_t n, uint64_t* dst) {
    if (L.row_stride == 1) {  // whole columns: of the dense layout, the trace's 7 n words as they lie
        for (unsigned c = 0; c < 7; c++) memcpy(dst + c * n, tr + c * L.col_stride, n * 8);
        return;
    }
    for (uint64_t s = 0; s < n; s++) {  // row by row: a row's cells are neighbours in the usual sources
        const uint64_t* row = tr + s * L.row_stride;
        for (unsigned c = 0; c < 7; c++) dst[c * n + s] = row[c * L.col_stride];
    }
}

}  // namespace xfg
