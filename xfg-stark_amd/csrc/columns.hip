// The classes of a trace's columns: finding them, writing the live ones of a generated trace and of a trace that
// lies in the caller's device memory in a strided layout (launches: columns.hpp).
//
// Constant columns: a column that holds one value v in every row interpolates to the constant v, and its
// LDE is v at every point: such columns take no NTT. const_detect_kernel finds them in whatever trace arrives
// (trace_probe_kernel: in the rows of a trace the prover generates itself, as they are generated),
// the NTT kernels return at once for them (NttArgs::skip, ntt.hip). Their coefficient and LDE planes stay
// unwritten in the prover: every reader of either takes the value from a ColConst (columns.hpp);
// const_fill_kernel serves xfg_debug_lde_skip and xfg_debug_interpolate_skip alone.
// There are two detection kernels, not one, because their blocks differ: a block per column of a trace of any
// width that lies in memory, against a block per proof on the seven columns of the rows it generates.
//
// Shared columns: a column of proof b > 0 of a unit that equals the same column of the unit's proof 0
// element for element has proof 0's coefficients and proof 0's LDE: it takes no NTT either, and its
// readers go to proof 0's planes (ColConst). The same detection pass finds them, in whatever traces
// arrive; the representative is proof 0 and nothing more general, so a unit whose first trace differs
// from the others shares nothing. A column that is constant stays constant (cheaper for every reader).
// The pass keeps two bytes per column, both preset to 1 and both only ever overwritten with 0, so that
// every writer of a byte stores the same value and nothing needs an atomic (one byte with two bits,
// cleared by atomic ANDs, measured 127 us per 64-proof unit against 41 for the constancy pass alone and
// 51 for this form, profiles/r15: the blocks of a proof's columns all hit the same one or two words):
// flags[col], the constancy, and same[col] = flags[detect_same_off(ncols) + col]. const_class_kernel
// then folds the second into the first as COL_SHARED
#include "dispatch.hpp"
#include "hip_util.hpp"
#include "kernels.hpp"

namespace xfg {

__global__ void const_flags_init_kernel(unsigned char* flags, int count, int period) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    flags[i] = 1;
    if (period) flags[detect_same_off(count) + i] = i >= period ? 1 : 0;  // trace 0's columns are never shared
}
// flags[col] (preset to 1) -> 0 where some element of cols[col][0..n) differs from element 0 and, SHARE,
// same[col] -> 0 where some element differs from the same element of column col % period (trace 0's; the
// columns below period are trace 0's own and are compared with nothing). One block per
// CONST_DETECT_SPAN rows of a column (min(256, n) threads, coalesced strides); a thread that saw a
// difference stores 0. The pass reads the trace once; trace 0's column (8 n bytes) is read again by
// every other trace's blocks, from the cache.
// vals[col] = element 0 (block 0 of the column; read only where the column turns out constant)
template <bool SHARE>
__global__ __launch_bounds__(256) void const_detect_kernel(const u64* cols, u64 n, unsigned char* flags, int period,
                                                           u64* vals) {
    const int col = blockIdx.y;
    const u64* c = cols + (u64)col * n;
    const u64 first = c[0];
    const u64 i0 = (u64)blockIdx.x * CONST_DETECT_SPAN, i1 = i0 + CONST_DETECT_SPAN < n ? i0 + CONST_DETECT_SPAN : n;
    if (vals && blockIdx.x == 0 && threadIdx.x == 0) vals[col] = first;
    u64 diff = 0;
    if (SHARE && col >= period) {  // block-uniform
        const u64* c0 = cols + (u64)(col % period) * n;
        u64 diff0 = 0;
#pragma unroll 4
        for (u64 i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const u64 x = c[i];
            diff |= x ^ first;
            diff0 |= x ^ c0[i];
        }
        if (diff0) flags[detect_same_off(gridDim.y) + col] = 0;
    } else {
        for (u64 i = i0 + threadIdx.x; i < i1; i += blockDim.x) diff |= c[i] ^ first;
    }
    if (diff) flags[col] = 0;
}
// flags[col]: 1 -> COL_CONST, else COL_SHARED where same[col] is still set, else 0
__global__ void const_class_kernel(unsigned char* flags, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) flags[i] = flags[i] ? COL_CONST : (flags[detect_same_off(count) + i] ? COL_SHARED : 0);
}
// The classification of ncols columns, traces of `period` columns each: preset the two bytes per column, run
// the detection launch detect(grid, block, period) -- ny blocks to each span of CONST_DETECT_SPAN rows -- and
// fold the classes. One trace (ncols <= period) shares nothing and nothing extra is run: detect gets period 0,
// the second byte is neither preset nor read, and without a class kernel the first is already 0 or COL_CONST
template <class Detect>
static void classify(unsigned char* flags, int ncols, int ny, int logn, int period, hipStream_t s, Detect detect) {
    const u64 n = 1ULL << logn;
    if (period <= 0 || ncols <= period) period = 0;
    const dim3 gi((unsigned)((ncols + 255) / 256)), bi(256);
    XFG_LAUNCH(const_flags_init_kernel, gi, bi, 0, s, flags, ncols, period);
    const dim3 g((unsigned)((n + CONST_DETECT_SPAN - 1) / CONST_DETECT_SPAN), ny), b(n < 256 ? (unsigned)n : 256u);
    detect(g, b, period);
    if (period) XFG_LAUNCH(const_class_kernel, gi, bi, 0, s, flags, ncols);
}
void launch_const_detect(const u64* cols, int ncols, int logn, unsigned char* flags, hipStream_t s, int period,
                         u64* vals) {
    classify(flags, ncols, ncols, logn, period, s, [&](dim3 g, dim3 b, int period) {
        with_bool(period != 0, [&](auto SHARE) {
            XFG_LAUNCH(const_detect_kernel<SHARE>, g, b, 0, s, cols, 1ULL << logn, flags, period, vals);
        });
    });
}
// f(gen), gen the row generator of a unit's generated traces: the synthetic one where given (debug), else the burn AIR's
template <class F>
static void with_row_gen(const SynthRowGen* synth, F f) { synth ? f(*synth) : f(BurnRowGen{}); }
// The detection for a unit of generated traces, on the rows as Gen (air.hpp) returns them: the trace is
// not in memory, and the kernel's only loads are the AirConsts. The geometry is const_detect_kernel's with
// the seven columns of a proof in one block: block (x, b) generates its CONST_DETECT_SPAN rows of proof b,
// row 0 of proof b and (period: more than one proof, b > 0) the same rows of proof 0, and ORs the
// differences per column; the two bytes per column, their presets, the stores of 0 and vals are as above.
// What it says about a column is what the values say, never which generator ran
template <class Gen>
__global__ __launch_bounds__(256) void trace_probe_kernel(Gen gen, const AirConst* air, int logn, unsigned char* flags,
                                                          int period, u64* vals) {
    const int b = blockIdx.y;
    const u64 n = 1ULL << logn;
    const AirConst& A = air[b];
    const u64 i0 = (u64)blockIdx.x * CONST_DETECT_SPAN, i1 = i0 + CONST_DETECT_SPAN < n ? i0 + CONST_DETECT_SPAN : n;
    u64 first[7], diff[7] = {}, diff0[7] = {};
    gen(A, logn, 0, first);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int c = 0; c < 7; c++) vals[b * 7 + c] = first[c];
    const bool share = period && b > 0;  // block-uniform
    for (u64 i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        u64 x[7];
        gen(A, logn, i, x);
#pragma unroll
        for (int c = 0; c < 7; c++) diff[c] |= x[c] ^ first[c];
        if (share) {
            u64 y[7];
            gen(air[0], logn, i, y);
#pragma unroll
            for (int c = 0; c < 7; c++) diff0[c] |= x[c] ^ y[c];
        }
    }
    unsigned char* same = flags + detect_same_off((size_t)gridDim.y * 7);
#pragma unroll
    for (int c = 0; c < 7; c++) {
        if (diff[c]) flags[b * 7 + c] = 0;
        if (share && diff0[c]) same[b * 7 + c] = 0;
    }
}
void launch_trace_probe(const AirConst* air, int B, int logn, unsigned char* flags, u64* vals, hipStream_t s,
                        const SynthRowGen* synth) {
    classify(flags, B * 7, B, logn, 7, s, [&](dim3 g, dim3 b, int period) {
        with_row_gen(synth, [&](auto gen) {
            XFG_LAUNCH(trace_probe_kernel<decltype(gen)>, g, b, 0, s, gen, air, logn, flags, period, vals);
        });
    });
}
// One thread per row of a proof's trace, rows as Gen (air.hpp) returns them. Only the live columns are
// stored: the proof's seven classified flags are read once, wave-uniform (the block's proof is blockIdx.y), and
// the plane of a constant or shared column is left as it was -- its readers take a ColConst, not the plane
template <class Gen>
__global__ __launch_bounds__(256) void trace_gen_kernel(Gen gen, const AirConst* air, u64* trace,
                                                        const unsigned char* flags, int logn) {
    const u64 n = 1ULL << logn;
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const int proof = blockIdx.y;
    const u64 bytes = row_flag_bytes(flags, (u64)proof * 7);
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) live |= ((bytes >> (8 * c)) & 0xFF ? 0u : 1u) << c;
    live = __builtin_amdgcn_readfirstlane(live);
    if (s >= n || !live) return;
    u64 r[7];
    gen(air[proof], logn, s, r);
    u64* tr = trace + (u64)proof * 7 * n;
#pragma unroll
    for (int c = 0; c < 7; c++)
        if ((live >> c) & 1) tr[c * n + s] = r[c];
}
void launch_trace_gen(const AirConst* air, int B, int logn, const unsigned char* flags, u64* trace, hipStream_t s,
                      const SynthRowGen* synth) {
    const dim3 g((unsigned)(((1ULL << logn) + 255) / 256), B);
    with_row_gen(synth, [&](auto gen) {
        XFG_LAUNCH(trace_gen_kernel<decltype(gen)>, g, dim3(256), 0, s, gen, air, trace, flags, logn);
    });
}
// ---- traces in the caller's device memory, in any layout (StridedRows, columns.hpp): read where they lie.
// Two launches stand where the copy into c->trace, trace_check_kernel and const_detect_kernel stood.
// Geometry of both: one thread per step, block (x, b) the steps [256 x, 256 x + 256) of proof b, like
// trace_check_kernel. Two load shapes, chosen on the host and block-uniform:
//   TILE = false  each thread loads its cells through the strides: right for every layout, coalesced when
//                 row_stride is 1
//   TILE = true   col_stride 1 and 7 <= row_stride <= 16: the block's rows are one contiguous run of words,
//                 which the block loads with coalesced 8-byte loads (lane i at word i of the run; a base
//                 that is only 8-byte aligned is as good as any) and of which it keeps the seven cells of
//                 every row in LDS, 7 words apart whatever the pitch in memory: the pad words of a padded
//                 row never reach a register that is used. A thread then reads its row with 8-byte LDS
//                 reads; 7 is odd, so the 32 rows of a half wave fall on 32 different bank pairs
//                 ((7 t) mod 32 is a permutation of the 64-bit banks). The run ends at the seventh cell of
//                 the last row it needs, not at that row's pitch: the pad words behind the last row of a
//                 buffer are outside the extent the library has checked.
//                 LDS: (256 + 1) rows x 7 words = 14,392 bytes per block
constexpr int INGEST_BLOCK = 256, INGEST_TILE_WORDS = (INGEST_BLOCK + 1) * 7;
__device__ __forceinline__ u64 canonical_cell(u64 v, unsigned& bad, int c) {
    if (v >= P) {
        bad |= 1u << c;
        v -= P;
    }
    return v;
}
// x = the seven cells of step s of `proof`, canonical, of which the generic form loads the columns of `live`
// alone; returns bit c set where cell c was >= p. NEXT: nxt4 = the canonical cell [4][s + 1] below the last
// step (the tile then holds one row more than the block has steps, except behind the last step), else 0.
// Every thread of the block calls it, the threads past the last step too (they get zeros): the tile form
// has two barriers, the first for the readers of what the tile held before
template <bool TILE, bool NEXT>
__device__ __forceinline__ unsigned ingest_row(const StridedRows& src, u64* tile, int proof, u64 s, u64 n, u64 (&x)[7],
                                               u64& nxt4, unsigned live = 0x7F) {
    u64 nx = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) x[c] = 0;
    if constexpr (TILE) {
        const u64 s0 = (u64)blockIdx.x * INGEST_BLOCK, left = n - s0;  // the grid has no block past the last step
        const unsigned rows = left > INGEST_BLOCK ? INGEST_BLOCK + (NEXT ? 1u : 0u) : (unsigned)left;
        const unsigned rs = (unsigned)src.at.row_stride, len = (rows - 1) * rs + 7;
        const u64* run = src.base + src.at.at((u64)proof, 0, s0);
        // word w of the run is cell k = w mod rs of row r = w / rs; a thread's words are 256 apart
        const unsigned dq = INGEST_BLOCK / rs, dr = INGEST_BLOCK % rs;
        unsigned r = threadIdx.x / rs, k = threadIdx.x % rs;
        __syncthreads();
        for (unsigned w = threadIdx.x; w < len; w += INGEST_BLOCK) {
            if (k < 7) tile[r * 7 + k] = run[w];
            r += dq;
            k += dr;
            if (k >= rs) {
                k -= rs;
                r++;
            }
        }
        __syncthreads();
        if (s < n) {
#pragma unroll
            for (int c = 0; c < 7; c++) x[c] = tile[threadIdx.x * 7 + c];
            if (NEXT && s + 1 < n) nx = tile[(threadIdx.x + 1) * 7 + 4];
        }
    } else if (s < n) {
        const u64* row = src.base + src.at.at((u64)proof, 0, s);
#pragma unroll
        for (int c = 0; c < 7; c++)
            if ((live >> c) & 1) x[c] = row[(u64)c * src.at.col_stride];
        if (NEXT && s + 1 < n) nx = row[4 * src.at.col_stride + src.at.row_stride];
    }
    unsigned bad = 0, unused = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) x[c] = canonical_cell(x[c], bad, c);
    nxt4 = canonical_cell(nx, unused, 0);
    return bad;
}
// One pass over the source. keys[proof]: trace_check_kernel's word, from the same per-row function
// (trace_row_key, kernels.hpp) and the same reduction. flags / same / vals: const_detect_kernel's, on the
// canonical values: the two bytes per column were preset by const_flags_init_kernel, a wave that saw a
// difference in a column stores one 0 to the column's byte (the differences are reduced over the wave
// first), and const_class_kernel folds them (classify). For the shared columns a block of proof b > 0 loads
// the same rows of proof 0 too, from the cache, as const_detect_kernel<true> does
template <bool AIR, bool TILE>
__global__ __launch_bounds__(INGEST_BLOCK) void trace_ingest_probe_kernel(StridedRows src, const AirConst* air, u64* keys,
                                                                          int logn, unsigned char* flags, int period,
                                                                          u64* vals) {
    __shared__ u64 tile[TILE ? INGEST_TILE_WORDS : 1];
    const u64 n = 1ULL << logn;
    const u64 s = (u64)blockIdx.x * INGEST_BLOCK + threadIdx.x;
    const int proof = blockIdx.y;
    u64 x[7], nxt4;
    const unsigned bad = ingest_row<TILE, AIR>(src, tile, proof, s, n, x, nxt4);
    u64 key = TRACE_KEY_VALID;
    if (s < n) key = trace_row_key<AIR>(air[proof], x, bad, nxt4, s, n);
    trace_key_commit(key, keys + proof);

    const bool lane0 = (threadIdx.x & 63) == 0;
    unsigned unused = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) {
        const u64 first = canonical_cell(src.base[src.at.at((u64)proof, (u64)c, 0)], unused, c);  // a uniform address
        if (blockIdx.x == 0 && threadIdx.x == 0) vals[proof * 7 + c] = first;
        if (__any(s < n && x[c] != first) && lane0) flags[proof * 7 + c] = 0;
    }
    if (period && proof > 0) {  // block-uniform
        u64 y[7], none;
        ingest_row<TILE, false>(src, tile, 0, s, n, y, none);
        unsigned char* same = flags + detect_same_off((size_t)gridDim.y * 7);
#pragma unroll
        for (int c = 0; c < 7; c++)
            if (__any(s < n && x[c] != y[c]) && lane0) same[proof * 7 + c] = 0;
    }
}
void launch_trace_ingest_probe(const StridedRows& src, const AirConst* air, int B, int logn, bool with_air, u64* keys,
                               unsigned char* flags, u64* vals, hipStream_t s) {
    HIPCHK(hipMemsetAsync(keys, 0xFF, (size_t)B * 8, s));  // TRACE_KEY_VALID
    const dim3 g((unsigned)(((1ULL << logn) + INGEST_BLOCK - 1) / INGEST_BLOCK), B);
    // classify's presets and fold; the launch between them has the check's geometry, a thread per step
    classify(flags, B * 7, B, logn, 7, s, [&](dim3, dim3, int period) {
        with_bool(with_air, [&](auto AIR) {
            with_bool(src.tiled(), [&](auto TILE) {
                XFG_LAUNCH((trace_ingest_probe_kernel<AIR, TILE>), g, dim3(INGEST_BLOCK), 0, s, src, air, keys, logn, flags,
                           period, vals);
            });
        });
    });
}
// The canonical cells of the live columns into trace [B][7][n], thread s of a block writing tr[c n + s]:
// coalesced. The seven classified flags of the proof are read once, wave-uniform, and the plane of a constant
// or shared column is left as it was, as by trace_gen_kernel; a proof with no live column returns at once
// (the whole block: the flags are the proof's, so no thread is left at a barrier)
template <bool TILE>
__global__ __launch_bounds__(INGEST_BLOCK) void trace_ingest_write_kernel(StridedRows src, u64* trace,
                                                                          const unsigned char* flags, int logn) {
    __shared__ u64 tile[TILE ? INGEST_TILE_WORDS : 1];
    const u64 n = 1ULL << logn;
    const u64 s = (u64)blockIdx.x * INGEST_BLOCK + threadIdx.x;
    const int proof = blockIdx.y;
    const u64 bytes = row_flag_bytes(flags, (u64)proof * 7);
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < 7; c++) live |= ((bytes >> (8 * c)) & 0xFF ? 0u : 1u) << c;
    live = __builtin_amdgcn_readfirstlane(live);
    if (!live) return;
    u64 x[7], none;
    ingest_row<TILE, false>(src, tile, proof, s, n, x, none, live);
    if (s >= n) return;
    u64* tr = trace + (u64)proof * 7 * n;
#pragma unroll
    for (int c = 0; c < 7; c++)
        if ((live >> c) & 1) tr[c * n + s] = x[c];
}
void launch_trace_ingest_write(const StridedRows& src, int B, int logn, const unsigned char* flags, u64* trace,
                               hipStream_t s) {
    const dim3 g((unsigned)(((1ULL << logn) + INGEST_BLOCK - 1) / INGEST_BLOCK), B);
    with_bool(src.tiled(), [&](auto TILE) {
        XFG_LAUNCH(trace_ingest_write_kernel<TILE>, g, dim3(INGEST_BLOCK), 0, s, src, trace, flags, logn);
    });
}
// launch_const_fill: block x of a column writes entries [x, x + 1) * CONST_FILL_SPAN of the LDE plane and the
// same fraction of the coefficients, in 16-byte stores (n and N = beta n are even, planes 16-byte aligned);
// blocks of unflagged columns exit
__global__ __launch_bounds__(256) void const_fill_kernel(const unsigned char* flags, const u64* src, u64 src_stride,
                                                         u64* coef, u64* lde, u64 n, int logbeta) {
    const int col = blockIdx.y;
    if (!flags[col]) return;
    const u64 v = src[(u64)col * src_stride];
    const u64 i0 = (u64)blockIdx.x * CONST_FILL_SPAN;
    if (lde) {
        const u64 N = n << logbeta, i1 = i0 + CONST_FILL_SPAN < N ? i0 + CONST_FILL_SPAN : N;
        u64* o = lde + (u64)col * N;
        const u64x2 d = {v, v};
        for (u64 i = i0 + 2 * threadIdx.x; i < i1; i += 2 * blockDim.x) *reinterpret_cast<u64x2*>(o + i) = d;
    }
    if (coef) {
        // the block's share of the n coefficients (at least two per block: beta <= CONST_FILL_SPAN / 2)
        const u64 span = lde ? (u64)CONST_FILL_SPAN >> logbeta : (u64)CONST_FILL_SPAN;
        const u64 c0 = (u64)blockIdx.x * span, c1 = c0 + span < n ? c0 + span : n;
        u64* o = coef + (u64)col * n;
        for (u64 i = c0 + 2 * threadIdx.x; i < c1; i += 2 * blockDim.x) {
            const u64x2 d = {i == 0 ? v : 0, 0};
            *reinterpret_cast<u64x2*>(o + i) = d;
        }
    }
}
void launch_const_fill(const unsigned char* flags, const u64* src, u64 src_stride, u64* coef, u64* lde, int ncols,
                       int logn, int logbeta, hipStream_t s) {
    if (!coef && !lde) return;
    const u64 n = 1ULL << logn, span = lde ? n << logbeta : n;
    XFG_LAUNCH(const_fill_kernel, dim3((unsigned)((span + CONST_FILL_SPAN - 1) / CONST_FILL_SPAN), ncols), dim3(256), 0, s,
               flags, src, src_stride, coef, lde, n, lde ? logbeta : 0);
}

}  // namespace xfg
