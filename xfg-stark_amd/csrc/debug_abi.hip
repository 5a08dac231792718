// The debug and bench entry points of the C ABI (include/xfg_stark.h): single kernels and launch
// sets of the prover run on lane 0, for the kernel-level parity tests and the micro-benchmarks.
// Each goes through on_lane0 (prover_internal.hpp): refused while batches are pending.
#include <cstring>
#include <vector>

#include "dev_coin.hpp"
#include "dispatch.hpp"
#include "field_dft.hpp"
#include "prover_internal.hpp"

using namespace xfg;

// field-primitive self test (xfg_debug_field): op 0 mul, 1 add, 2 sub, 3 canon(a), 4 a * 2^b,
// 5 fold(a, (u32)b), 6 sub_weak(a, b), 7 add_w(a, b) (the NTT butterfly add, b < p)
__global__ void field_op_kernel(int op, const u64* a, const u64* b, u64* out, u64 count) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const u64 x = a[i], y = b[i];
    u64 r = 0;
    switch (op) {
        case 0: r = gl_mul(x, y); break;
        case 1: r = gl_add(x, y); break;
        case 2: r = gl_sub(x, y); break;
        case 3: r = gl_canon(x); break;
        case 4: {
            const int sh = (int)(y % 96);
            static_for<96>([&](auto sc) {
                if (sh == decltype(sc)::value) r = mul_pow2<decltype(sc)::value>(x);
            });
            break;
        }
        case 5: r = gl_fold(x, (u32)y); break;
        case 6: r = gl_sub_weak(x, y); break;
        case 7: r = add_w(x, y); break;
        case 8: {  // gl_mul2: both products (x y and y x) must equal; the first is returned
            u64 p = x, q = y;
            gl_mul2(p, y, q, x);
            r = p == q ? p : ~0ULL;
            break;
        }
        default: break;
    }
    out[i] = r;
}
// ops 9..12: one thread per pair x = (a[2i], a[2i+1]), y = (b[2i], b[2i+1]) -> out[2i], out[2i+1]
__global__ void field_pair_op_kernel(int op, const u64* a, const u64* b, u64* out, u64 pairs) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    const E2 x{a[2 * i], a[2 * i + 1]}, y{b[2 * i], b[2 * i + 1]};
    E2 r{0, 0};
    switch (op) {
        case 9: {  // one gl_mul2 on two unrelated products
            r = x;
            gl_mul2(r.a, y.a, r.b, y.b);
            break;
        }
        case 10: r = e2_mul(x, y); break;
        case 11: r = e2_mulb(x, y.a); break;
        case 12: r = e2_inv(x); break;
        default: break;
    }
    out[2 * i] = r.a;
    out[2 * i + 1] = r.b;
}
static void launch_field_op(int op, const u64* a, const u64* b, u64* out, u64 count, hipStream_t s) {
    if (op >= 9) {  // count is even (checked by the caller)
        const u64 pairs = count / 2;
        XFG_LAUNCH(field_pair_op_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, op, a, b, out, pairs);
        return;
    }
    XFG_LAUNCH(field_op_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, op, a, b, out, count);
}

// transcript self test (xfg_debug_coin_draws): from coin c0, k <= 64 draws by one wave (out_wave) and
// one at a time (out_seq), both [k][2]; counters after each in ctr[2], success in ok[2].
// AcceptForced: AcceptP plus forced rejections: candidate counter c in [1, 256] is rejected when bit
// c - 1 of rej[4] is set (exercises wave_draw_e's window bookkeeping and its one-at-a-time fallback)
struct AcceptForced {
    const u64* rej;
    __device__ bool operator()(u64 ctr, u64 x, u64 y, int D) const {
        const bool forced = ctr >= 1 && ctr <= 256 && ((rej[(ctr - 1) >> 6] >> ((ctr - 1) & 63)) & 1);
        return !forced && AcceptP()(ctr, x, y, D);
    }
};
__global__ __launch_bounds__(64) void coin_draw_test_kernel(DevCoin c0, int k, int D, const u64* rej, u64* out_wave,
                                                            u64* out_seq, u64* ctr, int* ok) {
    const AcceptForced acc{rej};
    DevCoin c = c0;
    const bool okw = wave_draw_e(c, k, D, out_wave, 2, acc);
    DevCoin q = c0;
    bool oks = true;
    for (int j = 0; j < k; j++) {
        u64 a[2] = {0, 0};
        oks &= dev_draw_e(q, a, D, acc);
        if (threadIdx.x == 0) {
            out_seq[2 * j] = a[0];
            out_seq[2 * j + 1] = a[1];
        }
    }
    if (threadIdx.x == 0) {
        ctr[0] = c.counter;
        ctr[1] = q.counter;
        ok[0] = okw;
        ok[1] = oks;
    }
}
static void launch_coin_draw_test(const DevCoin& c0, int k, int ext, const u64* rej, u64* out_wave, u64* out_seq,
                                  u64* ctr, int* ok, hipStream_t s) {
    XFG_LAUNCH(coin_draw_test_kernel, dim3(1), dim3(64), 0, s, c0, k, ext, rej, out_wave, out_seq, ctr, ok);
}

// xfg_debug_lde / xfg_debug_lde_skip: skip (host, [npoly]) or nullptr
static int debug_lde(xfg_ctx* c, const uint64_t* coef, uint32_t npoly, uint64_t n, uint32_t blowup, const uint8_t* skip,
                     uint64_t* out) {
    if (!c || !coef || !out || !is_pow2(n) || !is_pow2(blowup) || n < 8 || blowup < 2 || blowup > 128)
        return XFG_INVALID_ARGUMENT;
    // (blowup 32, 64, 128: composed LDEs, n * blowup <= 2^24)
    if (!lde_supported((int)ilog2(n), (int)ilog2(blowup))) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const int logn = (int)ilog2(n), logbeta = (int)ilog2(blowup);
        const u64 N = n * blowup;
        ensure_tables(c, logn + logbeta);
        ensure_fourstep(c, logn, logbeta);
        Tables T = tables_of(c);
        L->coef.ensure((size_t)npoly * n);
        L->scratch.ensure((size_t)npoly * N);
        L->lde.ensure((size_t)npoly * N);
        HIPCHK(hipMemcpy(L->coef.p, coef, (size_t)npoly * n * 8, hipMemcpyHostToDevice));
        if (skip) {
            L->const_col.ensure(npoly);
            HIPCHK(hipMemcpy(L->const_col.p, skip, npoly, hipMemcpyHostToDevice));
            // the lane's buffers keep what an earlier call left, which may be this call's answer:
            // whatever the flagged run fails to write must show (0xFF..FF is no field element)
            HIPCHK(hipMemsetAsync(L->scratch.p, 0xFF, (size_t)npoly * N * 8, L->stream));
            HIPCHK(hipMemsetAsync(L->lde.p, 0xFF, (size_t)npoly * N * 8, L->stream));
        }
        launch_lde(L->coef.p, n, L->lde.p, L->scratch.p, npoly, logn, logbeta, T, L->stream, skip ? L->const_col.p : nullptr);
        if (skip) launch_const_fill(L->const_col.p, L->coef.p, n, nullptr, L->lde.p, npoly, logn, logbeta, L->stream);
        std::vector<u64> cm((size_t)npoly * N);
        HIPCHK(hipMemcpyAsync(cm.data(), L->lde.p, cm.size() * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        for (u64 p = 0; p < npoly; p++)  // coset-major -> natural order
            for (u64 t = 0; t < blowup; t++)
                for (u64 m = 0; m < n; m++) out[p * N + t + blowup * m] = cm[(p * blowup + t) * n + m];
        return XFG_OK;
    });
}

// xfg_debug_interpolate / xfg_debug_interpolate_skip
static int debug_interpolate(xfg_ctx* c, const uint64_t* evals, uint32_t npoly, uint64_t n, int offset7,
                             const uint8_t* skip, uint64_t* out) {
    if (!c || !evals || !out || !is_pow2(n) || n < 8 || !ntt_supported((int)ilog2(n), 0, true)) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const int logn = (int)ilog2(n);
        ensure_tables(c, std::max(logn, c->tables.LM));
        if (logn >= 4) ensure_fourstep(c, logn - 1, 1);  // inverse tables up to size n
        Tables T = tables_of(c);
        L->trace.ensure((size_t)npoly * n);
        L->coef.ensure((size_t)npoly * n);
        L->scratch.ensure((size_t)npoly * n);
        HIPCHK(hipMemcpy(L->trace.p, evals, (size_t)npoly * n * 8, hipMemcpyHostToDevice));
        if (skip) {
            L->const_col.ensure(npoly);
            HIPCHK(hipMemcpy(L->const_col.p, skip, npoly, hipMemcpyHostToDevice));
            // as in debug_lde: nothing of an earlier call's answer stays in the buffers
            HIPCHK(hipMemsetAsync(L->scratch.p, 0xFF, (size_t)npoly * n * 8, L->stream));
            HIPCHK(hipMemsetAsync(L->coef.p, 0xFF, (size_t)npoly * n * 8, L->stream));
        }
        launch_interpolate(L->trace.p, n, L->coef.p, n, L->scratch.p, npoly, logn, offset7 != 0, n, T, L->stream,
                           skip ? L->const_col.p : nullptr);
        if (skip) launch_const_fill(L->const_col.p, L->trace.p, n, L->coef.p, nullptr, npoly, logn, 0, L->stream);
        HIPCHK(hipMemcpyAsync(out, L->coef.p, (size_t)npoly * n * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

// xfg_debug_interpolate_keep: launch_interpolate as the prover calls it for the composition polynomial
// and the FRI remainder (keep < n coefficients per polynomial, out_stride = keep)
static constexpr u64 KEEP_GUARD_WORDS = 8;
static int debug_interpolate_keep(xfg_ctx* c, const uint64_t* evals, uint32_t npoly, uint64_t n, uint64_t keep,
                                  int offset7, uint64_t* out) {
    if (!c || !evals || !out || npoly == 0 || !is_pow2(n) || n < 8 || !ntt_supported((int)ilog2(n), 0, true) ||
        keep < 1 || keep > n)
        return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const int logn = (int)ilog2(n);
        ensure_tables(c, std::max(logn, c->tables.LM));
        // inverse tables up to size n, for n = 8 too: always the table path, which is the prover's
        ensure_fourstep(c, std::max(logn - 1, 3), 1);
        Tables T = tables_of(c);
        const size_t words = (size_t)npoly * keep + KEEP_GUARD_WORDS;
        L->trace.ensure((size_t)npoly * n);
        L->coef.ensure((size_t)npoly * n + KEEP_GUARD_WORDS);
        L->scratch.ensure((size_t)npoly * n);
        HIPCHK(hipMemcpy(L->trace.p, evals, (size_t)npoly * n * 8, hipMemcpyHostToDevice));
        // the whole buffer, so that a store anywhere past a polynomial's keep words lands on 0xFF bytes
        HIPCHK(hipMemsetAsync(L->coef.p, 0xFF, ((size_t)npoly * n + KEEP_GUARD_WORDS) * 8, L->stream));
        launch_interpolate(L->trace.p, n, L->coef.p, keep, L->scratch.p, npoly, logn, offset7 != 0, keep, T, L->stream,
                           nullptr);
        HIPCHK(hipMemcpyAsync(out, L->coef.p, words * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

extern "C" {

int xfg_bench_lde(xfg_ctx* c, uint32_t count, uint64_t n, uint32_t blowup, uint32_t iters, double* avg_ms) {
    if (!c || !avg_ms || !is_pow2(n) || !is_pow2(blowup) || n < 8 || blowup < 2 || blowup > 128 || iters == 0)
        return XFG_INVALID_ARGUMENT;
    if (!lde_supported((int)ilog2(n), (int)ilog2(blowup))) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const int logn = (int)ilog2(n), logbeta = (int)ilog2(blowup);
        const u64 N = n * blowup;
        ensure_tables(c, logn + logbeta);
        ensure_fourstep(c, logn, logbeta);
        Tables T = tables_of(c);
        L->coef.ensure((size_t)count * 7 * n);
        L->scratch.ensure((size_t)count * 7 * N);
        L->lde.ensure((size_t)count * 7 * N);
        // deterministic canonical coefficients
        std::vector<u64> h((size_t)count * 7 * n);
        u64 x = 0x46472d535441524bULL;  // "FG-STARK"
        for (auto& v : h) {
            x += 0x9E3779B97F4A7C15ULL;
            u64 z = x;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
            v = (z ^ (z >> 31)) % P;
        }
        HIPCHK(hipMemcpy(L->coef.p, h.data(), h.size() * 8, hipMemcpyHostToDevice));
        launch_lde(L->coef.p, n, L->lde.p, L->scratch.p, count * 7, logn, logbeta, T, L->stream);  // warm
        HIPCHK(hipEventRecord(L->ev[0], L->stream));
        for (uint32_t i = 0; i < iters; i++)
            launch_lde(L->coef.p, n, L->lde.p, L->scratch.p, count * 7, logn, logbeta, T, L->stream);
        HIPCHK(hipEventRecord(L->ev[1], L->stream));
        HIPCHK(hipEventSynchronize(L->ev[1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, L->ev[0], L->ev[1]));
        *avg_ms = ms / iters;
        return XFG_OK;
    });
}

int xfg_lde_probe(xfg_ctx* c, int enabled, double* total_ms, uint64_t* launch_sets, uint64_t* polys) {
    if (!c) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane*) -> int {
        double ms = 0;
        u64 sets = 0, np = 0;
        for (auto& L : c->lanes) {
            ms += L->lde_ms;
            sets += L->lde_sets;
            np += L->lde_polys;
            if (enabled) L->lde_ms = 0, L->lde_sets = 0, L->lde_polys = 0;
            L->lde_probe = enabled != 0;
        }
        if (total_ms) *total_ms = ms;
        c->lde_probe = enabled != 0;
        if (launch_sets) *launch_sets = sets;
        if (polys) *polys = np;
        return XFG_OK;
    });
}

int xfg_debug_lde(xfg_ctx* c, const uint64_t* coef, uint32_t npoly, uint64_t n, uint32_t blowup, uint64_t* out) {
    return debug_lde(c, coef, npoly, n, blowup, nullptr, out);
}
int xfg_debug_lde_skip(xfg_ctx* c, const uint64_t* coef, uint32_t npoly, uint64_t n, uint32_t blowup,
                       const uint8_t* skip, uint64_t* out) {
    if (!skip) return XFG_INVALID_ARGUMENT;
    return debug_lde(c, coef, npoly, n, blowup, skip, out);
}

int xfg_debug_interpolate(xfg_ctx* c, const uint64_t* evals, uint32_t npoly, uint64_t n, int offset7, uint64_t* out) {
    return debug_interpolate(c, evals, npoly, n, offset7, nullptr, out);
}
int xfg_debug_interpolate_skip(xfg_ctx* c, const uint64_t* evals, uint32_t npoly, uint64_t n, int offset7,
                               const uint8_t* skip, uint64_t* out) {
    if (!skip) return XFG_INVALID_ARGUMENT;
    return debug_interpolate(c, evals, npoly, n, offset7, skip, out);
}
int xfg_debug_interpolate_keep(xfg_ctx* c, const uint64_t* evals, uint32_t npoly, uint64_t n, uint64_t keep,
                               int offset7, uint64_t* out) {
    return debug_interpolate_keep(c, evals, npoly, n, keep, offset7, out);
}

int xfg_debug_const_columns(xfg_ctx* c, const uint64_t* trace, uint32_t count, uint32_t width, uint64_t n,
                            uint8_t* flags_out) {
    if (!c || !trace || !flags_out || count == 0 || width == 0 || !is_pow2(n) || n < 8 ||
        (uint64_t)count * width > 0xFFFF)  // one grid row per column
        return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t cols = (size_t)count * width;
        L->trace.ensure(cols * n);
        L->const_col.ensure(cols);
        HIPCHK(hipMemcpy(L->trace.p, trace, cols * n * 8, hipMemcpyHostToDevice));
        launch_const_detect(L->trace.p, (int)cols, (int)ilog2(n), L->const_col.p, L->stream);
        HIPCHK(hipMemcpyAsync(flags_out, L->const_col.p, cols, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

int xfg_debug_col_classes(xfg_ctx* c, const uint64_t* trace, uint32_t count, uint64_t n, uint8_t* classes_out,
                          uint64_t* vals_out) {
    if (!c || !trace || !classes_out || count == 0 || !is_pow2(n) || n < 8 || (uint64_t)count * 7 > 0xFFFF)
        return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t cols = (size_t)count * 7;
        L->trace.ensure(cols * n);
        L->const_col.ensure(const_flag_bytes(cols));
        L->const_val.ensure(cols);
        HIPCHK(hipMemcpy(L->trace.p, trace, cols * n * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(L->const_val.p, 0xFF, cols * 8, L->stream));
        launch_trace_front(L, (int)count, (int)ilog2(n), TraceFront{TraceFront::IN_LANE, TraceFront::NONE, nullptr, {}});
        HIPCHK(hipMemcpyAsync(classes_out, L->const_col.p, cols, hipMemcpyDeviceToHost, L->stream));
        if (vals_out) HIPCHK(hipMemcpyAsync(vals_out, L->const_val.p, cols * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        for (size_t k = 0; k < cols; k++) classes_out[k] = (uint8_t)col_class(classes_out[k]);
        return XFG_OK;
    });
}

int xfg_debug_trace_probe(xfg_ctx* c, uint32_t count, uint64_t n, const xfg_air_consts* airs, uint32_t generator,
                          const xfg_probe_pattern* pattern, uint8_t* classes_out, uint64_t* vals_out,
                          uint64_t* trace_out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    bool ok = airs && classes_out && vals_out && trace_out && count != 0 && (uint64_t)count * 7 <= 0xFFFF &&
              is_pow2(n) && n >= 8 && n <= (1ULL << 24) && generator <= 1 && (generator == 0 || pattern);
    for (int k = 0; ok && generator == 1 && k < 7; k++) ok = pattern->kind[k] <= 4;
    if (!ok) {
        c->err = "xfg_debug_trace_probe: null or unsupported argument";
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t B = count, cols = B * 7;
        std::vector<AirConst> ha;
        if (!airs_of(c, airs, B, ha, L)) return XFG_INVALID_ARGUMENT;
        SynthRowGen synth = {};
        if (generator == 1) {
            for (int k = 0; k < 7; k++) synth.kind[k] = pattern->kind[k], synth.row[k] = pattern->row[k];
            synth.proof = pattern->proof;
        }
        const SynthRowGen* sg = generator == 1 ? &synth : nullptr;
        const int logn = (int)ilog2(n);
        L->trace.ensure(cols * n);
        L->const_col.ensure(const_flag_bytes(cols));
        L->const_val.ensure(cols);
        hipStream_t s = L->stream;
        HIPCHK(hipMemsetAsync(L->trace.p, 0xFF, cols * n * 8, s));
        HIPCHK(hipMemsetAsync(L->const_val.p, 0xFF, cols * 8, s));
        launch_trace_front(L, (int)B, logn, TraceFront{TraceFront::GENERATED, TraceFront::NONE, sg, {}});
        HIPCHK(hipMemcpyAsync(classes_out, L->const_col.p, cols, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(vals_out, L->const_val.p, cols * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(trace_out, L->trace.p, cols * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t k = 0; k < cols; k++) classes_out[k] = (uint8_t)col_class(classes_out[k]);
        return XFG_OK;
    });
}

int xfg_debug_trace_ingest(xfg_ctx* c, uint32_t count, uint64_t n, const uint64_t* buf, uint64_t buf_words,
                           const xfg_trace_layout* layout, const xfg_air_consts* airs, int validate,
                           uint8_t* classes_out, uint64_t* vals_out, xfg_trace_fault* faults_out, uint64_t* trace_out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    const bool ok = buf && airs && classes_out && vals_out && faults_out && trace_out && count != 0 &&
                    (uint64_t)count * 7 <= 0xFFFF && is_pow2(n) && n >= 8 && n <= (1ULL << 24);
    const TraceLayout at = layout_of(ok ? layout : nullptr, n);
    u64 extent = 0;
    if (!ok || !trace_extent(at, count, n, &extent) || extent > buf_words) {
        c->err = "xfg_debug_trace_ingest: null or unsupported argument, or an extent outside the buffer";
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t B = count, cols = B * 7;
        std::vector<AirConst> ha;
        if (!airs_of(c, airs, B, ha, L)) return XFG_INVALID_ARGUMENT;
        const int logn = (int)ilog2(n);
        // buf_words and no headroom (DBuf adds some): what is read past the buffer is not the hook's memory
        struct DevFree {
            void operator()(u64* p) const { (void)hipFree(p); }
        };
        u64* raw = nullptr;
        HIPCHK(hipMalloc((void**)&raw, buf_words * 8));
        const std::unique_ptr<u64, DevFree> src(raw);
        L->trace.ensure(cols * n);
        L->tkeys.ensure(B);
        L->const_col.ensure(const_flag_bytes(cols));
        L->const_val.ensure(cols);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpy(src.get(), buf, buf_words * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(L->trace.p, 0xFF, cols * n * 8, s));
        HIPCHK(hipMemsetAsync(L->const_val.p, 0xFF, cols * 8, s));
        launch_trace_front(L, (int)B, logn, TraceFront{TraceFront::IN_PLACE, validate ? TraceFront::AIR : TraceFront::CANONICAL,
                                                      nullptr, StridedRows{src.get(), at}});
        std::vector<u64> keys(B);
        HIPCHK(hipMemcpyAsync(keys.data(), L->tkeys.p, B * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(classes_out, L->const_col.p, cols, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(vals_out, L->const_val.p, cols * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(trace_out, L->trace.p, cols * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (size_t k = 0; k < cols; k++) classes_out[k] = (uint8_t)col_class(classes_out[k]);
        TraceSrc host;  // `found` comes from the caller's copy of the buffer
        host.kind = TraceSrc::HOST_STAGED;
        host.p = buf;
        host.layout = at;
        for (size_t b = 0; b < B; b++) faults_out[b] = trace_fault_of(keys[b], ha[b], host, b, nullptr);
        return XFG_OK;
    });
}

int xfg_debug_field(xfg_ctx* c, uint32_t op, uint64_t count, const uint64_t* a, const uint64_t* b, uint64_t* out) {
    if (!c || !a || !b || !out || op > 12 || count == 0 || (op >= 9 && count % 2)) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        L->trace.ensure((size_t)count * 3);
        u64* da = L->trace.p;
        u64* db = da + count;
        u64* dout = db + count;
        HIPCHK(hipMemcpy(da, a, count * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(db, b, count * 8, hipMemcpyHostToDevice));
        launch_field_op((int)op, da, db, dout, count, L->stream);
        HIPCHK(hipMemcpyAsync(out, dout, count * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

int xfg_debug_coin_draws(xfg_ctx* c, const uint32_t seed[8], uint64_t counter, uint32_t k, uint32_t ext,
                         const uint64_t reject[4], uint64_t* out_wave, uint64_t* out_seq, uint64_t counters[2],
                         int ok[2]) {
    if (!c || !seed || !reject || !out_wave || !out_seq || !counters || !ok || k == 0 || k > 64 ||
        (ext != 1 && ext != 2))
        return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        L->trace.ensure(4 + 4 * (size_t)k + 2 + 1);
        u64* drej = L->trace.p;
        u64* dw = drej + 4;
        u64* ds = dw + 2 * k;
        u64* dctr = ds + 2 * k;
        int* dok = (int*)(dctr + 2);
        HIPCHK(hipMemcpy(drej, reject, 32, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(dw, 0, 16 * (size_t)k));
        DevCoin c0;
        memcpy(c0.seed.w, seed, 32);
        c0.counter = counter;
        c0.pad = 0;
        launch_coin_draw_test(c0, (int)k, (int)ext, drej, dw, ds, dctr, dok, L->stream);
        HIPCHK(hipMemcpyAsync(out_wave, dw, 16 * (size_t)k, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipMemcpyAsync(out_seq, ds, 16 * (size_t)k, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipMemcpyAsync(counters, dctr, 16, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipMemcpyAsync(ok, dok, 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

int xfg_debug_grind(xfg_ctx* c, uint32_t count, const uint32_t* seeds, uint32_t grind, uint64_t first_nonce,
                    uint64_t max_nonce, uint32_t chunk_log, uint32_t blocks, uint64_t* nonces_out) {
    if (!c || !seeds || !nonces_out || count == 0 || grind > GRIND_MAX || first_nonce == 0 ||
        (chunk_log != 0 && (chunk_log < GRIND_CHUNK_LOG_MIN || chunk_log > GRIND_CHUNK_LOG_MAX)) ||
        blocks > GRIND_FORCED_BLOCKS_MAX)
        return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        const GrindPlan gp = grind_plan(grind, count, (unsigned)L->cus);
        memcpy(grind_seeds(L, count), seeds, (size_t)count * sizeof(Digest));
        const u64* got = grind_search(L, (int)count, grind, first_nonce, max_nonce ? max_nonce : gp.max_nonce,
                                      chunk_log ? chunk_log : gp.chunk_log, blocks ? blocks : gp.blocks);
        memcpy(nonces_out, got, (size_t)count * 8);
        return XFG_OK;
    });
}

int xfg_debug_keccak256(xfg_ctx* c, uint32_t count, const uint8_t* msgs, const uint32_t* lens, uint8_t* out) {
    if (!c || !msgs || !lens || !out || count == 0 || count > 65535) return XFG_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < count; i++)
        if (lens[i] >= KECCAK_RATE) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane* L) -> int {
        // the lane's word buffers as byte buffers: messages in coef, lengths in trace, digests in scratch
        const size_t mbytes = (size_t)count * KECCAK_RATE;
        L->coef.ensure((mbytes + 7) / 8);
        L->trace.ensure(((size_t)count * 4 + 7) / 8);
        L->scratch.ensure((size_t)count * 4);
        HIPCHK(hipMemcpy(L->coef.p, msgs, mbytes, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(L->trace.p, lens, (size_t)count * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemsetAsync(L->scratch.p, 0xFF, (size_t)count * 32, L->stream));
        launch_keccak256((const uint8_t*)L->coef.p, (const u32*)L->trace.p, (int)count, (uint8_t*)L->scratch.p, L->stream);
        HIPCHK(hipMemcpyAsync(out, L->scratch.p, (size_t)count * 32, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        return XFG_OK;
    });
}

int xfg_grind_probe(const xfg_ctx* c, uint32_t* device_min, uint64_t* device_searches, uint64_t* host_searches) {
    if (!c) return XFG_INVALID_ARGUMENT;
    uint64_t dev = 0, host = 0;
    for (auto& L : c->lanes) {
        dev += L->grind_dev;
        host += L->grind_host;
    }
    if (device_min) *device_min = GRIND_DEVICE_MIN;
    if (device_searches) *device_searches = dev;
    if (host_searches) *host_searches = host;
    return XFG_OK;
}

int xfg_debug_ood_deep(xfg_ctx* c, uint32_t count, uint64_t n, const uint64_t* coef, const uint64_t* hcoef,
                       const uint64_t* zpts, const uint64_t* coeffs, uint64_t* ood_out, uint64_t* deep_out) {
    return xfg_debug_ood_deep_e(c, count, n, 1, coef, hcoef, zpts, coeffs, nullptr, nullptr, 0, ood_out, deep_out,
                                nullptr, nullptr, nullptr, nullptr);
}

int xfg_debug_ood_deep_e(xfg_ctx* c, uint32_t count, uint64_t n, uint32_t ext, const uint64_t* coef,
                         const uint64_t* hcoef, const uint64_t* zpts, const uint64_t* coeffs,
                         const uint32_t* coin_seeds, const uint64_t* coin_counters, uint64_t ginv, uint64_t* ood_out,
                         uint64_t* deep_out, uint64_t* dp_out, uint32_t* seeds_out, uint64_t* counters_out,
                         int* fail_out) {
    return xfg_debug_ood_deep_const(c, count, n, ext, coef, nullptr, nullptr, hcoef, zpts, coeffs, coin_seeds,
                                    coin_counters, ginv, ood_out, deep_out, dp_out, seeds_out, counters_out, fail_out);
}

int xfg_debug_ood_deep_const(xfg_ctx* c, uint32_t count, uint64_t n, uint32_t ext, const uint64_t* coef,
                             const uint8_t* flags, const uint64_t* vals, const uint64_t* hcoef, const uint64_t* zpts,
                             const uint64_t* coeffs, const uint32_t* coin_seeds, const uint64_t* coin_counters,
                             uint64_t ginv, uint64_t* ood_out, uint64_t* deep_out, uint64_t* dp_out, uint32_t* seeds_out,
                             uint64_t* counters_out, int* fail_out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    const bool coin = coin_seeds != nullptr;
    if (flags) {
        bool ok = vals != nullptr && count <= 0xFFFF;
        for (size_t k = 0; ok && k < (size_t)count * 7; k++) ok = flags[k] <= 2 && !(k < 7 && flags[k] == 2);
        if (!ok) {
            c->err = "xfg_debug_ood_deep_const: flags are 0, 1 or 2 (never 2 for instance 0) and come with vals";
            return XFG_INVALID_ARGUMENT;
        }
    }
    // the shape first: nothing below reads an array or sizes a buffer for a shape that is refused
    // (launch_deep: one carry thread per block of 2048 coefficients, at most 1024; one grid row per instance)
    if ((ext != 1 && ext != 2) || !is_pow2(n) || n < 8 || n > (1ULL << 21) || count == 0 || count > 0xFFFF) {
        c->err = "xfg_debug_ood_deep: ext is 1 or 2, n a power of two in [8, 2^21], count in [1, 65535]";
        return XFG_INVALID_ARGUMENT;
    }
    if (!coef || !hcoef || !zpts || !ood_out || !deep_out ||
        (coin ? !coin_counters || !dp_out || !seeds_out || !counters_out || !fail_out : !coeffs)) {
        c->err = "xfg_debug_ood_deep: null argument";
        return XFG_INVALID_ARGUMENT;
    }
    const size_t B = count, D = ext;
    if (!all_canonical(coef, B * 7 * n) || !all_canonical(hcoef, B * D * n) || !all_canonical(zpts, B * 2 * D) ||
        (coin ? ginv >= P : !all_canonical(coeffs, B * 8 * D))) {
        c->err = "xfg_debug_ood_deep: a word is not a canonical field element";
        return XFG_INVALID_ARGUMENT;
    }
    auto e_at = [D](const u64* v) { return E2{v[0], D == 2 ? v[1] : 0}; };
    if (!coin)  // the quotients by (x - z) and (x - z g) take 1 / z and 1 / (z g)
        for (size_t k = 0; k < B * 2; k++)
            if (e2_eq(e_at(zpts + k * D), E2{0, 0})) {
                c->err = "xfg_debug_ood_deep: z and z g must not be zero";
                return XFG_INVALID_ARGUMENT;
            }
    return on_lane0(c, [&](Lane* L) -> int {
        const ProofShape sh(n, Opts{0, 2, 0, ext, 8, 31});  // the blowup plays no part
        const int logn = sh.logn;
        L->coef.ensure(B * 7 * n);
        size_ood_deep(L, B, sh);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpyAsync(L->coef.p, coef, B * 7 * n * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(L->hcoef.p, hcoef, B * D * n * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(L->zpts.p, zpts, B * 2 * D * 8, hipMemcpyHostToDevice, s));
        ColConst cc;
        if (flags) {  // the flagged planes hold no field element: a kernel that reads one shows it
            const size_t cols = B * 7;
            L->const_col.ensure((cols + 3) & ~(size_t)3);
            L->const_val.ensure(cols);
            HIPCHK(hipMemcpyAsync(L->const_col.p, flags, cols, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(L->const_val.p, vals, cols * 8, hipMemcpyHostToDevice, s));
            for (size_t k = 0; k < cols; k++)
                if (flags[k]) HIPCHK(hipMemsetAsync(L->coef.p + k * n, 0xFF, n * 8, s));
            cc.flags = L->const_col.p;
            cc.vals = L->const_val.p;
            cc.val_stride = 1;
        }
        // as the Merkle entries: what a kernel fails to store must show, whatever an earlier call left
        const size_t nblk = ood_partial_count(logn);
        HIPCHK(hipMemsetAsync(L->partial.p, 0xFF, B * nblk * 15 * D * 8, s));
        HIPCHK(hipMemsetAsync(L->carry.p, 0xFF, B * nblk * 2 * D * 8, s));
        HIPCHK(hipMemsetAsync(L->ood.p, 0xFF, B * 15 * D * 8, s));
        HIPCHK(hipMemsetAsync(L->dp.p, 0xFF, B * sizeof(DeepParams), s));
        HIPCHK(hipMemsetAsync(L->deep.p, 0xFF, B * D * n * 8, s));
        if (coin) {  // as prove_lane: the frame's block draws the coefficients and writes the DeepParams
            L->dcoin.ensure(B);
            L->dfail.ensure(B);
            std::vector<DevCoin> hc(B);
            for (size_t b = 0; b < B; b++) {
                memcpy(hc[b].seed.w, coin_seeds + 8 * b, 32);
                hc[b].counter = coin_counters[b];
                hc[b].pad = 0;
            }
            HIPCHK(hipMemcpyAsync(L->dcoin.p, hc.data(), B * sizeof(DevCoin), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(L->dfail.p, 0, B * sizeof(int), s));
            DeepCoinStep dc;
            dc.coins = L->dcoin.p;
            dc.fail = L->dfail.p;
            dc.zpts = L->zpts.p;
            dc.dp = L->dp.p;
            dc.ginv = ginv;
            launch_ood(L->coef.p, L->hcoef.p, L->zpts.p, L->partial.p, L->ood.p, logn, (int)B, (int)ext, s, dc, cc);
            launch_deep(L->coef.p, L->hcoef.p, L->dp.p, L->partial.p, L->carry.p, L->deep.p, logn, (int)B, (int)ext, s, cc);
            std::vector<DeepParams> dps(B);
            HIPCHK(hipMemcpyAsync(ood_out, L->ood.p, B * 15 * D * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(deep_out, L->deep.p, B * D * n * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(dps.data(), L->dp.p, B * sizeof(DeepParams), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hc.data(), L->dcoin.p, B * sizeof(DevCoin), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(fail_out, L->dfail.p, B * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t b = 0; b < B; b++) {
                static_assert(sizeof(DeepParams) == 30 * 8, "dp_out: the 28 words before DeepParams::pad");
                memcpy(dp_out + 28 * b, &dps[b], 28 * 8);
                memcpy(seeds_out + 8 * b, hc[b].seed.w, 32);
                counters_out[b] = hc[b].counter;
            }
            return XFG_OK;
        }
        launch_ood(L->coef.p, L->hcoef.p, L->zpts.p, L->partial.p, L->ood.p, logn, (int)B, (int)ext, s, DeepCoinStep{}, cc);
        HIPCHK(hipMemcpyAsync(ood_out, L->ood.p, B * 15 * D * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::vector<DeepParams> dps(B);
        for (size_t b = 0; b < B; b++) {  // what the device transcript step derives: c1, c2 from the OOD values
            DeepParams& dp = dps[b];
            memset(&dp, 0, sizeof dp);
            auto put = [D](u64* d, E2 v) {
                d[0] = v.a;
                if (D == 2) d[1] = v.b;
            };
            const u64* cf = coeffs + b * 8 * D;
            const u64* o = ood_out + b * 15 * D;
            const E2 z = e_at(zpts + b * 2 * D), zg = e_at(zpts + b * 2 * D + D), gamma = e_at(cf + 7 * D);
            E2 c1 = e2_mul(gamma, e_at(o + 14 * D)), c2{0, 0};
            for (int k = 0; k < 7; k++) {
                const E2 a = e_at(cf + k * D);
                put(dp.a[k], a);
                c1 = e2_add(c1, e2_mul(a, e_at(o + 2 * k * D)));
                c2 = e2_add(c2, e2_mul(a, e_at(o + (2 * k + 1) * D)));
            }
            put(dp.gamma, gamma);
            put(dp.z, z);
            put(dp.zg, zg);
            put(dp.zinv, e2_inv(z));
            put(dp.zginv, e2_inv(zg));
            put(dp.c1, c1);
            put(dp.c2, c2);
        }
        HIPCHK(hipMemcpyAsync(L->dp.p, dps.data(), B * sizeof(DeepParams), hipMemcpyHostToDevice, s));
        launch_deep(L->coef.p, L->hcoef.p, L->dp.p, L->partial.p, L->carry.p, L->deep.p, logn, (int)B, (int)ext, s, cc);
        HIPCHK(hipMemcpyAsync(deep_out, L->deep.p, B * D * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return XFG_OK;
    });
}

int xfg_debug_constraint_eval(xfg_ctx* c, uint32_t count, uint64_t n, uint32_t blowup, uint32_t ext,
                              const uint64_t* trace, const xfg_air_consts* airs, const uint64_t* coeffs,
                              uint64_t* ce) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!trace || !airs || !coeffs || !ce || count == 0 || !is_pow2(n) || n < 8 || !is_pow2(blowup) || blowup < 2 ||
        blowup > 128 || wide_lde_too_large(n, blowup) || (ext != 1 && ext != 2)) {
        c->err = "xfg_debug_constraint_eval: null or unsupported argument";
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t B = count;
        if (!all_canonical(trace, B * 7 * n) || !all_canonical(coeffs, B * 15 * ext)) {
            c->err = "trace element or coefficient is not a canonical field element";
            return XFG_INVALID_ARGUMENT;
        }
        std::vector<AirConst> ha;
        if (!airs_of(c, airs, B, ha, L)) return XFG_INVALID_ARGUMENT;
        const ProofShape sh(n, Opts{0, blowup, 0, ext, 8, 31});
        ensure_tables(c, std::max(sh.logn + sh.logbeta, sh.logn + 1));
        ensure_fourstep(c, sh.logn, sh.logbeta);
        const Tables T = tables_of(c);
        const u64* ce_div = ensure_ce_table(c, sh.logn);
        size_trace_lde(L, B, sh);
        size_constraint_eval(L, B, sh);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpy(L->trace.p, trace, B * 7 * n * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(L->coeffs.p, coeffs, B * 15 * ext * 8, hipMemcpyHostToDevice));
        launch_trace_front(L, (int)B, sh.logn, TraceFront{TraceFront::IN_LANE, TraceFront::NONE, nullptr, {}});
        launch_trace_lde(L, T, (int)B, sh, false);
        launch_constraint_eval(L->lde.p, L->air.p, L->coeffs.p, ce_div, L->ce.p, sh.logn, sh.logbeta, (int)B, sh.DE, s,
                               trace_const(L, sh), L->ce_uni.p);
        HIPCHK(hipMemcpyAsync(ce, L->ce.p, B * ext * 2 * n * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return XFG_OK;
    });
}

int xfg_debug_fri_fold(xfg_ctx* c, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                       const uint64_t* vals, const uint64_t* alpha, uint64_t* out) {
    return xfg_debug_fri_fold_f(c, count, ext, logn, logbeta, coset_major, 8, vals, alpha, out);
}

int xfg_debug_fri_fold_f(xfg_ctx* c, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                         uint32_t fold, const uint64_t* vals, const uint64_t* alpha, uint64_t* out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    const unsigned logf = fold_log2(fold);  // 0: no kernel; D >= 2 fold
    if (!vals || !alpha || !out || count == 0 || (ext != 1 && ext != 2) || logn > 28 || logbeta > 28 || !logf ||
        logn + logbeta < logf + 1 || logn + logbeta > 28) {
        c->err = "xfg_debug_fri_fold: null or unsupported argument";
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t B = count;
        const int logD = (int)(logn + logbeta);
        const u64 D = 1ULL << logD, rows = D / fold;
        if (!all_canonical(vals, B * ext * D) || !all_canonical(alpha, B * ext)) {
            c->err = "layer value or alpha is not a canonical field element";
            return XFG_INVALID_ARGUMENT;
        }
        ensure_tables(c, logD);
        const Tables T = tables_of(c);
        L->f0.ensure(B * ext * D);
        L->alpha7.ensure(B * ext);
        L->deep.ensure(B * ext * rows);
        // alpha * 7^-1 per coordinate (7^-1 is a base-field element), as the device transcript step stores it
        const u64 i7 = gl_inv(GEN);
        std::vector<u64> a7(B * ext);
        for (size_t k = 0; k < a7.size(); k++) a7[k] = gl_mul(alpha[k], i7);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpy(L->f0.p, vals, B * ext * D * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(L->alpha7.p, a7.data(), a7.size() * 8, hipMemcpyHostToDevice));
        launch_fri_fold(L->f0.p, ext * D, D, coset_major != 0, (int)logn, (int)logbeta, rows, logD, L->alpha7.p,
                        L->deep.p, rows, T, (int)B, (int)ext, (int)fold, s);
        HIPCHK(hipMemcpyAsync(out, L->deep.p, B * ext * rows * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return XFG_OK;
    });
}

// The Merkle entries set the heaps to 0xFF bytes before the launches: a node a kernel fails to
// store must show, whatever an earlier call left in the lane's buffers.
// xfg_debug_merkle_lde (flags = vals = nullptr, blowup up to 16) and xfg_debug_merkle_lde_const
static int debug_merkle_lde(xfg_ctx* c, uint32_t count, uint32_t nc, uint64_t n, uint32_t blowup, uint32_t max_blowup,
                            const uint64_t* lde, const uint8_t* flags, const uint64_t* vals, const uint64_t* entries,
                            uint64_t nentries, uint8_t* nodes_out, uint8_t* local_out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!lde || !nodes_out || (nentries && (!entries || !local_out)) || count == 0 || count > 0xFFFF ||
        (nc != 1 && nc != 2 && nc != 7) || !is_pow2(blowup) || blowup < 2 || blowup > max_blowup || !is_pow2(n) ||
        n < 8 || n > (1ULL << 24) || (flags && (!vals || nc != 7))) {
        c->err = "xfg_debug_merkle_lde: null or unsupported argument";
        return XFG_INVALID_ARGUMENT;
    }
    for (uint64_t e = 0; e < nentries; e++)
        if (entries[e] >= (uint64_t)count * n) {
            c->err = "xfg_debug_merkle_lde: entry names a proof or row out of range";
            return XFG_INVALID_ARGUMENT;
        }
    return on_lane0(c, [&](Lane* L) -> int {
        const int logn = (int)ilog2(n), logbeta = (int)ilog2(blowup);
        const size_t B = count, nlde = B * nc * blowup * n, nloc = (size_t)nentries * 2 * blowup;
        L->lde.ensure(nlde);
        L->tnodes.ensure(B * 2 * n);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpyAsync(L->lde.p, lde, nlde * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(L->tnodes.p, 0xFF, B * 2 * n * sizeof(Digest), s));
        ColConst cc;
        if (flags) {  // the flagged planes hold no field element: a kernel that reads one hashes 0xFF bytes
            const size_t cols = B * nc, N = (size_t)blowup * n;
            L->const_col.ensure((cols + 3) & ~(size_t)3);
            L->coef.ensure(cols);
            HIPCHK(hipMemcpyAsync(L->const_col.p, flags, cols, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(L->coef.p, vals, cols * 8, hipMemcpyHostToDevice, s));
            for (size_t k = 0; k < cols; k++)
                if (flags[k]) HIPCHK(hipMemsetAsync(L->lde.p + k * N, 0xFF, N * 8, s));
            cc.flags = L->const_col.p;
            cc.vals = L->coef.p;
            cc.val_stride = 1;
        }
        launch_merkle_lde(L->lde.p, (int)nc, L->tnodes.p, (int)B, logn, logbeta, s, CoinStep{}, cc);
        HIPCHK(hipMemcpyAsync(nodes_out, L->tnodes.p, B * 2 * n * sizeof(Digest), hipMemcpyDeviceToHost, s));
        if (nentries) {
            L->scratch.ensure(nentries);
            L->hnodes.ensure(nloc);
            HIPCHK(hipMemcpyAsync(L->scratch.p, entries, nentries * 8, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(L->hnodes.p, 0xFF, nloc * sizeof(Digest), s));
            launch_open_rows(L->lde.p, (int)nc, L->scratch.p, nentries, L->hnodes.p, logn, logbeta, s, cc);
            HIPCHK(hipMemcpyAsync(local_out, L->hnodes.p, nloc * sizeof(Digest), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s));
        return XFG_OK;
    });
}

int xfg_debug_merkle_lde(xfg_ctx* c, uint32_t count, uint32_t nc, uint64_t n, uint32_t blowup, const uint64_t* lde,
                         const uint64_t* entries, uint64_t nentries, uint8_t* nodes_out, uint8_t* local_out) {
    return debug_merkle_lde(c, count, nc, n, blowup, 16, lde, nullptr, nullptr, entries, nentries, nodes_out, local_out);
}
int xfg_debug_merkle_lde_const(xfg_ctx* c, uint32_t count, uint32_t nc, uint64_t n, uint32_t blowup,
                               const uint64_t* lde, const uint8_t* flags, const uint64_t* vals, const uint64_t* entries,
                               uint64_t nentries, uint8_t* nodes_out, uint8_t* local_out) {
    return debug_merkle_lde(c, count, nc, n, blowup, 128, lde, flags, vals, entries, nentries, nodes_out, local_out);
}

int xfg_debug_poison_lde(xfg_ctx* c, int on) {
    if (!c) return XFG_INVALID_ARGUMENT;
    return on_lane0(c, [&](Lane*) -> int {
        c->poison_lde = on != 0;
        for (auto& L : c->lanes) L->poison_lde = on != 0;
        return XFG_OK;
    });
}

int xfg_debug_merkle_fri(xfg_ctx* c, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                         const uint64_t* vals, uint8_t* nodes_out) {
    return xfg_debug_merkle_fri_f(c, count, ext, logn, logbeta, coset_major, 8, vals, nodes_out);
}

int xfg_debug_merkle_fri_f(xfg_ctx* c, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                           uint32_t fold, const uint64_t* vals, uint8_t* nodes_out) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    const unsigned logf = fold_log2(fold);  // 0: no kernel; D >= 2 fold
    if (!vals || !nodes_out || count == 0 || count > 0xFFFF || (ext != 1 && ext != 2) || logn > 28 || logbeta > 28 ||
        !logf || logn + logbeta < logf + 1 || logn + logbeta > 28) {
        c->err = "xfg_debug_merkle_fri: null or unsupported argument";
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t B = count;
        const u64 D = 1ULL << (logn + logbeta), rows = D / fold;
        if (!all_canonical(vals, B * ext * D)) {
            c->err = "layer value is not a canonical field element";
            return XFG_INVALID_ARGUMENT;
        }
        L->f0.ensure(B * ext * D);
        L->tnodes.ensure(B * 2 * rows);
        hipStream_t s = L->stream;
        HIPCHK(hipMemcpyAsync(L->f0.p, vals, B * ext * D * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(L->tnodes.p, 0xFF, B * 2 * rows * sizeof(Digest), s));
        launch_merkle_fri(L->f0.p, ext * D, D, coset_major != 0, (int)logn, (int)logbeta, rows, L->tnodes.p, (int)B,
                          (int)ext, (int)fold, s);
        HIPCHK(hipMemcpyAsync(nodes_out, L->tnodes.p, B * 2 * rows * sizeof(Digest), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return XFG_OK;
    });
}

}  // extern "C"
