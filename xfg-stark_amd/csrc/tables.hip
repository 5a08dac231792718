// The context's table registry: twiddles and powers of the coset generator, the constraint divisors
// per trace length and the four-step / pass tables of the NTT sizes a proof shape uses. Built on
// demand by the submitting thread (prover.hip bind_tables, drained first) and the debug entry points.
#include <algorithm>

#include "prover_internal.hpp"

namespace xfg {

// Data-independent constraint divisors on the CE domain x_i = 7 w_2n^i (i = 2m + par), laid out
// [3][par][m]: transition (x - g^(n-1)) / (x^n - 1), boundary 1/(x - 1) and 1/(x - g^(n-1))
// (ConstraintDivisor::from_transition / from_assertion). Batch-inverted once per trace length.
static std::vector<u64> ce_divisor_table(int logn) {
    const u64 n = 1ULL << logn, nce = 2 * n;
    const u64 w = gl_root(logn + 1), g_last = gl_pow(gl_root(logn), n - 1);
    const u64 sn = gl_pow(GEN, n);
    const u64 inv_xn1[2] = {gl_inv(gl_sub(sn, 1)), gl_inv(gl_sub(gl_neg(sn), 1))};
    std::vector<u64> xa(nce), xb(nce), prod(nce);
    u64 x = GEN, acc = 1;
    for (u64 i = 0; i < nce; i++, x = gl_mul(x, w)) {
        xa[i] = gl_sub(x, 1);
        xb[i] = gl_sub(x, g_last);
        acc = gl_mul(acc, gl_mul(xa[i], xb[i]));
        prod[i] = acc;
    }
    u64 inv = gl_inv(acc);
    std::vector<u64> out(3 * nce);
    for (u64 i = nce; i-- > 0;) {
        u64 inv_ab = i ? gl_mul(inv, prod[i - 1]) : inv;  // 1 / (xa_i xb_i)
        inv = gl_mul(inv, gl_mul(xa[i], xb[i]));
        const u64 par = i & 1, m = i >> 1, di = par * n + m;
        out[di] = gl_mul(xb[i], inv_xn1[par]);
        out[nce + di] = gl_mul(inv_ab, xb[i]);
        out[2 * nce + di] = gl_mul(inv_ab, xa[i]);
    }
    return out;
}

void ensure_tables(xfg_ctx* c, int LM) {
    if (c->tables.LM >= LM) return;
    u64 M = 1ULL << LM;
    std::vector<u64> tw(M), p7(M), ip7(M);
    u64 w = gl_root(LM), x = 1, y = 1, z = 1, i7 = gl_inv(GEN);
    for (u64 e = 0; e < M; e++) {
        tw[e] = x;
        p7[e] = y;
        ip7[e] = z;
        x = gl_mul(x, w);
        y = gl_mul(y, GEN);
        z = gl_mul(z, i7);
    }
    c->tables.tw.release();
    c->tables.pow7.release();
    c->tables.ipow7.release();
    c->tables.tw.ensure(M);
    c->tables.pow7.ensure(M);
    c->tables.ipow7.ensure(M);
    HIPCHK(hipMemcpy(c->tables.tw.p, tw.data(), M * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->tables.pow7.p, p7.data(), M * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->tables.ipow7.p, ip7.data(), M * 8, hipMemcpyHostToDevice));
    c->tables.LM = LM;
}
const u64* ensure_ce_table(xfg_ctx* c, int logn) {
    auto& d = c->tables.ce_div[logn];
    if (!d.p) {
        std::vector<u64> t = ce_divisor_table(logn);
        d.ensure(t.size());
        HIPCHK(hipMemcpy(d.p, t.data(), t.size() * 8, hipMemcpyHostToDevice));
    }
    return d.p;
}
Tables tables_of(xfg_ctx* c) {
    Tables T;
    T.tw = c->tables.tw.p;
    T.LM = c->tables.LM;
    T.pow7 = c->tables.pow7.p;
    T.ipow7 = c->tables.ipow7.p;
    T.fs = &c->tables.fs;
    return T;
}
__global__ void fourstep_kernel(u64* out, int logn, int logbeta, int logC, u64 scale, Tables T) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 n = 1ULL << logn;
    if (logbeta < 0) {
        if (i >= n) return;
        const u64 k1 = i >> logC, j2 = i & ((1ULL << logC) - 1);
        out[i] = gl_mul(tw_get(T, logn, (j2 * k1) & (n - 1), true), scale);
    } else {
        const int logN = logn + logbeta;
        if (i >= (1ULL << logN)) return;
        const u64 t = i >> logn, k1 = (i & (n - 1)) >> logC, j2 = i & ((1ULL << logC) - 1);
        out[i] = gl_mul(T.pow7[j2], tw_get(T, logN, (j2 * (t + (k1 << logbeta))) & ((1ULL << logN) - 1), false));
    }
}
// the pass tables (PassTableLayout, ntt_plan.hpp): what every pass block would otherwise gather from
// the master tables at its start
__global__ void pass_tables_kernel(u64* out, PassTableLayout L, Tables T) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const int logR = L.logR, logC = L.logC, logbeta = L.logbeta;
    const u64 R = L.R(), C = L.C(), Z = 0;
    if (i >= L.total()) return;
    if (i < L.wC()) {
        out[i] = tw_get(T, logR, i, !L.fwd());
    } else if (i < L.pre(Z)) {
        out[i] = tw_get(T, logC, i - L.wC(), !L.fwd());
    } else if (i < L.comb(Z)) {
        const u64 t = (i - L.pre(Z)) >> logR, j = (i - L.pre(Z)) & (R - 1);
        out[i] = gl_mul(T.pow7[j << logC], tw_get(T, logR + logbeta, (t * j) & ((1ULL << (logR + logbeta)) - 1), false));
    } else if (L.has_r1024() && i < L.r1024_seed(Z)) {
        // ntt_pass_a_r1024: [t][r][k] = w_1024^(r k) g_t^r, g_t^r = 7^(C r) w_(beta R)^(t r)  (r, k < 32)
        const u64 q = i - L.comb(Z);
        const u64 t = q >> 10, r = (q >> 5) & 31, k = q & 31;
        const u64 g = gl_mul(T.pow7[r << logC], tw_get(T, logR + logbeta, (t * r) & ((1ULL << (logR + logbeta)) - 1), false));
        out[i] = gl_mul(tw_get(T, logR, r * k, false), g);
    } else if (L.has_r1024()) {
        // ntt_pass_a_r1024's four-step factors: [t][j2] 7^j2 w_N^(j2 t) (t < beta, j2 < C) and the
        // t-independent four-step table [k1][j2] w_n^(j2 k1) (R x C)
        const int logn = logR + logC, logN = logn + logbeta;
        const u64 j2 = i & (C - 1);  // both regions start at multiples of C
        if (i < L.r1024_t4()) {
            const u64 t = (i - L.r1024_seed(Z)) >> logC;
            out[i] = gl_mul(T.pow7[j2], tw_get(T, logN, (j2 * t) & ((1ULL << logN) - 1), false));
        } else {
            const u64 k1 = (i - L.r1024_t4()) >> logC;
            out[i] = tw_get(T, logn, (j2 * k1) & ((1ULL << logn) - 1), false);
        }
    } else if (i < L.cos2_scal()) {
        // ntt_pass_a_cos2: [t][r][k] = w_R^(r k) 7^(C r) w_(beta R)^(t r)
        const u64 q = i - L.comb(Z);
        const u64 t = q >> 8, r = (q >> 4) & 15, k = q & 15;
        const u64 grp = gl_mul(T.pow7[r << logC], tw_get(T, logR + logbeta, (t * r) & ((1ULL << (logR + logbeta)) - 1), false));
        out[i] = gl_mul(tw_get(T, logR, r * k, false), grp);
    } else {
        // ntt_pass_a_cos2: [c][r] = 7^(16 C r) w_(16 beta)^(c r)
        const u64 q = i - L.cos2_scal();
        const u64 c = q >> 4, r = q & 15;
        out[i] = gl_mul(T.pow7[(16 * r) << logC], tw_get(T, 4 + logbeta, (c * r) & ((1ULL << (4 + logbeta)) - 1), false));
    }
}
// the pass tables alone (forward, for sizes without a four-step table; pass_tables_size entries)
static void build_pass_tables(u64* out, int logn, int logbeta, const Tables& T, hipStream_t s) {
    const PassTableLayout L = pass_table_layout(logn, logbeta);
    XFG_LAUNCH(pass_tables_kernel, dim3((unsigned)((L.total() + 255) / 256)), dim3(256), 0, s, out, L, T);
}
// the four-step table with its pass tables behind it (fourstep_size entries)
static void build_fourstep(u64* out, int logn, int logbeta, const Tables& T, hipStream_t s) {
    const u64 cnt = fourstep_main(logn, logbeta);
    XFG_LAUNCH(fourstep_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, out, logn, logbeta,
               pass_table_layout(logn, logbeta).logC, gl_inv(1ULL << logn), T);
    build_pass_tables(out + cnt, logn, logbeta, T, s);
}
// four-step twiddle tables of the NTT sizes one (n, beta) proof uses: the forward LDE and the
// inverse NTTs of sizes 8 .. 2n (trace, composition, FRI remainder). Sizes whose table would exceed
// 2^FOURSTEP_MAX_LOG entries get the per-size pass tables instead (at 2^20 with the n-entry [k1][j2]
// table of ntt_pass_a_r1024: a full 2^24-entry table for configs[4] measured slower).
// Returns false when one is missing.
bool fourstep_ready(xfg_ctx* c, int logn, int logbeta) {
    const FourStep& f = c->tables.fs;
    logbeta = lde_table_logbeta(logbeta);
    const TableKind k = table_kind(logn, logbeta);
    if (k == TableKind::fourstep && !f.fwd[logn][logbeta]) return false;
    if (k == TableKind::pass_only && !f.pass_fwd[logn][logbeta]) return false;
    for (int l = 3; l <= std::min(logn + 1, FOURSTEP_MAX_LOG); l++)
        if (!f.inv[l]) return false;
    return true;
}
// caller guarantees no kernel in flight reads the registry (fresh context or drained)
void ensure_fourstep(xfg_ctx* c, int logn, int logbeta) {
    if (fourstep_ready(c, logn, logbeta)) return;
    ensure_tables(c, std::max(logn + logbeta, logn + 1));
    const Tables T = tables_of(c);
    auto build = [&](int ln, int lb) {
        DBuf<u64>& b = c->tables.four_buf[ln * 8 + lb + 1];
        b.ensure(fourstep_size(ln, lb));
        build_fourstep(b.p, ln, lb, T, 0);
        return (const u64*)b.p;
    };
    FourStep& f = c->tables.fs;
    // a composed LDE (blowup 32, 64, 128) runs on the tables of its blowup-16 sub-transforms
    logbeta = lde_table_logbeta(logbeta);
    const TableKind k = table_kind(logn, logbeta);
    if (k == TableKind::fourstep && !f.fwd[logn][logbeta]) f.fwd[logn][logbeta] = build(logn, logbeta);
    if (k == TableKind::pass_only && !f.pass_fwd[logn][logbeta]) {
        DBuf<u64>& b = c->tables.pass_buf[logn * 8 + logbeta];
        b.ensure(pass_tables_size(logn, logbeta));
        build_pass_tables(b.p, logn, logbeta, T, 0);
        f.pass_fwd[logn][logbeta] = b.p;
    }
    for (int l = 3; l <= std::min(logn + 1, FOURSTEP_MAX_LOG); l++)
        if (!f.inv[l]) f.inv[l] = build(l, -1);
    HIPCHK(hipStreamSynchronize(0));
}

}  // namespace xfg
