// Host orchestration of the MI355X burn-proof STARK prover + the C ABI (include/xfg_stark.h).
//
// Pipeline = Winterfell 0.8.3 `Prover::prove` as bound by the reference
// (src/burn_mint_air.rs:479-531, src/burn_mint_prover.rs:62-129), batched over independent
// proofs: every kernel launch covers all proofs of the batch, and the host only touches the
// serial Fiat-Shamir steps (a few BLAKE3 calls per proof per round) between launch sets.
//
// This file: the table registry, the lanes, prove_lane (one work unit: the device chain, then the
// host steps of proof_assembly.hpp), the lane scheduler and the production ABI. The debug / bench
// entry points are in debug_abi.hip, the GPU batch verifier's host side in verify_batch_gpu.hip.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "host_pool.hpp"
#include "marshal.hpp"
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

static const char* STAGE_NAMES[] = {"trace_lde",     "trace_commit", "constraint_eval", "composition",
                                    "comp_commit",   "ood",          "deep",            "fri",
                                    "queries_gather", "host_total",  "host_queries",    "host_serialize"};

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
// four-step twiddle tables of the NTT sizes one (n, beta) proof uses: the forward LDE and the
// inverse NTTs of sizes 8 .. 2n (trace, composition, FRI remainder). Sizes whose table would exceed
// 2^FOURSTEP_MAX_LOG entries get the per-size pass tables instead (at 2^20 with the n-entry [k1][j2]
// table of ntt_pass_a_r1024: a full 2^24-entry table for configs[4] measured slower).
// Returns false when one is missing.
static bool fourstep_ready(xfg_ctx* c, int logn, int logbeta) {
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


static void stage_mark(Lane* c, int k, hipStream_t on = nullptr) {
    if (c->timing) HIPCHK(hipEventRecord(c->ev[k], on ? on : c->stream));
}

// the lane's stream for the openings' gathers, at the highest stream priority (a second stream at
// the default priority measured 4-5 % slower)
// created when the lanes are (ensure_lanes, after every lane's proving stream): a high-priority stream
// costs ~10 ms to create, which a lazily created one added to the first unit every lane ran (XFG_TRACE,
// profiles/r06/host_phases.txt); lane 0 used alone (the debug / bench entry points) creates it here
static hipStream_t gather_stream(Lane* c) {
    if (!c->gstream) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
        HIPCHK(hipStreamCreateWithPriority(&c->gstream, hipStreamNonBlocking, greatest));
    }
    return c->gstream;
}

// ------------------------------------------------------------------ one work unit on a lane
void size_trace_lde(Lane* c, size_t B, const ProofShape& sh) {
    c->trace.ensure(B * 7 * sh.n);
    c->coef.ensure(B * 7 * sh.n);
    c->scratch.ensure(B * 7 * sh.N);
    c->lde.ensure(B * 7 * sh.N);
    c->const_col.ensure((B * 7 + 3) & ~(size_t)3);
}
void size_constraint_eval(Lane* c, size_t B, const ProofShape& sh) {
    c->air.ensure(B);
    c->coeffs.ensure(B * 15 * sh.DE);
    c->ce.ensure(B * sh.DE * 2 * sh.n);
}
void size_ood_deep(Lane* c, size_t B, const ProofShape& sh) {
    c->hcoef.ensure(B * sh.DE * sh.n);
    c->zpts.ensure(B * 2 * sh.DE);
    c->partial.ensure(B * 15 * sh.DE * ood_partial_count(sh.logn));
    c->ood.ensure(B * 15 * sh.DE);
    c->dp.ensure(B);
    c->carry.ensure(B * 2 * sh.DE * ood_partial_count(sh.logn));
    c->deep.ensure(B * sh.DE * sh.n);
}
// where a unit's traces come from, and what is checked on the way. p: the unit's own slice [B][7][n]
// (null: generated on the device from the AIR constants)
struct TraceSrc {
    enum Kind { GENERATED, HOST_DIRECT, HOST_STAGED, DEVICE };
    Kind kind = GENERATED;
    const u64* p = nullptr;
    bool validate = false;        // XFG_TRACE_VALIDATE: the AIR check behind the upload
    bool size_staging = false;    // grow the lane's pinned trace staging with its other buffers
    const int* refused = nullptr;  // [B] non-zero: refused at submission, the slot is proven over zeros
    u64* keys = nullptr;          // [B] out: the check kernel's words (when checks())
    // device traces are always tested for canonical cells; host traces were on the host
    bool checks() const { return validate || kind == DEVICE; }
};

// every device buffer of a unit of B proofs, and the pinned opening buffers
static void size_lane_buffers(Lane* c, size_t B, const ProofShape& sh, const Opts& o, const TraceSrc& ts) {
    const u64 n = sh.n, N = sh.N;
    const size_t DE = sh.DE;
    const unsigned nl = sh.nl;
    size_trace_lde(c, B, sh);
    size_constraint_eval(c, B, sh);
    size_ood_deep(c, B, sh);
    c->tnodes.ensure(B * 2 * n);
    c->hlde.ensure(B * DE * N);
    c->hnodes.ensure(B * 2 * n);
    c->f0.ensure(B * DE * N);
    c->alpha7.ensure(B * DE);
    c->falpha.ensure((size_t)std::max(1u, nl) * B * DE);
    c->dn2.ensure(B * DE);
    c->dcoin.ensure(B);
    c->dfail.ensure(B);
    c->droots.ensure((size_t)(2 + nl) * B);  // trace, composition, FRI layer roots: [tree][B]
    if (c->flayer.size() < nl + 1) {
        c->flayer.resize(nl + 1);
        c->fnodes.resize(nl + 1);
    }
    for (unsigned l = 0; l < nl; l++) {
        c->fnodes[l].ensure(B * 2 * (sh.D[l] / o.fold));
        c->flayer[l + 1].ensure(B * DE * sh.D[l + 1]);
    }
    c->rem.ensure(B * DE * std::max<u64>(sh.rem_len, 1));
    // opening buffers (pinned, device-mapped: the gathers read and write them directly) sized by
    // upper bounds once, so steady-state calls never re-allocate (hipHostMalloc would serialise
    // the device and the other lanes)
    const size_t q = o.q, depth = sh.logn + sh.logbeta;
    const size_t vals = B * q * (7 + DE + o.fold * DE * nl);
    size_t digs = B * q * 2 * depth;
    for (unsigned l = 0; l < nl; l++) digs += B * q * ilog2(sh.D[l] / o.fold);
    const size_t opens = B * q * 2 * 2 * 2 * sh.beta;
    c->h_idx.ensure(vals + digs + B * 2 * q);
    c->h_gv.ensure(vals);
    c->h_gd.ensure(digs + opens);
    size_grind(c, B);
    if (ts.checks()) c->tkeys.ensure(B);
    if (ts.kind == TraceSrc::HOST_STAGED || ts.size_staging) c->h_trace.ensure(B * 7 * n);
}

// the unit's small uploads are copied by a kernel from the pinned, device-mapped host blocks: no
// copy-engine transfer for the lane stream to wait on (see pack_replay_block). The lane
// rewrites these blocks only for its next unit, after this one's stream has drained.
static void upload(void* dst, const void* host, size_t bytes, hipStream_t s) {
    void* hd = nullptr;
    HIPCHK(hipHostGetDevicePointer(&hd, const_cast<void*>(host), 0));
    PackSet u;
    u.src[0] = hd;
    u.off[0] = 0;
    u.words[0] = bytes / 4;
    u.nseg = 1;
    launch_pack(u, dst, s);
}
static_assert(sizeof(AirConst) % 4 == 0 && sizeof(DevCoin) % 4 == 0, "uploads copy 32-bit words");

void size_grind(Lane* c, size_t B) {
    c->h_gseed.ensure(B);
    c->h_gnonce.ensure(B);
    c->gseed.ensure(B);
    c->gstate.ensure(grind_state_words(B));
}
Digest* grind_seeds(Lane* c, size_t B) {
    size_grind(c, B);
    return c->h_gseed.p;
}
const u64* grind_search(Lane* c, int B, unsigned grind, u64 first, u64 max_nonce, unsigned chunk_log, unsigned blocks) {
    size_grind(c, B);
    const hipStream_t s = gather_stream(c);
    void* out = nullptr;
    HIPCHK(hipHostGetDevicePointer(&out, c->h_gnonce.p, 0));
    upload(c->gseed.p, c->h_gseed.p, (size_t)B * sizeof(Digest), s);
    launch_grind(c->gseed.p, c->gstate.p, (u64*)out, (unsigned)B, grind, first, max_nonce, chunk_log, blocks, s);
    HIPCHK(hipStreamSynchronize(s));
    return c->h_gnonce.p;
}

// AIR constants and transcript seeds of the unit's proofs, on the host and on the device.
// The Fiat-Shamir steps between the commitments (coefficient, OOD point, DEEP and FRI alpha
// draws) run on the device from a copy of each proof's coin, so the whole chain from the trace
// to the FRI remainder is enqueued without a host round trip; the host replays the same
// transcript from the roots and OOD values once the chain has finished (replay_transcript).
static void upload_unit_inputs(Lane* c, ProofJob* jobs, int B, const ProofShape& sh, const Opts& o) {
    hipStream_t s = c->stream;
    AirConst* airs = c->h_air.ensure(B);
    for (int b = 0; b < B; b++) airs[b] = jobs[b].air;
    upload(c->air.p, airs, B * sizeof(AirConst), s);
    // transcript seed: Context::to_elements || public inputs (ProverChannel::new)
    DevCoin* hc = c->h_coin.ensure(B);
    for (int b = 0; b < B; b++) {
        ProofJob& j = jobs[b];
        u64 e[20];
        context_elements(sh.n, o, e);
        memcpy(e + 8, j.air.pub, 12 * 8);
        j.coin.init(e, 20);
        j.commitments.clear();
        hc[b].seed = j.coin.seed;
        hc[b].counter = j.coin.counter;
        hc[b].pad = 0;
    }
    upload(c->dcoin.p, hc, B * sizeof(DevCoin), s);
    HIPCHK(hipMemsetAsync(c->dfail.p, 0, B * sizeof(int), s));
}

void launch_trace_lde(Lane* c, const Tables& T, int B, const ProofShape& sh, bool probe) {
    hipStream_t s = c->stream;
    const unsigned char* skip = c->const_col.p;
    launch_const_detect(c->trace.p, B * 7, sh.logn, c->const_col.p, s);
    launch_interpolate(c->trace.p, sh.n, c->coef.p, sh.n, c->scratch.p, B * 7, sh.logn, false, sh.n, T, s, skip);
    if (probe) {
        if (!c->lde_ev[0]) {
            HIPCHK(hipEventCreate(&c->lde_ev[0]));
            HIPCHK(hipEventCreate(&c->lde_ev[1]));
        }
        HIPCHK(hipEventRecord(c->lde_ev[0], s));
    }
    launch_lde(c->coef.p, sh.n, c->lde.p, c->scratch.p, B * 7, sh.logn, sh.logbeta, T, s, skip);
    if (probe) HIPCHK(hipEventRecord(c->lde_ev[1], s));
    // the constant columns' coefficients and LDE planes (outside the probe's window: it times the
    // transforms of the polynomials it counts)
    launch_const_fill(skip, c->trace.p, sh.n, c->coef.p, c->lde.p, B * 7, sh.logn, sh.logbeta, s);
}

// FRI layers (FriProver::build_layers), folding factor `fold`: commit -> reseed -> draw alpha -> fold,
// every round on the device; then the remainder: interpolate the last layer over 7*<w_D>, keep
// D/blowup coefficients (with no folding layer this is the DEEP polynomial's own coefficients),
// planes [b][c][rem_len]
static void enqueue_fri_layers(Lane* c, const Tables& T, int B, const ProofShape& sh, int fold, CoinStep& cs,
                               HostTrace& ht) {
    hipStream_t s = c->stream;
    const int DE = sh.DE;
    const unsigned nl = sh.nl;
    for (unsigned l = 0; l < nl; l++) {
        const u64 rows = sh.D[l] / fold;
        const bool cm = (l == 0);
        const u64* src = cm ? c->f0.p : c->flayer[l].p;
        const u64 cstride = cm ? sh.N : sh.D[l], sstride = DE * cstride;
        cs.kind = CoinStep::FRI_ALPHA;
        cs.out = c->alpha7.p;
        cs.hist = c->falpha.p + (size_t)l * B * DE;  // the raw alpha of this layer, for the replay
        cs.root_out = c->droots.p + (size_t)(2 + l) * B;
        launch_merkle_fri(src, sstride, cstride, cm, sh.logn, sh.logbeta, rows, c->fnodes[l].p, B, DE, fold, s, cs);
        launch_fri_fold(src, sstride, cstride, cm, sh.logn, sh.logbeta, rows, (int)ilog2(sh.D[l]), c->alpha7.p,
                        c->flayer[l + 1].p, rows, T, B, DE, fold, s);
    }
    ht.mark("chain_launch");
    if (nl > 0) {
        launch_interpolate(c->flayer[nl].p, sh.D[nl], c->rem.p, sh.rem_len, c->scratch.p, B * DE,
                           (int)ilog2(sh.D[nl]), true, sh.rem_len, T, s);
    } else {
        HIPCHK(hipMemcpy2DAsync(c->rem.p, sh.rem_len * 8, c->deep.p, sh.n * 8, sh.rem_len * 8, (size_t)B * DE,
                                hipMemcpyDeviceToDevice, s));
    }
}

// transcript inputs for the host replay (trace / composition / FRI roots, OOD frame, the device's
// draws, DEEP parameters, FRI alphas, rejections, remainder, DEEP degree check): one kernel packs
// them straight into the pinned host block (device-mapped, written with plain vector stores),
// visible to the host after the lane stream's synchronisation. As eight hipMemcpyAsync blits each
// could start ~0.2 ms after the previous one (rocprof, scripts/fri_timeline.sh: 1.7 ms of idle
// stream after the last FRI fold); as one larger copy the runtime takes the SDMA engine, whose
// dependency on the lane stream cost 17 % of the pipelined throughput (same box, lib_ab.sh)
// with_keys: the trace check's word per proof rides along (units of caller-supplied traces that are checked)
static ReplayView pack_replay_block(Lane* c, size_t B, const ProofShape& sh, bool with_keys) {
    const size_t DE = sh.DE, nl = sh.nl;
    PackSet pk;
    u64 words = 0;
    auto seg = [&](const void* src, size_t bytes) {
        const u64 at = words;
        pk.src[pk.nseg] = src;
        pk.off[pk.nseg] = at;
        pk.words[pk.nseg++] = bytes / 4;
        words = (at + bytes / 4 + 63) & ~63ULL;  // 256 B aligned segments
        return at * 4;
    };
    const u64 o_roots = seg(c->droots.p, (2 + nl) * B * sizeof(Digest));
    const u64 o_ood = seg(c->ood.p, B * 15 * DE * 8);
    const u64 o_co = seg(c->coeffs.p, B * 15 * DE * 8);
    const u64 o_dp = seg(c->dp.p, B * sizeof(DeepParams));
    const u64 o_falpha = seg(c->falpha.p, nl * B * DE * 8);
    const u64 o_fail = seg(c->dfail.p, B * sizeof(int));
    const u64 o_rem = seg(c->rem.p, B * DE * sh.rem_len * 8);
    const u64 o_dn2 = seg(c->dn2.p, B * DE * 8);
    const u64 o_const = seg(c->const_col.p, (B * 7 + 3) & ~(size_t)3);  // whole words; B * 7 flags
    const u64 o_keys = with_keys ? seg(c->tkeys.p, B * 8) : 0;
    unsigned char* hx = c->h_xfer.ensure(words * 4);
    void* hx_dev = nullptr;
    HIPCHK(hipHostGetDevicePointer(&hx_dev, hx, 0));
    launch_pack(pk, hx_dev, c->stream);
    ReplayView rv;
    rv.roots = (const Digest*)(hx + o_roots);
    rv.ood = (const u64*)(hx + o_ood);
    rv.co = (const u64*)(hx + o_co);
    rv.dps = (const DeepParams*)(hx + o_dp);
    rv.falpha = (const u64*)(hx + o_falpha);
    rv.ffail = (const int*)(hx + o_fail);
    rv.remh = (const u64*)(hx + o_rem);
    rv.dn2h = (const u64*)(hx + o_dn2);
    c->h_const_col = hx + o_const;
    c->h_tkeys = with_keys ? (const u64*)(hx + o_keys) : nullptr;
    return rv;
}

// the whole device chain of a unit, trace to FRI remainder and the replay block, enqueued on the
// lane stream without a host round trip. g: the trace domain generator
static ReplayView enqueue_commit_chain(Lane* c, const Tables& T, const u64* ce_div, ProofJob* jobs, int B,
                                       const TraceSrc& ts, const ProofShape& sh, const Opts& o, u64 g,
                                       HostTrace& ht) {
    const u64 n = sh.n;
    const int logn = sh.logn, logbeta = sh.logbeta, DE = sh.DE;
    hipStream_t s = c->stream;
    upload_unit_inputs(c, jobs, B, sh, o);
    // ---- 1. trace LDE + commitment (DefaultTraceLde::new)
    ht.mark("setup");
    stage_mark(c, 0);
    const size_t tbytes = (size_t)7 * n * 8;  // one proof's trace
    switch (ts.kind) {
        case TraceSrc::GENERATED: launch_trace_gen(c->air.p, c->trace.p, logn, B, s); break;
        case TraceSrc::HOST_DIRECT:  // xfg_prove_trace: one trace, straight from the caller's memory
            HIPCHK(hipMemcpyAsync(c->trace.p, ts.p, B * tbytes, hipMemcpyHostToDevice, s));
            break;
        case TraceSrc::HOST_STAGED: {
            // into the lane's pinned staging (the stream has drained: the last unit's upload is over),
            // then one asynchronous DMA; a proof refused at submission (cell >= p) is staged as zeros
            u64* st = c->h_trace.p;
            const u64* src = ts.p;
            const int* refused = ts.refused;
            host_pool().parallel_for(B, [st, src, refused, n, tbytes](int b) {
                if (refused[b]) memset(st + (size_t)b * 7 * n, 0, tbytes);
                else memcpy(st + (size_t)b * 7 * n, src + (size_t)b * 7 * n, tbytes);
            });
            HIPCHK(hipMemcpyAsync(c->trace.p, st, B * tbytes, hipMemcpyHostToDevice, s));
            break;
        }
        case TraceSrc::DEVICE:
            HIPCHK(hipMemcpyAsync(c->trace.p, ts.p, B * tbytes, hipMemcpyDeviceToDevice, s));
            break;
    }
    if (ts.checks()) launch_trace_check(c->trace.p, c->air.p, c->tkeys.p, logn, B, ts.validate, s);
    launch_trace_lde(c, T, B, sh, c->lde_probe);
    stage_mark(c, 1);
    // ---- 2. trace root -> constraint composition coefficients (7 transition + 8 boundary)
    CoinStep cs;
    cs.ext = DE;
    cs.coins = c->dcoin.p;
    cs.fail = c->dfail.p;
    cs.kind = CoinStep::COEFFS;
    cs.out = c->coeffs.p;
    cs.root_out = c->droots.p;
    launch_merkle_lde(c->lde.p, 7, c->tnodes.p, B, logn, logbeta, s, cs);
    stage_mark(c, 2);
    // ---- 3. constraint evaluation + composition polynomial + commitment
    launch_constraint_eval(c->lde.p, c->air.p, c->coeffs.p, ce_div, c->ce.p, logn, logbeta, B, DE, s);
    stage_mark(c, 3);
    launch_interpolate(c->ce.p, 2 * n, c->hcoef.p, n, c->scratch.p, B * DE, logn + 1, true, n, T, s);
    launch_lde(c->hcoef.p, n, c->hlde.p, c->scratch.p, B * DE, logn, logbeta, T, s);
    stage_mark(c, 4);
    // ---- 4. composition root -> OOD point (z, z g); the frame, then the DEEP draws
    cs.kind = CoinStep::OOD_POINT;
    cs.out = c->zpts.p;
    cs.root_out = c->droots.p + B;
    cs.g = g;
    launch_merkle_lde(c->hlde.p, DE, c->hnodes.p, B, logn, logbeta, s, cs);
    stage_mark(c, 5);
    DeepCoinStep dc;
    dc.coins = c->dcoin.p;
    dc.fail = c->dfail.p;
    dc.zpts = c->zpts.p;
    dc.dp = c->dp.p;
    dc.ginv = gl_inv(g);
    launch_ood(c->coef.p, c->hcoef.p, c->zpts.p, c->partial.p, c->ood.p, logn, B, DE, s, dc);
    stage_mark(c, 6);
    // ---- 5. DEEP composition polynomial (coefficient form) + its LDE
    launch_deep(c->coef.p, c->hcoef.p, c->dp.p, c->partial.p, c->carry.p, c->deep.p, logn, B, DE, s);
    launch_lde(c->deep.p, n, c->f0.p, c->scratch.p, B * DE, logn, logbeta, T, s);
    // degree check: deg(DEEP) == n - 2  <=>  coefficient n-2 != 0 (coefficient n-1 is 0 by construction)
    HIPCHK(hipMemcpy2DAsync(c->dn2.p, 8, c->deep.p + (n - 2), n * 8, 8, (size_t)B * DE, hipMemcpyDeviceToDevice, s));
    stage_mark(c, 7);
    // ---- 6. FRI layers and remainder, then the replay's inputs
    enqueue_fri_layers(c, T, B, sh, (int)o.fold, cs, ht);
    const ReplayView rv = pack_replay_block(c, B, sh, ts.checks());
    stage_mark(c, 8);
    ht.mark("launch_rem");
    return rv;
}

// the unit's openings: the indices go to, and the opened values and digests come back in, the
// pinned host blocks directly (device-mapped): no copy-engine transfers whose completion the stream
// would wait on (one larger D2H on the SDMA engine cost 17 % of the pipelined throughput).
// The gathers (a few hundred microseconds of small kernels) go to the lane's high-priority stream:
// on its own stream a lane's gathers queued behind the other lanes' chains in the shared hardware
// queue (XFG_TRACE: 3.1 ms mean, 9 ms p90 to sync them); the lane's stream has drained, so they
// need no event. Timing mode takes the same stream: stage 9 is measured from the lane stream's
// last event to an event behind the gathers' copies on this one
struct Gathered {
    const u64* gv;     // values, the segments of OpeningIndex end to end
    const Digest* gd;  // stored digests, then the recomputed subtrees (trace tree, composition tree)
};
static Gathered enqueue_gathers(Lane* c, const ProofShape& sh, const OpeningIndex& ix, HostTrace& ht) {
    const size_t nvals = ix.nvals, ndig = ix.ndig, nent = ix.nent, nopen = nent * 2 * sh.beta;
    u64* hidx = c->h_idx.ensure(ix.allidx.size());
    memcpy(hidx, ix.allidx.data(), ix.allidx.size() * 8);
    u64* gv = c->h_gv.ensure(nvals);
    Digest* gd = c->h_gd.ensure(ndig + 2 * nopen);
    void *didx = nullptr, *dgv = nullptr, *dgd = nullptr;
    HIPCHK(hipHostGetDevicePointer(&didx, hidx, 0));
    HIPCHK(hipHostGetDevicePointer(&dgv, gv, 0));
    HIPCHK(hipHostGetDevicePointer(&dgd, gd, 0));
    const u64* gidx = (const u64*)didx;
    u64* gval = (u64*)dgv;
    Digest* gdig = (Digest*)dgd;
    ht.mark("q_idx_host");
    const hipStream_t sq = gather_stream(c);
    ht.mark("q_h2d");
    // the segments lie end to end in allidx: values first, then digests
    GatherSet gs;
    size_t vo = 0, dof = 0, gbase = 0;  // gbase: index entries consumed by launches already made
    auto add = [&](const void* src, void* dst, bool dig, size_t cnt) {
        if (gs.nseg == GatherSet::MAX) {  // very deep FRI: flush and continue in a new launch
            launch_gather_set(gs, gidx + gbase, sq);
            gbase += gs.first[gs.nseg];
            gs = GatherSet{};
        }
        gs.src[gs.nseg] = src;
        gs.dst[gs.nseg] = dst;
        gs.digest[gs.nseg] = dig ? 1 : 0;
        gs.first[gs.nseg + 1] = gs.first[gs.nseg] + cnt;
        gs.nseg++;
    };
    const u64* vsrc[2] = {c->lde.p, c->hlde.p};
    for (size_t k = 0; k < ix.vseg.size(); k++) {
        const u64* src = k < 2 ? vsrc[k] : (k == 2 ? c->f0.p : c->flayer[k - 2].p);
        add(src, gval + vo, false, ix.vseg[k].second);
        vo += ix.vseg[k].second;
    }
    for (size_t k = 0; k < ix.dseg.size(); k++) {
        const Digest* src = k == 0 ? c->tnodes.p : (k == 1 ? c->hnodes.p : c->fnodes[k - 2].p);
        add(src, gdig + dof, true, ix.dseg[k].second);
        dof += ix.dseg[k].second;
    }
    launch_gather_set(gs, gidx + gbase, sq);
    const u64* ent = gidx + nvals + ndig;
    launch_open_rows(c->lde.p, 7, ent, nent, gdig + ndig, sh.logn, sh.logbeta, sq);
    launch_open_rows(c->hlde.p, sh.DE, ent, nent, gdig + ndig + nopen, sh.logn, sh.logbeta, sq);
    ht.mark("q_launch");
    stage_mark(c, 9, sq);
    return Gathered{gv, gd};
}

// the batched prover: jobs[i].air filled; trace_host optional ([B][7][n], else generated on device).
// Device chain -> host transcript replay -> opening plans -> gathers -> serialisation; the per-proof
// host steps (proof_assembly.hpp) are independent and spread over the host pool
static void prove_lane(Lane* c, const Tables& T, const u64* ce_div, ProofJob* jobs, int B, const TraceSrc& ts,
                       u64 n, const Opts& o) {
    using clk = std::chrono::steady_clock;
    const auto t_host0 = clk::now();
    HostTrace ht;
    ht.mark("start");
    const ProofShape sh(n, o);
    const u64 g = gl_root(sh.logn);
    HostPool& pool = host_pool();

    size_lane_buffers(c, B, sh, o, ts);
    const ReplayView rv = enqueue_commit_chain(c, T, ce_div, jobs, B, ts, sh, o, g, ht);
    HIPCHK(hipStreamSynchronize(c->stream));
    ht.mark("sync_rem");
    // trace columns that went through the NTTs (the rest were constant: detected, filled in)
    u64 live_cols = 0;
    for (int k = 0; k < B * 7; k++) live_cols += c->h_const_col[k] ? 0 : 1;
    pool.parallel_for(B, [jobs, B, &sh, g, &rv](int b) { replay_transcript(jobs[b], b, B, sh, g, rv); });

    const auto t_q0 = clk::now();
    // ---- 7. grinding + query positions, gather lists: every proof's plan is built on its own into
    // per-proof index lists, which are then laid end to end
    std::vector<LaneLayout>& lay = c->hs.lay;
    if (lay.size() < (size_t)B) lay.resize(B);
    if (o.grind < GRIND_DEVICE_MIN) {
        pool.parallel_for(B, [jobs, &sh, &o, &rv, &lay](int b) { plan_queries(jobs[b], b, sh, o, rv, lay[b]); });
        c->grind_host += (u64)B;
    } else {
        // plan_queries with the device's search in the place of the host's: remainder commitments on the
        // pool, the unit's B seeds to the device, one launch on the gather stream, each nonce checked with
        // one hash, then the openings on the pool
        pool.parallel_for(B, [jobs, &sh, &rv, &lay](int b) { plan_commit_remainder(jobs[b], b, sh, rv, lay[b]); });
        Digest* seeds = grind_seeds(c, B);
        for (int b = 0; b < B; b++) seeds[b] = jobs[b].coin.seed;
        const GrindPlan gp = grind_plan((unsigned)o.grind, (uint32_t)B, (unsigned)c->cus);
        const u64* nonces = grind_search(c, B, (unsigned)o.grind, 1, gp.max_nonce, gp.chunk_log, gp.blocks);
        ht.mark("grind");
        for (int b = 0; b < B; b++) {
            if (nonces[b] == 0) {  // no nonce up to max_nonce (probability e^-256): this proof fails, the others go on
                jobs[b].status = XFG_PROVER_ERROR;
                jobs[b].pow_exhausted = true;
            } else if (nonces[b] > gp.max_nonce || pow_zeros(jobs[b].coin.seed, nonces[b]) < o.grind) {
                throw std::runtime_error("device / host transcript diverged");
            }
        }
        pool.parallel_for(B, [jobs, &sh, &o, nonces, &lay](int b) { plan_openings(jobs[b], b, sh, o, nonces[b], lay[b]); });
        c->grind_dev += (u64)B;
    }
    ht.mark("queries_plan");
    OpeningIndex& ix = c->hs.ix;
    concat_indices(lay, B, sh, ix);
    const Gathered got = enqueue_gathers(c, sh, ix, ht);
    const auto t_q1 = clk::now();
    ht.mark("queries_host");
    HIPCHK(hipStreamSynchronize(c->gstream));
    ht.mark("sync_gather");
    const auto t_s0 = clk::now();

    // ---- 8. StarkProof::to_bytes, one proof per pool task
    pool.parallel_for(B, [jobs, B, &sh, &o, &lay, &ix, got](int b) {
        serialize_proof(jobs[b], b, B, sh, o, lay[b], ix, got.gv, got.gd);
    });
    ht.mark("serialize");
    // caller-supplied traces: what the check found, or the refusal at submission, is the proof's status
    // whatever the chain made of the slot (an invalid trace usually fails the DEEP degree check too)
    for (int b = 0; b < B && ts.kind != TraceSrc::GENERATED; b++) {
        const u64 key = c->h_tkeys ? c->h_tkeys[b] : TRACE_KEY_VALID;
        const bool refused = ts.refused && ts.refused[b];  // its key word was written at submission
        if (ts.keys && !refused) ts.keys[b] = key;
        if (refused) jobs[b].status = ts.refused[b];
        else if (key != TRACE_KEY_VALID)
            jobs[b].status = (key >> 62) == TRACE_KEY_NONCANONICAL ? XFG_INVALID_ARGUMENT : XFG_INVALID_TRACE;
    }
    ht.dump(B, (long)((u64)B * 7 - live_cols));
    if (c->lde_probe) {  // the stream has passed both events (root / query fetches synchronised it)
        float ms = 0;
        HIPCHK(hipEventSynchronize(c->lde_ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, c->lde_ev[0], c->lde_ev[1]));
        c->lde_ms += ms;
        c->lde_sets++;
        c->lde_polys += live_cols;
    }
    if (c->timing) {
        for (int k = 0; k < 9; k++) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, c->ev[k], c->ev[k + 1]));
            c->stage_ms[k] = ms;
        }
        const auto t_end = clk::now();
        c->stage_ms[ST_HOST] = std::chrono::duration<double, std::milli>(t_end - t_host0).count();
        c->stage_ms[ST_HQUERY] = std::chrono::duration<double, std::milli>(t_q1 - t_q0).count();
        c->stage_ms[ST_HSER] = std::chrono::duration<double, std::milli>(t_end - t_s0).count();
    }
}

// a lane's proving stream (default priority: graded or high lane priorities measured equal or worse)
// and events
static void create_lane_stream(xfg_ctx* c, Lane* L) {
    L->lde_probe = c->lde_probe;
    HIPCHK(hipDeviceGetAttribute(&L->cus, hipDeviceAttributeMultiprocessorCount, c->device));
    HIPCHK(hipStreamCreateWithFlags(&L->stream, hipStreamNonBlocking));
    for (auto& e : L->ev) HIPCHK(hipEventCreate(&e));
}
Lane* lane0(xfg_ctx* c) {
    if (c->lanes.empty()) {
        c->lanes.emplace_back(new Lane());
        create_lane_stream(c, c->lanes[0].get());
    }
    return c->lanes[0].get();
}
// every lane's proving stream first, then the gather streams: streams take the process's hardware
// queues (GPU_MAX_HW_QUEUES, 4) in creation order, and a gather stream created between two lanes'
// proving streams left the proving streams two of the four queues (-9 % burn-proofs/s,
// profiles/r06/gather_stream_ab.txt)
static void ensure_lanes(xfg_ctx* c, size_t k) {
    lane0(c);
    while (c->lanes.size() < k) {
        c->lanes.emplace_back(new Lane());
        create_lane_stream(c, c->lanes.back().get());
    }
    for (auto& L : c->lanes) gather_stream(L.get());
}
// lane / work-unit tuning knobs (XFG_LANES, XFG_UNIT)
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// ------------------------------------------------------------------ batch submission / lane workers
// a submitted batch: jobs [0, B) proven in units of XFG_UNIT proofs by the lane workers; proof
// bytes are copied into the caller's buffers on the worker thread as each unit finishes
struct Batch {
    std::vector<ProofJob> jobs;
    std::vector<uint32_t> which;   // jobs[k] -> caller index
    std::vector<uint8_t*> outs;    // caller buffers (null entry or empty: size query)
    size_t* out_lens = nullptr;    // caller capacities in, proof lengths out
    int* statuses = nullptr;       // caller statuses, written by wait
    std::vector<int> st;           // per-job copy-out status
    // caller-supplied traces [jobs][7][n] (job k <-> caller index k: such a batch keeps refused proofs
    // as jobs so that every unit's slice stays at b0 * 7 * n); trace.p is the batch's base
    TraceSrc trace;
    std::vector<int> refused;          // per job: status set at submission (cell >= p), else 0
    std::vector<u64> keys;             // per job: the trace check's word
    xfg_trace_fault* faults = nullptr;  // caller's, filled by wait (may be null)
    u64 n = 0;
    Opts o{};
    Tables T{};
    const u64* ce_div = nullptr;
    int units_left = 0;
    std::exception_ptr err;
};
}  // namespace xfg

xfg_ctx::~xfg_ctx() = default;  // here, where Batch (xfg_ctx::pending) is complete

namespace xfg {

static int max_lanes() {
    static const int v = std::max(1, env_int("XFG_LANES", 7));
    return v;
}
// 32 proofs per unit: a 64-proof batch is two units. Same box, 3 x 20 steps at bench.py's depth 6:
// 12,069 +- 70 burn-proofs/s against 11,890 +- 50 with 22, 11,645 with 64, 11,557 with 16. (At depth
// 3 the unit queue ran dry and smaller units won: 22 gave 11,400 against 10,790 with 32; with the
// transcript's host round trips still in place 20 had been best.)
static int unit_size() {
    static const int v = std::max(1, env_int("XFG_UNIT", 32));
    return v;
}
// past blowup 16 a unit holds 16 / beta as many proofs, so that a lane's device workspace (the LDE buffers
// and their scratch, the twisted coefficients of the composed LDE among it) grows no faster than at blowup
// 16. Scheduling only: the unit size plays no part in the proof bytes
static int unit_size(u64 beta) { return beta > 16 ? std::max(1, (int)(unit_size() * 16 / beta)) : unit_size(); }

// smallest unit a queued unit is split into when lanes would otherwise idle (0: never split).
// 16 (a 32-proof unit splits once): with the host tail on the pool, same box, 4 interleaved 20-step
// bench runs each: 16 -> 12,725, 0 -> 12,675, 12 -> 12,576, 8 -> 12,575 burn-proofs/s (8 cut the
// first batch of a window into 8 pieces for 7 lanes)
static int split_min() {
    static const int v = std::max(0, env_int("XFG_SPLIT_MIN", 16));
    return v;
}

static void copy_unit(Batch* b, int b0, int b1) {
    host_pool().parallel_for(b1 - b0, [&](int i0) {
        const int k = b0 + i0;
        ProofJob& j = b->jobs[k];
        if (j.status) {
            b->st[k] = j.status;
            if (j.status == XFG_INVALID_TRACE) {  // no proof: whatever the slot's chain produced is dropped
                b->out_lens[b->which[k]] = 0;
                std::vector<uint8_t>().swap(j.bytes);
            }
            return;
        }
        if (b->which.empty()) {  // warm-up batch (xfg_prepare): bytes discarded
            std::vector<uint8_t>().swap(j.bytes);
            return;
        }
        uint32_t i = b->which[k];
        size_t need = j.bytes.size();
        uint8_t* dst = b->outs.empty() ? nullptr : b->outs[i];
        if (!dst) {
            b->st[k] = XFG_OK;  // size query (copy_out semantics)
        } else if (b->out_lens[i] >= need) {
            memcpy(dst, j.bytes.data(), need);
            b->st[k] = XFG_OK;
        } else {
            b->st[k] = XFG_BUFFER_TOO_SMALL;
        }
        b->out_lens[i] = need;
        std::vector<uint8_t>().swap(j.bytes);
    });
}

static void worker_main(xfg_ctx* c, int l) {
    (void)hipSetDevice(c->device);
    Lane* L = c->lanes[l].get();
    for (;;) {
        Unit u;
        bool skip;
        {
            std::unique_lock<std::mutex> g(c->qm);
            std::deque<Unit>::iterator it;
            auto pick = [&] {
                for (it = c->q.begin(); it != c->q.end(); ++it)
                    if (it->lane < 0 || it->lane == l) return true;
                return false;
            };
            c->idle++;
            c->qcv.wait(g, [&] { return c->stop || pick(); });
            c->idle--;
            if (c->stop) return;
            u = *it;
            c->q.erase(it);
            skip = (bool)u.b->err;  // a failed batch drops its remaining units
            L->timing = c->timing;
            // fewer queued units than idle lanes (the end of a run of batches, or a lone batch):
            // halve this unit until every idle lane has a share, the halves at the queue's front
            if (u.lane < 0 && !c->timing && !skip && split_min() > 0) {
                int avail = 0;
                for (auto& x : c->q) avail += x.lane < 0;
                bool pushed = false;
                while (u.b1 - u.b0 >= 2 * split_min() && avail < c->idle) {
                    const int mid = u.b0 + (u.b1 - u.b0) / 2;
                    c->q.push_front(Unit{u.b, mid, u.b1, -1});
                    u.b->units_left++;
                    u.b1 = mid;
                    avail++;
                    pushed = true;
                }
                if (pushed) c->qcv.notify_all();
            }
        }
        Batch* b = u.b;
        std::exception_ptr e;
        if (!skip) {
            try {
                // the unit's own slice of the batch's traces, refusals and key words (halved units too)
                TraceSrc ts = b->trace;
                if (ts.p) ts.p += (size_t)u.b0 * 7 * b->n;
                if (!b->refused.empty()) ts.refused = b->refused.data() + u.b0;
                if (!b->keys.empty()) ts.keys = b->keys.data() + u.b0;
                prove_lane(L, b->T, b->ce_div, b->jobs.data() + u.b0, u.b1 - u.b0, ts, b->n, b->o);
                copy_unit(b, u.b0, u.b1);
            } catch (...) {
                e = std::current_exception();
            }
        }
        std::lock_guard<std::mutex> g(c->qm);
        if (e && !b->err) b->err = e;
        c->last_lane = l;
        if (--b->units_left == 0) c->dcv.notify_all();
    }
}

static void ensure_workers(xfg_ctx* c) {
    const int nl = max_lanes();
    ensure_lanes(c, nl);
    while ((int)c->workers.size() < nl) {
        int l = (int)c->workers.size();
        c->workers.emplace_back(worker_main, c, l);
    }
}

// blocks until no submitted unit is queued or running (tables may only be replaced then)
static void drain(xfg_ctx* c) {
    std::unique_lock<std::mutex> g(c->qm);
    c->dcv.wait(g, [&] {
        for (auto& kv : c->pending)
            if (kv.second->units_left) return false;
        return true;
    });
}

static void bind_tables(xfg_ctx* c, Batch* b) {
    const int LM = (int)(ilog2(b->n) + ilog2(b->o.beta));
    if (c->tables.LM < LM || !fourstep_ready(c, (int)ilog2(b->n), (int)ilog2(b->o.beta))) {
        drain(c);
        ensure_tables(c, LM);
        ensure_fourstep(c, (int)ilog2(b->n), (int)ilog2(b->o.beta));
    }
    b->T = tables_of(c);
    b->ce_div = ensure_ce_table(c, (int)ilog2(b->n));
}

// units of unit_size(beta) proofs (the whole batch as one unit in timing mode, so the per-stage
// times describe one launch set of the batch)
static std::vector<Unit> split_units(xfg_ctx* c, int B, u64 beta) {
    std::vector<Unit> u;
    const int U = c->timing ? std::max(1, B) : unit_size(beta);
    for (int b0 = 0; b0 < B; b0 += U) u.push_back(Unit{nullptr, b0, std::min(B, b0 + U), -1});
    return u;
}

static uint64_t enqueue(xfg_ctx* c, std::unique_ptr<Batch> bp, std::vector<Unit> units) {
    ensure_workers(c);
    Batch* b = bp.get();
    b->st.assign(b->jobs.size(), XFG_OK);
    std::lock_guard<std::mutex> g(c->qm);
    uint64_t t = c->next_ticket++;
    b->units_left = (int)units.size();
    c->pending[t] = std::move(bp);
    for (auto& u : units) {
        u.b = b;
        c->q.push_back(u);
    }
    c->qcv.notify_all();
    return t;
}

static std::unique_ptr<Batch> wait_batch(xfg_ctx* c, uint64_t t) {
    std::unique_lock<std::mutex> g(c->qm);
    auto it = c->pending.find(t);
    if (it == c->pending.end()) return nullptr;
    Batch* b = it->second.get();
    c->dcv.wait(g, [&] { return b->units_left == 0; });
    std::unique_ptr<Batch> bp = std::move(it->second);
    c->pending.erase(it);
    return bp;
}

bool busy(xfg_ctx* c) {
    std::lock_guard<std::mutex> g(c->qm);
    return !c->pending.empty();
}

static const char* prover_error_text(const ProofJob& j) {
    return j.pow_exhausted ? "Prover error: proof-of-work search exhausted"
                           : "Prover error: proof generation failed (degenerate transcript or DEEP degree)";
}

// the trace check's word (trace_key, kernels.hpp) as the C ABI reports it; cell(column, step) fetches
// that cell of the proof's trace as the caller holds it
template <class Cell>
static xfg_trace_fault decode_trace_key(u64 key, const AirConst& A, Cell cell) {
    xfg_trace_fault f{};
    if (key == TRACE_KEY_VALID) return f;
    const unsigned kind = (unsigned)(key >> 62), idx = (unsigned)(key & 7);
    f.step = (key << 2) >> 5;
    if (kind == TRACE_KEY_TRANSITION) {
        f.kind = 2;
        f.index = idx;
        return f;
    }
    if (kind == TRACE_KEY_ASSERTION) {
        const u64 asserted[8] = {A.pub[0], A.pub[1], A.pub[2], A.pub[3], 0, A.nullifier, A.commitment, AIR_LAST_STATE};
        f.kind = 1;
        f.index = idx;
        f.column = idx < 7 ? idx : 4;
        f.expected = asserted[idx];
    } else {
        f.kind = 3;
        f.column = idx;
    }
    f.found = cell(f.column, f.step);
    return f;
}
// Trace::validate's panic messages (winter-air 0.8)
static std::string trace_fault_text(const xfg_trace_fault& f) {
    if (f.kind == 1)
        return "trace does not satisfy assertion main_trace(" + std::to_string(f.column) + ", " +
               std::to_string(f.step) + ") == " + std::to_string(f.expected);
    if (f.kind == 2)
        return "main transition constraint " + std::to_string(f.index) + " did not evaluate to ZERO at step " +
               std::to_string(f.step);
    return f.kind == 3 ? "trace element is not a canonical field element" : "";
}
// one cell of a caller's trace buffer (host memory, or device memory of the current device)
static u64 fetch_cell(const u64* traces, bool on_device, size_t at) {
    if (!on_device) return traces[at];
    u64 v = 0;
    HIPCHK(hipMemcpy(&v, traces + at, 8, hipMemcpyDeviceToHost));
    return v;
}

}  // namespace xfg

using namespace xfg;

extern "C" {

xfg_ctx* xfg_ctx_create(int device_id) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return nullptr;
    if (hipSetDevice(device_id) != hipSuccess) return nullptr;
    xfg_ctx* c = new xfg_ctx();
    c->device = device_id;
    try {
        lane0(c);
    } catch (...) {
        delete c;
        return nullptr;
    }
    return c;
}

void xfg_ctx_destroy(xfg_ctx* c) {
    if (!c) return;
    drain(c);
    {
        std::lock_guard<std::mutex> g(c->qm);
        c->stop = true;
        c->qcv.notify_all();
    }
    for (auto& t : c->workers) t.join();
    (void)hipSetDevice(c->device);
    c->lanes.clear();  // each lane synchronises its two streams, then frees its buffers
    delete c;          // the tables and the verifier workspace
}

int xfg_default_options(xfg_options* o) {
    if (!o) return XFG_INVALID_ARGUMENT;
    // ProofOptions::new(42, 8, 4, FieldExtension::None, 8, 31) -- src/burn_mint_prover.rs:28-35
    *o = xfg_options{42, 8, 4, 1, 8, 31};
    return XFG_OK;
}

int xfg_last_error(const xfg_ctx* c, char* buf, size_t len) {
    if (!c) return XFG_INVALID_ARGUMENT;
    if (buf && len) {
        size_t k = std::min(len - 1, c->err.size());
        memcpy(buf, c->err.data(), k);
        buf[k] = 0;
    }
    return (int)c->err.size();
}

// the largest proof serialize_proof emits for (n, options): proof_size_bound
size_t xfg_proof_size_bound(uint64_t n, const xfg_options* opts) {
    if (!opts || !is_pow2(n)) return 0;
    Opts o = to_opts(opts);
    if (o.fold < 2 || !is_pow2(o.fold) || o.beta == 0 || !is_pow2(o.beta)) return 0;
    // no blowup above 128; past 16 the LDE domain is limited (check_options)
    if (o.beta > 128 || wide_lde_too_large(n, o.beta)) return 0;
    return proof_size_bound(ProofShape(n, o), o);
}

int xfg_burn_air_consts(const xfg_burn_inputs* in, xfg_air_consts* out) {
    if (!in || !out) return XFG_INVALID_ARGUMENT;
    AirConst a;
    std::string err;
    int st = marshal(in, a, err);
    if (st) return st;
    memcpy(out->pub_inputs, a.pub, sizeof a.pub);
    out->nullifier = a.nullifier;
    out->commitment = a.commitment;
    return XFG_OK;
}

// options the prover takes, and a kernel for every NTT the proof will run: the forward LDE of size n
// and the inverse NTTs of the trace (n), the composition (2n) and the FRI remainder (D[nl])
static int check_request(xfg_ctx* c, u64 n, const Opts& o) {
    if (const char* m = check_options(n, o)) {
        c->err = std::string("Prover error: ") + m;
        if (!strcmp(m, WIDE_LDE_REFUSAL))  // the last rule: n and beta have passed theirs
            c->err = "Prover error: trace length " + std::to_string(n) + " at blowup factor " + std::to_string(o.beta) +
                     " is an LDE domain of " + std::to_string(n * o.beta) + " points; blowup factors above 16 are limited to " +
                     std::to_string(WIDE_LDE_MAX) + " (2^24)";
        return XFG_PROVER_ERROR;
    }
    const ProofShape sh(n, o);
    // a last layer smaller than the blowup leaves the remainder no coefficient (last_layer_below_blowup:
    // folding factors 2, 4, 16, and every factor past blowup 16)
    if (last_layer_below_blowup(n, o)) {
        c->err = "Prover error: folding factor " + std::to_string(o.fold) + " takes the " + std::to_string(sh.N) +
                 "-point LDE domain down to a last FRI layer of " + std::to_string(sh.D[sh.nl]) +
                 ", smaller than the blowup factor " + std::to_string(sh.beta) + ": the remainder would be empty";
        return XFG_PROVER_ERROR;
    }
    const u64 rem = sh.nl > 0 ? sh.D[sh.nl] : 0;  // size the FRI remainder is interpolated at
    const char* what = nullptr;
    u64 size = 0;
    if (!lde_supported(sh.logn, sh.logbeta) || !ntt_supported(sh.logn, 0, true)) what = "", size = n;
    else if (!ntt_supported(sh.logn + 1, 0, true)) what = "", size = 2 * n;
    else if (sh.nl > 0 && !ntt_supported((int)ilog2(rem), 0, true)) what = " (the FRI remainder)", size = rem;
    if (!what) return XFG_OK;
    c->err = "Prover error: these options need an NTT of size " + std::to_string(size) + what +
             ", which this prover has no kernel for";
    return XFG_PROVER_ERROR;
}

int xfg_prove_trace(xfg_ctx* c, const uint64_t* trace, uint32_t width, uint64_t n, const xfg_air_consts* air,
                    const xfg_options* opts, uint8_t* out, size_t* out_len) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!trace || !air || !opts || !out_len) {
        c->err = "null argument";
        return XFG_INVALID_ARGUMENT;
    }
    if (width != 7) {
        c->err = "XfgBurnMintAir traces have 7 columns";
        return XFG_INVALID_ARGUMENT;
    }
    Opts o = to_opts(opts);
    if (int st = check_request(c, n, o)) return st;
    if (!all_canonical(trace, 7 * n)) {
        c->err = "trace element is not a canonical field element";
        return XFG_INVALID_ARGUMENT;
    }
    if (!air_canonical(air)) {  // the constraint kernel subtracts them from trace values
        c->err = "AIR constant is not a canonical field element";
        return XFG_INVALID_ARGUMENT;
    }
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        std::unique_ptr<Batch> bp(new Batch());
        bp->jobs.resize(1);
        bp->jobs[0].air = air_of(air);
        bp->which = {0};
        bp->outs = {out};
        bp->out_lens = out_len;
        bp->trace.kind = TraceSrc::HOST_DIRECT;
        bp->trace.p = trace;
        bp->n = n;
        bp->o = o;
        bind_tables(c, bp.get());
        std::unique_ptr<Batch> b = wait_batch(c, enqueue(c, std::move(bp), {Unit{nullptr, 0, 1, -1}}));
        if (b->err) std::rethrow_exception(b->err);
        if (b->st[0] == XFG_PROVER_ERROR) {
            c->err = prover_error_text(b->jobs[0]);
        } else if (b->st[0] == XFG_BUFFER_TOO_SMALL) {
            c->err = "output buffer too small";
        }
        return b->st[0];
    });
}

int xfg_prove_batch_submit(xfg_ctx* c, uint32_t count, const xfg_burn_inputs* inputs, uint64_t trace_length,
                           const xfg_options* opts, uint8_t* const* outs, size_t* out_lens, int* statuses,
                           uint64_t* ticket) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!inputs || !opts || !out_lens || !statuses || !ticket || count == 0) {
        c->err = count == 0 ? "empty batch" : "null argument";
        return XFG_INVALID_ARGUMENT;
    }
    *ticket = 0;
    u64 n = trace_length ? trace_length : 64;
    Opts o = to_opts(opts);
    if (int st = check_request(c, n, o)) return st;
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        std::unique_ptr<Batch> bp(new Batch());
        // validation + marshalling (three Keccak-256 per proof) per input on the host pool: the
        // submitting thread is the start of every batch's latency
        std::vector<AirConst> airs(count);
        std::vector<std::string> errs(count);
        host_pool().parallel_for((int)count, [&](int i) { statuses[i] = marshal(&inputs[i], airs[i], errs[i]); });
        for (uint32_t i = 0; i < count; i++) {
            if (statuses[i]) {
                c->err = errs[i];
                continue;
            }
            bp->jobs.emplace_back();
            bp->jobs.back().air = airs[i];
            bp->which.push_back(i);
        }
        if (outs) bp->outs.assign(outs, outs + count);
        bp->out_lens = out_lens;
        bp->statuses = statuses;
        bp->n = n;
        bp->o = o;
        bind_tables(c, bp.get());
        std::vector<Unit> units = split_units(c, (int)bp->jobs.size(), o.beta);
        *ticket = enqueue(c, std::move(bp), std::move(units));
        return XFG_OK;
    });
}

int xfg_batch_wait(xfg_ctx* c, uint64_t ticket) {
    if (!c) return XFG_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        std::unique_ptr<Batch> b = wait_batch(c, ticket);
        if (!b) {
            c->err = "unknown batch ticket";
            return XFG_INVALID_ARGUMENT;
        }
        if (b->err) std::rethrow_exception(b->err);
        for (size_t k = 0; k < b->jobs.size(); k++) {
            b->statuses[b->which[k]] = b->st[k];
            if (b->st[k] == XFG_BUFFER_TOO_SMALL) c->err = "output buffer too small";
            if (b->st[k] == XFG_PROVER_ERROR) c->err = prover_error_text(b->jobs[k]);
        }
        // caller-supplied traces: what the check found, decoded (the cell of a failed assertion is read
        // from the caller's buffer, which stays theirs until here)
        if (!b->keys.empty()) {
            const bool dev = b->trace.kind == TraceSrc::DEVICE;
            if (dev) HIPCHK(hipSetDevice(c->device));
            for (size_t k = 0; k < b->jobs.size(); k++) {
                const u64* tr = b->trace.p + k * 7 * b->n;
                const u64 n = b->n;
                const xfg_trace_fault f = decode_trace_key(b->keys[k], b->jobs[k].air, [&](uint32_t col, u64 step) {
                    return fetch_cell(tr, dev, (size_t)col * n + step);
                });
                if (b->faults) b->faults[b->which[k]] = f;
                if (f.kind) c->err = trace_fault_text(f);
            }
        }
        return XFG_OK;
    });
}

int xfg_prove_batch(xfg_ctx* c, uint32_t count, const xfg_burn_inputs* inputs, uint64_t trace_length,
                    const xfg_options* opts, uint8_t* const* outs, size_t* out_lens, int* statuses) {
    uint64_t t = 0;
    int r = xfg_prove_batch_submit(c, count, inputs, trace_length, opts, outs, out_lens, statuses, &t);
    if (r) return r;
    return xfg_batch_wait(c, t);
}

// XFG_TRACE_ON_DEVICE: `traces` must be device memory of the context's device that this process's HIP
// runtime allocated, and the allocation must hold all `bytes` (the lanes copy that range). Returns what
// is wrong, or null. Asks the runtime only: nothing is launched or copied
static const char* device_traces_problem(xfg_ctx* c, const void* traces, size_t bytes) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, traces) != hipSuccess) {
        (void)hipGetLastError();
        return "traces is not a device pointer known to the library's HIP runtime";
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->device) return "traces is not device memory of the context's device";
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(traces)) != hipSuccess) {
        (void)hipGetLastError();
        return "traces is not a device pointer known to the library's HIP runtime";
    }
    if ((const char*)traces + bytes > (const char*)base + size) return "the device allocation is smaller than [count][7][n] traces";
    return nullptr;
}

// the key of the first cell >= p of a host trace [7][n] in the check kernel's order (step, then
// column), TRACE_KEY_VALID when every cell is canonical
static u64 host_noncanonical_key(const u64* tr, u64 n) {
    u64 key = TRACE_KEY_VALID;
    for (unsigned col = 0; col < 7; col++)
        for (u64 s = 0; s < n; s++)
            if (tr[col * n + s] >= P) {
                key = std::min(key, trace_key(TRACE_KEY_NONCANONICAL, s, col));
                break;
            }
    return key;
}

int xfg_prove_trace_batch_submit(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                                 const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags,
                                 uint8_t* const* outs, size_t* out_lens, int* statuses, xfg_trace_fault* faults,
                                 uint64_t* ticket) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!traces || !airs || !opts || !out_lens || !statuses || !ticket || count == 0) {
        c->err = count == 0 ? "empty batch" : "null argument";
        return XFG_INVALID_ARGUMENT;
    }
    *ticket = 0;
    if (width != 7) {
        c->err = "XfgBurnMintAir traces have 7 columns";
        return XFG_INVALID_ARGUMENT;
    }
    if (flags & ~(XFG_TRACE_VALIDATE | XFG_TRACE_ON_DEVICE)) {
        c->err = "unknown trace flag";
        return XFG_INVALID_ARGUMENT;
    }
    Opts o = to_opts(opts);
    if (int st = check_request(c, n, o)) return st;
    for (uint32_t i = 0; i < count; i++)
        if (!air_canonical(&airs[i])) {  // the constraint kernel subtracts them from trace values
            c->err = "AIR constant is not a canonical field element";
            return XFG_INVALID_ARGUMENT;
        }
    const bool dev = (flags & XFG_TRACE_ON_DEVICE) != 0;
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        if (const char* m = dev ? device_traces_problem(c, traces, (size_t)count * 7 * n * 8) : nullptr) {
            c->err = m;
            return XFG_INVALID_ARGUMENT;
        }
        std::unique_ptr<Batch> bp(new Batch());
        bp->jobs.resize(count);
        bp->which.resize(count);
        bp->refused.assign(count, 0);
        bp->keys.assign(count, TRACE_KEY_VALID);
        for (uint32_t i = 0; i < count; i++) {
            bp->jobs[i].air = air_of(&airs[i]);
            bp->which[i] = i;
            statuses[i] = XFG_OK;
        }
        if (!dev) {
            // all_canonical per proof on the host pool (the submitting thread starts every batch's latency)
            u64* keys = bp->keys.data();
            host_pool().parallel_for((int)count, [&](int i) { keys[i] = host_noncanonical_key(traces + (size_t)i * 7 * n, n); });
            for (uint32_t i = 0; i < count; i++)
                if (keys[i] != TRACE_KEY_VALID) {
                    bp->refused[i] = statuses[i] = XFG_INVALID_ARGUMENT;
                    c->err = "trace element is not a canonical field element";
                }
            c->stage_traces = true;
        }
        bp->trace.kind = dev ? TraceSrc::DEVICE : TraceSrc::HOST_STAGED;
        bp->trace.p = traces;
        bp->trace.validate = (flags & XFG_TRACE_VALIDATE) != 0;
        bp->faults = faults;
        if (outs) bp->outs.assign(outs, outs + count);
        bp->out_lens = out_lens;
        bp->statuses = statuses;
        bp->n = n;
        bp->o = o;
        bind_tables(c, bp.get());
        std::vector<Unit> units = split_units(c, (int)count, o.beta);
        *ticket = enqueue(c, std::move(bp), std::move(units));
        return XFG_OK;
    });
}

int xfg_prove_trace_batch(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                          const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags, uint8_t* const* outs,
                          size_t* out_lens, int* statuses, xfg_trace_fault* faults) {
    uint64_t t = 0;
    int r = xfg_prove_trace_batch_submit(c, count, traces, width, n, airs, opts, flags, outs, out_lens, statuses,
                                         faults, &t);
    if (r) return r;
    return xfg_batch_wait(c, t);
}

int xfg_check_traces(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n, const xfg_air_consts* airs,
                     uint32_t flags, xfg_trace_fault* faults) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!traces || !airs || !faults || count == 0) {
        c->err = count == 0 ? "empty batch" : "null argument";
        return XFG_INVALID_ARGUMENT;
    }
    if (count > 65535 || !is_pow2(n) || n < 8 || n > (1ULL << 32) || (flags & ~XFG_TRACE_ON_DEVICE)) {
        c->err = "xfg_check_traces: at most 65535 traces of a power-of-two length from 8 to 2^32, flags 0 or "
                 "XFG_TRACE_ON_DEVICE";
        return XFG_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < count; i++)
        if (!air_canonical(&airs[i])) {
            c->err = "AIR constant is not a canonical field element";
            return XFG_INVALID_ARGUMENT;
        }
    const bool dev = (flags & XFG_TRACE_ON_DEVICE) != 0;
    return on_lane0(c, [&](Lane* L) -> int {
        const size_t cells = (size_t)count * 7 * n;
        if (const char* m = dev ? device_traces_problem(c, traces, cells * 8) : nullptr) {
            c->err = m;
            return XFG_INVALID_ARGUMENT;
        }
        L->trace.ensure(cells);
        L->air.ensure(count);
        L->tkeys.ensure(count);
        std::vector<AirConst> ha(count);
        for (uint32_t i = 0; i < count; i++) ha[i] = air_of(&airs[i]);
        HIPCHK(hipMemcpy(L->air.p, ha.data(), count * sizeof(AirConst), hipMemcpyHostToDevice));
        // the kernel works on the lane's copy (it canonicalises what it reports as >= p)
        HIPCHK(hipMemcpyAsync(L->trace.p, traces, cells * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                              L->stream));
        launch_trace_check(L->trace.p, L->air.p, L->tkeys.p, (int)ilog2(n), (int)count, true, L->stream);
        std::vector<u64> keys(count);
        HIPCHK(hipMemcpyAsync(keys.data(), L->tkeys.p, count * 8, hipMemcpyDeviceToHost, L->stream));
        HIPCHK(hipStreamSynchronize(L->stream));
        for (uint32_t i = 0; i < count; i++) {
            const u64* tr = traces + (size_t)i * 7 * n;
            faults[i] = decode_trace_key(keys[i], ha[i], [&](uint32_t col, u64 step) {
                return fetch_cell(tr, dev, (size_t)col * n + step);
            });
            if (faults[i].kind) c->err = trace_fault_text(faults[i]);
        }
        return XFG_OK;
    });
}

int xfg_prepare(xfg_ctx* c, uint32_t count, uint64_t trace_length, const xfg_options* opts) {
    if (!c || !opts || count == 0) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    u64 n = trace_length ? trace_length : 64;
    Opts o = to_opts(opts);
    if (int st = check_request(c, n, o)) return st;
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        // two throw-away proving passes over a fixed valid statement size every lane workspace
        // (device + pinned host) and load every code object; nothing is cached between proofs
        xfg_burn_inputs in{};
        in.burn_amount = in.mint_amount = STANDARD_BURN;
        for (int i = 0; i < 32; i++) in.tx_prefix_hash[i] = (uint8_t)(i + 1);
        static const uint8_t rcpt[20] = {1}, sec[32] = {2};
        in.recipient_address = rcpt;
        in.recipient_len = 20;
        in.secret = sec;
        in.secret_len = 32;
        in.network_id = 1;
        in.target_chain_id = 42161;
        in.commitment_version = 1;
        AirConst a;
        std::string err;
        if (marshal(&in, a, err)) return XFG_PROVER_ERROR;
        // every lane proves one full unit, twice (lane-pinned units)
        ensure_workers(c);
        const int nl = (int)c->workers.size(), U = std::min<int>((int)count, unit_size(o.beta));
        for (int pass = 0; pass < 2; pass++) {
            std::unique_ptr<Batch> bp(new Batch());
            bp->jobs.resize((size_t)nl * U);
            for (auto& j : bp->jobs) j.air = a;
            bp->trace.size_staging = c->stage_traces;
            bp->n = n;
            bp->o = o;
            bind_tables(c, bp.get());
            std::vector<Unit> units;
            for (int l = 0; l < nl; l++) units.push_back(Unit{nullptr, l * U, (l + 1) * U, l});
            std::unique_ptr<Batch> b = wait_batch(c, enqueue(c, std::move(bp), std::move(units)));
            if (b->err) std::rethrow_exception(b->err);
        }
        HIPCHK(hipDeviceSynchronize());
        return XFG_OK;
    });
}

int xfg_prove_burn_mint(xfg_ctx* c, const xfg_burn_inputs* in, uint64_t trace_length, const xfg_options* opts,
                        uint8_t* out, size_t* out_len) {
    if (!c) return XFG_INVALID_ARGUMENT;
    if (!out_len) return XFG_INVALID_ARGUMENT;
    int st = 0;
    uint8_t* outs[1] = {out};
    size_t lens[1] = {*out_len};
    int r = xfg_prove_batch(c, 1, in, trace_length, opts, outs, lens, &st);
    if (r) return r;
    *out_len = lens[0];
    return st;
}

int xfg_selftest_field(uint64_t a, uint64_t b, uint64_t* out3) {
    if (!out3 || a >= P || b >= P) return XFG_INVALID_ARGUMENT;
    out3[0] = gl_mul(a, b);
    out3[1] = gl_add(a, b);
    out3[2] = gl_sub(a, b);
    return XFG_OK;
}

int xfg_set_timing(xfg_ctx* c, int enabled) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->timing = enabled != 0;
    for (auto& L : c->lanes) L->timing = c->timing;
    return XFG_OK;
}

int xfg_stage_times(const xfg_ctx* c, double* ms, const char** names, int max) {
    if (!c) return 0;
    int k = std::min<int>(max, ST_COUNT);
    for (int i = 0; i < k; i++) {
        if (ms) ms[i] = c->lanes.empty() ? 0.0 : c->lanes[c->last_lane]->stage_ms[i];
        if (names) names[i] = STAGE_NAMES[i];
    }
    return k;
}

}  // extern "C"
