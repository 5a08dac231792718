// One work unit on a lane: the lanes and their streams, buffer sizing, and prove_lane (the device
// chain from the trace to the FRI remainder, then the host steps of proof_assembly.hpp and the
// openings' gathers). The lane workers (prover.hip) and the debug entry points (debug_abi.hip) call in.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "host_pool.hpp"
#include "prover_internal.hpp"

namespace xfg {

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
    c->const_col.ensure(const_flag_bytes(B * 7));
    c->const_val.ensure(B * 7);
}
void size_constraint_eval(Lane* c, size_t B, const ProofShape& sh) {
    c->air.ensure(B);
    c->coeffs.ensure(B * 15 * sh.DE);
    c->ce.ensure(B * sh.DE * 2 * sh.n);
    c->ce_uni.ensure(B);
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

// every device buffer of a unit of B proofs, and the pinned opening buffers
static void size_lane_buffers(Lane* c, size_t B, const ProofShape& sh, const Opts& o, const TraceSrc& ts,
                              const RecordSrc& rs) {
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
    c->rstatus.ensure(B);  // a few bytes, sized for every unit so that xfg_prepare covers units of records too
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

// the job's host coin at the start of its transcript: Context::to_elements || public inputs (ProverChannel::new)
static void seed_coin(ProofJob& j, const ProofShape& sh, const Opts& o) {
    u64 e[20];
    context_elements(sh.n, o, e);
    memcpy(e + 8, j.air.pub, 12 * 8);
    j.coin.init(e, 20);
    j.commitments.clear();
}

// AIR constants and transcript seeds of the unit's proofs, on the host and on the device.
// The Fiat-Shamir steps between the commitments (coefficient, OOD point, DEEP and FRI alpha
// draws) run on the device from a copy of each proof's coin, so the whole chain from the trace
// to the FRI remainder is enqueued without a host round trip; the host replays the same
// transcript from the roots and OOD values once the chain has finished (replay_transcript).
// Records in device memory: the record kernel puts both on the device from the unit's records, with no host work
// per proof before the launch; the host takes the constants from the replay block afterwards (adopt_record_inputs)
static void upload_unit_inputs(Lane* c, ProofJob* jobs, int B, const ProofShape& sh, const Opts& o, const RecordSrc& rs) {
    hipStream_t s = c->stream;
    if (rs.p) {
        launch_burn_marshal(rs.p, B, coin_context(sh.n, o), c->air.p, c->dcoin.p, c->rstatus.p, s);
        HIPCHK(hipMemsetAsync(c->dfail.p, 0, B * sizeof(int), s));
        return;
    }
    AirConst* airs = c->h_air.ensure(B);
    for (int b = 0; b < B; b++) airs[b] = jobs[b].air;
    upload(c->air.p, airs, B * sizeof(AirConst), s);
    DevCoin* hc = c->h_coin.ensure(B);
    for (int b = 0; b < B; b++) {
        ProofJob& j = jobs[b];
        seed_coin(j, sh, o);
        hc[b].seed = j.coin.seed;
        hc[b].counter = j.coin.counter;
        hc[b].pad = 0;
    }
    upload(c->dcoin.p, hc, B * sizeof(DevCoin), s);
    HIPCHK(hipMemsetAsync(c->dfail.p, 0, B * sizeof(int), s));
}
// a unit of device records, its stream synchronised: the jobs' AIR constants from the replay block and their coins
// seeded from them on the host, as upload_unit_inputs does for marshalled jobs. The replay then checks the
// device's draws, and with them the seed the record kernel computed, against this coin
static void adopt_record_inputs(const Lane* c, ProofJob* jobs, int B, const ProofShape& sh, const Opts& o) {
    host_pool().parallel_for(B, [c, jobs, &sh, &o](int b) {
        jobs[b].air = c->h_rair[b];
        seed_coin(jobs[b], sh, o);
    });
}

ColConst trace_const(const Lane* c, const ProofShape& sh) {
    ColConst cc;
    cc.flags = c->const_col.p;
    cc.vals = c->const_val.p;  // [B][7], element 0 of every column (launch_const_detect)
    cc.val_stride = 1;
    return cc;
}

void launch_trace_front(Lane* c, int B, int logn, const TraceFront& f) {
    hipStream_t s = c->stream;
    // xfg_debug_poison_lde: the planes of constant and shared columns are never written where the live ones
    // alone are: nothing an earlier unit left there can pass for a plane of this one
    if (c->poison_lde && f.kind != TraceFront::IN_LANE)
        HIPCHK(hipMemsetAsync(c->trace.p, 0xFF, ((size_t)B * 7 * 8) << logn, s));
    // constant columns, and the columns of proofs 1 .. B - 1 that equal proof 0's
    switch (f.kind) {
        case TraceFront::GENERATED:  // found in the rows as they are generated
            launch_trace_probe(c->air.p, B, logn, c->const_col.p, c->const_val.p, s, f.synth);
            launch_trace_gen(c->air.p, B, logn, c->const_col.p, c->trace.p, s, f.synth);
            break;
        case TraceFront::IN_LANE:  // one pass over the trace, behind its check
            if (f.check != TraceFront::NONE)
                launch_trace_check(c->trace.p, c->air.p, c->tkeys.p, logn, B, f.check == TraceFront::AIR, s);
            launch_const_detect(c->trace.p, B * 7, logn, c->const_col.p, s, 7, c->const_val.p);
            break;
        case TraceFront::IN_PLACE:  // found, with the check's words, in the caller's buffer where it lies
            launch_trace_ingest_probe(f.rows, c->air.p, B, logn, f.check == TraceFront::AIR, c->tkeys.p, c->const_col.p,
                                      c->const_val.p, s);
            launch_trace_ingest_write(f.rows, B, logn, c->const_col.p, c->trace.p, s);
            break;
    }
}

void launch_trace_lde(Lane* c, const Tables& T, int B, const ProofShape& sh, bool probe) {
    hipStream_t s = c->stream;
    const unsigned char* skip = c->const_col.p;
    // xfg_debug_poison_lde: the LDE planes and the coefficients of constant and shared columns are never written
    if (c->poison_lde) {
        HIPCHK(hipMemsetAsync(c->lde.p, 0xFF, (size_t)B * 7 * sh.N * 8, s));
        HIPCHK(hipMemsetAsync(c->coef.p, 0xFF, (size_t)B * 7 * sh.n * 8, s));
    }
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
    // the planes of the flagged columns, in c->coef and in c->lde, are never written: every reader of
    // either takes trace_const along
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
// with_records: the AIR constants and the statuses the record kernel wrote ride along (units of device records)
static ReplayView pack_replay_block(Lane* c, size_t B, const ProofShape& sh, bool with_keys, bool with_records) {
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
    const u64 o_rair = with_records ? seg(c->air.p, B * sizeof(AirConst)) : 0;
    const u64 o_rstatus = with_records ? seg(c->rstatus.p, B * sizeof(int)) : 0;
    static_assert(PackSet::MAX >= 12, "nine segments, the keys and the two of a unit of records");
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
    c->h_rair = with_records ? (const AirConst*)(hx + o_rair) : nullptr;
    c->h_rstatus = with_records ? (const int*)(hx + o_rstatus) : nullptr;
    return rv;
}

// the whole device chain of a unit, trace to FRI remainder and the replay block, enqueued on the
// lane stream without a host round trip. g: the trace domain generator
static ReplayView enqueue_commit_chain(Lane* c, const Tables& T, const u64* ce_div, ProofJob* jobs, int B,
                                       const TraceSrc& ts, const RecordSrc& rs, const ProofShape& sh, const Opts& o,
                                       u64 g, HostTrace& ht) {
    const u64 n = sh.n;
    const int logn = sh.logn, logbeta = sh.logbeta, DE = sh.DE;
    hipStream_t s = c->stream;
    upload_unit_inputs(c, jobs, B, sh, o, rs);
    // ---- 1. trace LDE + commitment (DefaultTraceLde::new)
    ht.mark("setup");
    stage_mark(c, 0);
    const size_t tbytes = (size_t)7 * n * 8;  // one proof's trace
    switch (ts.kind) {
        case TraceSrc::GENERATED: break;
        case TraceSrc::HOST_DIRECT:  // xfg_prove_trace: one trace, straight from the caller's memory
            HIPCHK(hipMemcpyAsync(c->trace.p, ts.p, B * tbytes, hipMemcpyHostToDevice, s));
            break;
        case TraceSrc::HOST_STAGED: {
            // gathered into the lane's pinned dense staging (the stream has drained: the last unit's upload is
            // over), then one asynchronous DMA; a proof refused at submission (cell >= p) is staged as zeros
            u64* st = c->h_trace.p;
            const u64* src = ts.p;
            const int* refused = ts.refused;
            const TraceLayout L = ts.layout;
            host_pool().parallel_for(B, [st, src, refused, n, tbytes, L](int b) {
                if (refused[b]) memset(st + (size_t)b * 7 * n, 0, tbytes);
                else gather_trace(src + (size_t)b * L.trace_stride, L, n, st + (size_t)b * 7 * n);
            });
            HIPCHK(hipMemcpyAsync(c->trace.p, st, B * tbytes, hipMemcpyHostToDevice, s));
            break;
        }
        case TraceSrc::DEVICE: break;  // read where they lie
    }
    TraceFront front{TraceFront::GENERATED, TraceFront::NONE, nullptr, {}};
    if (ts.kind != TraceSrc::GENERATED) {
        front.kind = ts.on_device() ? TraceFront::IN_PLACE : TraceFront::IN_LANE;
        front.check = ts.validate ? TraceFront::AIR : ts.checks() ? TraceFront::CANONICAL : TraceFront::NONE;
        if (ts.on_device()) front.rows = StridedRows{ts.p, ts.layout};
    }
    launch_trace_front(c, B, logn, front);
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
    const ColConst cc = trace_const(c, sh);
    launch_merkle_lde(c->lde.p, 7, c->tnodes.p, B, logn, logbeta, s, cs, cc);
    stage_mark(c, 2);
    // ---- 3. constraint evaluation + composition polynomial + commitment
    launch_constraint_eval(c->lde.p, c->air.p, c->coeffs.p, ce_div, c->ce.p, logn, logbeta, B, DE, s, cc,
                           c->ce_uni.p);
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
    launch_ood(c->coef.p, c->hcoef.p, c->zpts.p, c->partial.p, c->ood.p, logn, B, DE, s, dc, cc);
    stage_mark(c, 6);
    // ---- 5. DEEP composition polynomial (coefficient form) + its LDE
    launch_deep(c->coef.p, c->hcoef.p, c->dp.p, c->partial.p, c->carry.p, c->deep.p, logn, B, DE, s, cc);
    launch_lde(c->deep.p, n, c->f0.p, c->scratch.p, B * DE, logn, logbeta, T, s);
    // degree check: deg(DEEP) == n - 2  <=>  coefficient n-2 != 0 (coefficient n-1 is 0 by construction)
    HIPCHK(hipMemcpy2DAsync(c->dn2.p, 8, c->deep.p + (n - 2), n * 8, 8, (size_t)B * DE, hipMemcpyDeviceToDevice, s));
    stage_mark(c, 7);
    // ---- 6. FRI layers and remainder, then the replay's inputs
    enqueue_fri_layers(c, T, B, sh, (int)o.fold, cs, ht);
    const ReplayView rv = pack_replay_block(c, B, sh, ts.checks(), rs.p != nullptr);
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
    // segment 0, the opened trace values: an index into c->lde, whose constant columns' planes are not written
    const ColConst cc = trace_const(c, sh);
    gs.cc_seg = 0;
    gs.cc_shift = sh.logn + sh.logbeta;
    gs.cc = cc;
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
    launch_open_rows(c->lde.p, 7, ent, nent, gdig + ndig, sh.logn, sh.logbeta, sq, cc);
    launch_open_rows(c->hlde.p, sh.DE, ent, nent, gdig + ndig + nopen, sh.logn, sh.logbeta, sq);
    ht.mark("q_launch");
    stage_mark(c, 9, sq);
    return Gathered{gv, gd};
}

// the batched prover: jobs[i].air filled; trace_host optional ([B][7][n], else generated on device).
// Device chain -> host transcript replay -> opening plans -> gathers -> serialisation; the per-proof
// host steps (proof_assembly.hpp) are independent and spread over the host pool
void prove_lane(Lane* c, const Tables& T, const u64* ce_div, ProofJob* jobs, int B, const TraceSrc& ts,
                       u64 n, const Opts& o, const RecordSrc& rs) {
    using clk = std::chrono::steady_clock;
    const auto t_host0 = clk::now();
    HostTrace ht;
    ht.mark("start");
    const ProofShape sh(n, o);
    const u64 g = gl_root(sh.logn);
    HostPool& pool = host_pool();

    size_lane_buffers(c, B, sh, o, ts, rs);
    const ReplayView rv = enqueue_commit_chain(c, T, ce_div, jobs, B, ts, rs, sh, o, g, ht);
    HIPCHK(hipStreamSynchronize(c->stream));
    ht.mark("sync_rem");
    if (rs.p) adopt_record_inputs(c, jobs, B, sh, o);
    // trace columns that went through the NTTs; the rest were found constant, or the same as proof 0's
    u64 live_cols = 0, shared_cols = 0;
    for (int k = 0; k < B * 7; k++) {
        const int cls = col_class(c->h_const_col[k]);
        live_cols += cls == 0 ? 1 : 0;
        shared_cols += cls == 2 ? 1 : 0;
    }
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
    // device records: the record kernel's status is the proof's, whatever prover error the discarded slot earned
    for (int b = 0; b < B && rs.p; b++)
        if (c->h_rstatus[b]) jobs[b].status = c->h_rstatus[b];
    ht.dump(B, (long)((u64)B * 7 - live_cols - shared_cols), (long)shared_cols);
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
    L->poison_lde = c->poison_lde;
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
void ensure_lanes(xfg_ctx* c, size_t k) {
    lane0(c);
    while (c->lanes.size() < k) {
        c->lanes.emplace_back(new Lane());
        create_lane_stream(c, c->lanes.back().get());
    }
    for (auto& L : c->lanes) gather_stream(L.get());
}

}  // namespace xfg
