// The prover context as its translation units share it: the table registry (tables.hip), the lanes
// and one work unit on a lane (lane_unit.hip), the batches and their queue (prover.hip,
// unit_queue.hpp), the debug / bench entry points (debug_abi.hip) and the GPU batch verifier's
// host side (verify_batch_gpu.hip).
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xfg_stark.h"
#include "grind_plan.hpp"
#include "hip_util.hpp"
#include "host_common.hpp"
#include "kernels.hpp"
#include "proof_assembly.hpp"
#include "unit_queue.hpp"
#include "verifier.hpp"

namespace xfg {

struct TablesHost {
    int LM = -1;
    DBuf<u64> tw, pow7, ipow7;
    std::map<int, DBuf<u64>> ce_div;  // constraint divisor tables per log2(trace length)
    FourStep fs;                      // four-step twiddle tables (pointers into four_buf)
    std::map<int, DBuf<u64>> four_buf;
    std::map<int, DBuf<u64>> pass_buf;  // standalone forward pass tables (fs.pass_fwd)
};

enum {
    ST_LDE, ST_TCOMMIT, ST_CE, ST_COMP, ST_CCOMMIT, ST_OOD, ST_DEEP, ST_FRI, ST_GATHER, ST_HOST, ST_HQUERY, ST_HSER,
    ST_COUNT
};

// one lane = one HIP stream + its pooled device buffers + one host thread; a batch is split
// across lanes so one lane's host-side Fiat-Shamir / serialisation overlaps another's kernels.
// Destroyed with no work in flight: the destructor synchronises both streams, then the buffers go.
struct Lane {
    hipStream_t stream = nullptr;
    hipStream_t gstream = nullptr;  // the openings' gathers (gather_stream)
    bool timing = false;
    double stage_ms[ST_COUNT] = {0};
    hipEvent_t ev[ST_COUNT + 1] = {};
    // xfg_lde_probe: events around the trace LDE launch set, totals of the units so far
    bool lde_probe = false;
    hipEvent_t lde_ev[2] = {};
    double lde_ms = 0;
    u64 lde_sets = 0, lde_polys = 0;
    // xfg_debug_poison_lde: launch_trace_lde sets c->lde and c->coef to 0xFF bytes first, launch_trace_front the
    // c->trace of a unit whose live planes alone it writes
    bool poison_lde = false;
    DBuf<AirConst> air;
    DBuf<CeUniform> ce_uni;  // [B] launch_constraint_eval's per-proof uniform part (constant trace columns)
    DBuf<u64> coeffs, trace, coef, scratch, lde, ce, hcoef, hlde, zpts, partial, ood, carry, deep, f0, alpha7,
        rem, dn2, falpha;
    DBuf<Digest> tnodes, hnodes, droots;
    DBuf<DeepParams> dp;
    DBuf<DevCoin> dcoin;  // device-side transcript
    DBuf<int> dfail;
    // [B][7] (padded to whole 32-bit words): COL_CONST where a trace column holds one value in every row,
    // COL_SHARED where it equals the same column of the unit's proof 0 (launch_const_detect); such columns
    // skip the interpolation and the LDE. const_val [B][7]: element 0 of every column, the value of a
    // constant one. h_const_col: the unit's flags in the replay block, for the counters
    DBuf<unsigned char> const_col;
    DBuf<u64> const_val;
    const unsigned char* h_const_col = nullptr;
    // caller-supplied traces (xfg_prove_trace_batch): tkeys [B] the check kernel's word per proof
    // (launch_trace_check), h_tkeys the unit's words in the replay block; h_trace the pinned staging host
    // traces are uploaded from (sized with the lane's buffers, so the upload is a true asynchronous DMA
    // that never waits on the caller's pageable memory)
    DBuf<u64> tkeys;
    const u64* h_tkeys = nullptr;
    // statements as packed records in device memory (xfg_prove_records): rstatus [B] the record kernel's status
    // per record (launch_burn_marshal); h_rair, h_rstatus the unit's AIR constants and statuses in the replay block
    DBuf<int> rstatus;
    const AirConst* h_rair = nullptr;
    const int* h_rstatus = nullptr;
    HBuf<u64> h_trace;
    std::vector<DBuf<u64>> flayer;
    std::vector<DBuf<Digest>> fnodes;
    // pinned host staging
    MappedHBuf<Digest> h_gd;
    MappedHBuf<u64> h_idx, h_gv;
    MappedHBuf<unsigned char> h_xfer;  // the replay's inputs, written by launch_pack
    MappedHBuf<AirConst> h_air;
    MappedHBuf<DevCoin> h_coin;
    // the device's proof-of-work search (grind_search): seeds in, nonces out, the kernel's per-proof words
    MappedHBuf<Digest> h_gseed;
    MappedHBuf<u64> h_gnonce;
    DBuf<Digest> gseed;
    DBuf<u64> gstate;
    int cus = 0;  // compute units of the device (grind_plan)
    std::atomic<uint64_t> grind_dev{0}, grind_host{0};  // proofs whose nonce was searched there (xfg_grind_probe)
    // host scratch of the opening plans and the serialiser, kept across units so steady-state
    // units neither allocate nor page-fault (their cost grew with the shared hosts' load)
    struct {
        OpeningIndex ix;
        std::vector<LaneLayout> lay;
    } hs;
    Lane() = default;
    Lane(const Lane&) = delete;
    Lane& operator=(const Lane&) = delete;
    ~Lane() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (gstream) (void)hipStreamSynchronize(gstream);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : lde_ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (gstream) (void)hipStreamDestroy(gstream);
    }
};

// where a unit's traces come from, and what is checked on the way. p: cell (0, 0, 0) of the unit's own slice
// (null: generated on the device from the AIR constants)
struct TraceSrc {
    enum Kind { GENERATED, HOST_DIRECT, HOST_STAGED, DEVICE };
    Kind kind = GENERATED;
    const u64* p = nullptr;
    // where the cells lie from p on: dense_layout(n) unless the caller gave another. A unit's slice starts
    // trace_stride words per proof further on
    TraceLayout layout{0, 0, 0};
    // read where they lie, or copied into the lane's dense [B][7][n] first: device traces, in whatever layout, are
    // never copied (the IN_PLACE front end, launch_trace_front; check_traces); host traces are gathered into the
    // lane's staging
    bool on_device() const { return kind == DEVICE; }
    bool validate = false;        // XFG_TRACE_VALIDATE: the AIR check behind the upload
    bool size_staging = false;    // grow the lane's pinned trace staging with its other buffers
    const int* refused = nullptr;  // [B] non-zero: refused at submission, the slot is proven over zeros
    u64* keys = nullptr;          // [B] out: the check kernel's words (when checks())
    // device traces are always tested for canonical cells; host traces were on the host
    bool checks() const { return validate || on_device(); }
};

// a unit's statements as packed records in device memory: p the unit's own slice (null: the jobs carry AIR
// constants marshalled on the host). The record kernel marshals them at the head of the chain; a record the
// kernel finds invalid keeps its slot, gets its status after the unit's host steps and no proof
struct RecordSrc {
    const xfg_burn_record* p = nullptr;
};

// a submitted batch: jobs [0, B) proven in units of XFG_UNIT proofs by the lane workers; proof
// bytes are copied into the caller's buffers on the worker thread as each unit finishes
struct Batch {
    std::vector<ProofJob> jobs;
    std::vector<uint32_t> which;   // jobs[k] -> caller index
    std::vector<uint8_t*> outs;    // caller buffers (null entry or empty: size query)
    size_t* out_lens = nullptr;    // caller capacities in, proof lengths out
    int* statuses = nullptr;       // caller statuses, written by wait
    std::vector<int> st;           // per-job copy-out status
    // caller-supplied traces, trace.p the batch's base (job k <-> caller index k: such a batch keeps refused
    // proofs as jobs so that every unit's slice stays at b0 * trace.layout.trace_stride)
    TraceSrc trace;
    std::vector<int> refused;          // per job: status set at submission (cell >= p), else 0
    std::vector<u64> keys;             // per job: the trace check's word
    xfg_trace_fault* faults = nullptr;  // caller's, filled by wait (may be null)
    // statements as device records, records.p the batch's base (job k <-> caller index k, as for traces: every
    // unit's records are the contiguous slice at b0)
    RecordSrc records;
    u64 n = 0;
    Opts o{};
    Tables T{};
    const u64* ce_div = nullptr;
    int units_left = 0;
    std::exception_ptr err;
};

struct HostTrace {
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> m;
    std::map<std::string, double> acc;  // accumulated sub-phase ms
    using clk = std::chrono::steady_clock;
    clk::time_point t_ = {};
    void tic() {
        if (trace_on()) t_ = clk::now();
    }
    void toc(const char* what) {
        if (!trace_on()) return;
        auto t = clk::now();
        acc[what] += std::chrono::duration<double, std::milli>(t - t_).count();
        t_ = t;
    }
    void mark(const char* what) {
        if (trace_on()) m.push_back({what, std::chrono::steady_clock::now()});
    }
    // const_cols, shared_cols: trace columns found constant, or equal to the unit's first proof's, and
    // not transformed (-1: not a proving batch)
    void dump(int B, long const_cols = -1, long shared_cols = -1) {
        if (!trace_on() || m.size() < 2) return;
        std::string line = "[xfg] B=" + std::to_string(B);
        if (const_cols >= 0) line += " const_cols=" + std::to_string(const_cols);
        if (shared_cols >= 0) line += " shared_cols=" + std::to_string(shared_cols);
        for (size_t i = 1; i < m.size(); i++) {
            char buf[96];
            snprintf(buf, sizeof buf, " %s=%.2f", m[i].first,
                     std::chrono::duration<double, std::milli>(m[i].second - m[i - 1].second).count());
            line += buf;
        }
        for (auto& kv : acc) {
            char buf[96];
            snprintf(buf, sizeof buf, " [%s=%.3f]", kv.first.c_str(), kv.second);
            line += buf;
        }
        fprintf(stderr, "%s\n", line.c_str());
    }
};

}  // namespace xfg

struct xfg_ctx {
    int device = 0;
    std::string err;
    bool lde_probe = false;  // xfg_lde_probe state, inherited by lanes created later
    bool poison_lde = false;  // xfg_debug_poison_lde state, inherited likewise
    // set by the first batch of host traces (xfg_prove_trace_batch): from then on xfg_prepare sizes
    // every lane's pinned trace staging too
    bool stage_traces = false;
    xfg::TablesHost tables;
    std::vector<std::unique_ptr<xfg::Lane>> lanes;
    // persistent lane workers: one host thread per lane pulls proof units from a FIFO shared by
    // every submitted batch, so the host tail of one batch overlaps the kernels of the next.
    // Timing mode (xfg_set_timing) is the queue's whole-units switch
    xfg::UnitQueue<xfg::Batch> queue;
    std::vector<std::thread> workers;
    // batched GPU verification workspace (xfg_verify_batch_gpu)
    struct {
        xfg::HBuf<uint8_t> stage;  // pinned: proof blob + task lists, one DMA
        xfg::DBuf<uint8_t> dstage;
        xfg::DBuf<xfg::u64> flags;  // one 64-bit word per proof (verifier.hpp VF_*)
        std::vector<xfg::VState> st;        // per-proof transcript states, reused between calls
        std::vector<xfg::VerifyPlan> frag;  // per-proof plan fragments, reused between calls
    } vb;
};

namespace xfg {

// ---- defined in tables.hip
void ensure_tables(xfg_ctx* c, int LM);
const u64* ensure_ce_table(xfg_ctx* c, int logn);
// false when a four-step (or pass) table of the NTT sizes one (n, beta) proof uses is missing
bool fourstep_ready(xfg_ctx* c, int logn, int logbeta);
// caller guarantees no kernel in flight reads the registry (fresh context or drained)
void ensure_fourstep(xfg_ctx* c, int logn, int logbeta);
Tables tables_of(xfg_ctx* c);
// ---- defined in lane_unit.hip
Lane* lane0(xfg_ctx* c);
void ensure_lanes(xfg_ctx* c, size_t k);
// one work unit: jobs[0, B) with .air filled (or rs.p: the unit's records, from which the record kernel fills the
// lane's constants and the host then the jobs'), proven on the lane's streams and serialised into .bytes
void prove_lane(Lane* c, const Tables& T, const u64* ce_div, ProofJob* jobs, int B, const TraceSrc& ts, u64 n,
                const Opts& o, const RecordSrc& rs = RecordSrc{});
// Context::to_elements of a proof of this shape as the record kernel takes them
static inline CoinContext coin_context(u64 n, const Opts& o) {
    CoinContext cx;
    context_elements(n, o, cx.e);
    return cx;
}
// buffer sizing and launch sets of the proving chain that the debug entry points run too; of the
// shape they read n, beta and DE only
void size_trace_lde(Lane* c, size_t B, const ProofShape& sh);        // trace, coef, scratch, lde
void size_constraint_eval(Lane* c, size_t B, const ProofShape& sh);  // air, coeffs, ce, ce_uni
void size_ood_deep(Lane* c, size_t B, const ProofShape& sh);  // hcoef, zpts, partial, ood, dp, carry, deep
// The front end of a unit's trace: whatever the source, it leaves the live columns in c->trace [B][7][n], the
// classes of the columns (constant, equal to proof 0's, live) in c->const_col, element 0 of every column in
// c->const_val and, where the source is checked, the check's word per proof in c->tkeys; c->air holds the
// unit's AIR constants.
// GENERATED: the rows of the burn row generator on c->air (synth: the synthetic generator, debug) are
//   classified as they are produced (launch_trace_probe), then launch_trace_gen writes the live columns alone.
// IN_LANE: the traces lie in c->trace (whatever put them there): launch_trace_check unless check is NONE (it
//   canonicalises the cells it reports as >= p), then one pass for the classes (launch_const_detect).
// IN_PLACE: the traces lie in device memory behind `rows` and are not copied: one pass finds the words
//   (canonicity, and the AIR's constraints when check is AIR), the classes and the values
//   (launch_trace_ingest_probe), a second writes the canonical live columns (launch_trace_ingest_write).
// GENERATED and IN_PLACE leave the planes of constant and shared columns of c->trace unwritten
struct TraceFront {
    enum Kind { GENERATED, IN_LANE, IN_PLACE } kind;
    enum Check { NONE, CANONICAL, AIR } check;
    const SynthRowGen* synth;
    StridedRows rows;
};
void launch_trace_front(Lane* c, int B, int logn, const TraceFront& f);
// trace -> coefficients -> LDE (DefaultTraceLde::new) behind launch_trace_front; probe: the xfg_lde_probe
// events around the LDE. The columns flagged in c->const_col are not transformed: their planes of c->coef and
// c->lde are left unwritten, and whatever reads either afterwards takes trace_const along
void launch_trace_lde(Lane* c, const Tables& T, int B, const ProofShape& sh, bool probe);
ColConst trace_const(const Lane* c, const ProofShape& sh);
// the proof-of-work search on the device for the B seeds the caller wrote to grind_seeds(c, B): launched on
// the lane's gather stream (idle between a unit's chain and its gathers) and waited for. Returns the B
// nonces (pinned host memory, valid until the lane's next search), 0 where [first, max_nonce] held none
void size_grind(Lane* c, size_t B);
Digest* grind_seeds(Lane* c, size_t B);
const u64* grind_search(Lane* c, int B, unsigned grind, u64 first, u64 max_nonce, unsigned chunk_log, unsigned blocks);

// the kernels' subtractions (gl_sub) are exact for canonical operands only: host inputs are checked
static inline bool all_canonical(const uint64_t* v, size_t k) {
    for (size_t i = 0; i < k; i++)
        if (v[i] >= P) return false;
    return true;
}
static inline bool air_canonical(const xfg_air_consts* a) {
    return all_canonical(a->pub_inputs, 12) && a->nullifier < P && a->commitment < P;
}

// air_of (verifier.hpp) the other way round: the kernels' constants as a caller reads them
static inline void air_out(const AirConst& a, xfg_air_consts* out) {
    memcpy(out->pub_inputs, a.pub, sizeof a.pub);
    out->nullifier = a.nullifier;
    out->commitment = a.commitment;
}

// `count` AIR constants of a caller as the kernels take them, into out; false, with the text in c->err, when
// one is not canonical (the constraint kernel subtracts them from trace values). up: copied to that lane's
// c->air as well, before the call returns
static bool airs_of(xfg_ctx* c, const xfg_air_consts* airs, size_t count, std::vector<AirConst>& out, Lane* up = nullptr) {
    out.resize(count);
    for (size_t i = 0; i < count; i++) {
        if (!air_canonical(&airs[i])) {
            c->err = "AIR constant is not a canonical field element";
            return false;
        }
        out[i] = air_of(&airs[i]);
    }
    if (up) {
        up->air.ensure(count);
        HIPCHK(hipMemcpy(up->air.p, out.data(), count * sizeof(AirConst), hipMemcpyHostToDevice));
    }
    return true;
}

// the layout an entry was given: NULL is the dense one
static inline TraceLayout layout_of(const xfg_trace_layout* layout, u64 n) {
    return layout ? TraceLayout{layout->trace_stride, layout->col_stride, layout->row_stride} : dense_layout(n);
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

// the trace check's word (trace_key, trace_layout.hpp) for trace i of src as the C ABI reports it: the cell of
// a failed assertion or of a value >= p is read from the caller's buffer through the layout (host memory, or
// device memory of the current device: one 8-byte copy); the text of a fault goes to *err (null: nowhere)
static xfg_trace_fault trace_fault_of(u64 key, const AirConst& A, const TraceSrc& src, size_t i, std::string* err) {
    xfg_trace_fault f{};
    if (key == TRACE_KEY_VALID) return f;
    const unsigned kind = (unsigned)(key >> 62), idx = (unsigned)(key & 7);
    f.step = (key << 2) >> 5;
    if (kind == TRACE_KEY_TRANSITION) {
        f.kind = 2;
        f.index = idx;
    } else {
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
        const u64* cell = src.p + src.layout.at(i, f.column, f.step);
        if (src.on_device()) HIPCHK(hipMemcpy(&f.found, cell, 8, hipMemcpyDeviceToHost));
        else f.found = *cell;
    }
    if (err) *err = trace_fault_text(f);
    return f;
}

template <class F>
static int guarded(xfg_ctx* c, F f) {
    try {
        return f();
    } catch (const HipError& e) {
        c->err = e.what();
        return XFG_DEVICE_ERROR;
    } catch (const std::exception& e) {
        c->err = std::string("Prover error: ") + e.what();
        return XFG_PROVER_ERROR;
    }
}

// an entry point that uses lane 0 directly: refused while batches are pending (lane 0's stream,
// buffers and counters belong to the workers then), else f(lane 0) with the context's device current.
// The lane's timing flag follows timing mode here; the workers set it for the units they pick
template <class F>
static int on_lane0(xfg_ctx* c, F f) {
    if (c->queue.busy()) {
        c->err = "batches pending: call xfg_batch_wait first";
        return XFG_INVALID_ARGUMENT;
    }
    return guarded(c, [&]() -> int {
        Lane* L = lane0(c);
        L->timing = c->queue.whole_units();
        HIPCHK(hipSetDevice(c->device));
        return f(L);
    });
}

// lane / work-unit tuning knobs (XFG_LANES, XFG_UNIT)
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
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

}  // namespace xfg
