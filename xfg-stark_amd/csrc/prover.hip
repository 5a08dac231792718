// Host orchestration of the MI355X burn-proof STARK prover + the C ABI (include/xfg_stark.h).
//
// Pipeline = Winterfell 0.8.3 `Prover::prove` as bound by the reference
// (src/burn_mint_air.rs:479-531, src/burn_mint_prover.rs:62-129), batched over independent
// proofs: every kernel launch covers all proofs of the batch, and the host only touches the
// serial Fiat-Shamir steps (a few BLAKE3 calls per proof per round) between launch sets.
//
// This file: the production ABI and its glue to the lane scheduler (unit_queue.hpp): batches, their
// units and tables, the copy-out. The table registry is in tables.hip, the lanes and prove_lane (one
// work unit: the device chain, then the host steps of proof_assembly.hpp) in lane_unit.hip, the debug /
// bench entry points in debug_abi.hip, the GPU batch verifier's host side in verify_batch_gpu.hip.
#include <algorithm>
#include <cstring>

#include "host_pool.hpp"
#include "marshal.hpp"
#include "prover_internal.hpp"

namespace xfg {

static const char* STAGE_NAMES[] = {"trace_lde",     "trace_commit", "constraint_eval", "composition",
                                    "comp_commit",   "ood",          "deep",            "fri",
                                    "queries_gather", "host_total",  "host_queries",    "host_serialize"};

// the statuses record_status gives an invalid record
static bool record_refusal(int st) {
    return st == XFG_INVALID_BURN_AMOUNT || st == XFG_MINT_MISMATCH || st == XFG_ZERO_TX_HASH || st == XFG_INVALID_ARGUMENT;
}

static void copy_unit(Batch* b, int b0, int b1) {
    host_pool().parallel_for(b1 - b0, [&](int i0) {
        const int k = b0 + i0;
        ProofJob& j = b->jobs[k];
        if (j.status) {
            b->st[k] = j.status;
            // no proof: whatever the slot's chain produced is dropped (an invalid trace; a record the kernel
            // found invalid, its status the validation's 1, 2, 3 or XFG_INVALID_ARGUMENT)
            if (j.status == XFG_INVALID_TRACE || (b->records.p && record_refusal(j.status))) {
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

// lane l's worker: the queue's loop (unit_queue.hpp) with one unit's proving and copy-out as the work
static void worker_main(xfg_ctx* c, int l) {
    (void)hipSetDevice(c->device);
    Lane* L = c->lanes[l].get();
    c->queue.run(l, split_min(), [L](Batch* b, int b0, int b1, bool timing) {
        L->timing = timing;
        // the unit's own slice of the batch's traces, refusals and key words (halved units too)
        TraceSrc ts = b->trace;
        if (ts.p) ts.p += (size_t)b0 * ts.layout.trace_stride;
        if (!b->refused.empty()) ts.refused = b->refused.data() + b0;
        if (!b->keys.empty()) ts.keys = b->keys.data() + b0;
        RecordSrc rs = b->records;
        if (rs.p) rs.p += b0;
        prove_lane(L, b->T, b->ce_div, b->jobs.data() + b0, b1 - b0, ts, b->n, b->o, rs);
        copy_unit(b, b0, b1);
    });
}

static void ensure_workers(xfg_ctx* c) {
    const int nl = max_lanes();
    ensure_lanes(c, nl);
    while ((int)c->workers.size() < nl) {
        int l = (int)c->workers.size();
        c->workers.emplace_back(worker_main, c, l);
    }
}

// tables may only be replaced with no submitted unit queued or running: the queue is drained first
static void bind_tables(xfg_ctx* c, Batch* b) {
    const int LM = (int)(ilog2(b->n) + ilog2(b->o.beta));
    if (c->tables.LM < LM || !fourstep_ready(c, (int)ilog2(b->n), (int)ilog2(b->o.beta))) {
        c->queue.drain();
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
    const int U = c->queue.whole_units() ? std::max(1, B) : unit_size(beta);
    for (int b0 = 0; b0 < B; b0 += U) u.push_back(Unit{b0, std::min(B, b0 + U), -1});
    return u;
}

// a batch with its jobs (and trace source) filled: the caller's `count` buffers (outs may be null),
// the shape and the tables onto it, then its units to the lane workers. Returns the ticket
static uint64_t submit_batch(xfg_ctx* c, std::unique_ptr<Batch> bp, u64 n, const Opts& o, uint32_t count,
                             uint8_t* const* outs, size_t* out_lens, int* statuses, const std::vector<Unit>& units) {
    if (outs) bp->outs.assign(outs, outs + count);
    bp->out_lens = out_lens;
    bp->statuses = statuses;
    bp->n = n;
    bp->o = o;
    bind_tables(c, bp.get());
    ensure_workers(c);
    bp->st.assign(bp->jobs.size(), XFG_OK);
    return c->queue.submit(std::move(bp), units);
}

// a finished job's copy-out status as the context's error text
static void note_status(xfg_ctx* c, const Batch& b, size_t k) {
    if (b.st[k] == XFG_BUFFER_TOO_SMALL) c->err = "output buffer too small";
    if (b.st[k] == XFG_PROVER_ERROR)
        c->err = b.jobs[k].pow_exhausted ? "Prover error: proof-of-work search exhausted"
                                         : "Prover error: proof generation failed (degenerate transcript or DEEP degree)";
}

// the text of an invalid record's status as the host marshaller words it; the two amounts a mint mismatch names are read
// from the caller's record (device memory of the current device: one 16-byte copy)
static std::string record_text_of(const xfg_burn_record* rec, int status, bool on_device) {
    uint64_t amounts[2] = {0, 0};  // burn, mint: the record's first two words
    if (status == XFG_MINT_MISMATCH) {
        if (on_device) HIPCHK(hipMemcpy(amounts, rec, sizeof amounts, hipMemcpyDeviceToHost));
        else memcpy(amounts, rec, sizeof amounts);
    }
    return record_status_text(status, amounts[0], amounts[1]);
}

// `count` host statements, their arguments and options checked (xfg_prove_batch_submit, host records): validation
// and marshalling (four Keccak-256 per proof) through marshal_one(i, air, text) on the host pool, since the
// submitting thread is the start of every batch's latency; the valid statements become the batch's jobs.
// zero_refused: an invalid statement's out_lens[i] is set to 0 (records) or left as the caller gave it (inputs)
template <class Marshal>
static int submit_statements(xfg_ctx* c, uint32_t count, Marshal marshal_one, bool zero_refused, u64 n, const Opts& o,
                             uint8_t* const* outs, size_t* out_lens, int* statuses, uint64_t* ticket) {
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        std::unique_ptr<Batch> bp(new Batch());
        std::vector<AirConst> airs(count);
        std::vector<std::string> errs(count);
        host_pool().parallel_for((int)count, [&](int i) { statuses[i] = marshal_one((uint32_t)i, airs[i], errs[i]); });
        for (uint32_t i = 0; i < count; i++) {
            if (statuses[i]) {
                c->err = errs[i];
                if (zero_refused) out_lens[i] = 0;
                continue;
            }
            bp->jobs.emplace_back();
            bp->jobs.back().air = airs[i];
            bp->which.push_back(i);
        }
        const std::vector<Unit> units = split_units(c, (int)bp->jobs.size(), o.beta);
        *ticket = submit_batch(c, std::move(bp), n, o, count, outs, out_lens, statuses, units);
        return XFG_OK;
    });
}

// a synchronous entry behind its _submit: what the submission returned, or else the wait for its ticket
static int wait_submitted(xfg_ctx* c, int submitted, uint64_t ticket) {
    return submitted ? submitted : xfg_batch_wait(c, ticket);
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
    c->queue.drain();
    c->queue.stop();
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
    if (int st = marshal(in, a, err)) return st;
    air_out(a, out);
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
        bp->trace.kind = TraceSrc::HOST_DIRECT;
        bp->trace.p = trace;
        bp->trace.layout = dense_layout(n);
        std::unique_ptr<Batch> b =
            c->queue.wait(submit_batch(c, std::move(bp), n, o, 1, &out, out_len, nullptr, {Unit{0, 1, -1}}));
        if (b->err) std::rethrow_exception(b->err);
        note_status(c, *b, 0);
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
    auto marshal_one = [inputs](uint32_t i, AirConst& a, std::string& err) { return marshal(&inputs[i], a, err); };
    return submit_statements(c, count, marshal_one, false, n, o, outs, out_lens, statuses, ticket);
}

int xfg_batch_wait(xfg_ctx* c, uint64_t ticket) {
    if (!c) return XFG_INVALID_ARGUMENT;
    return guarded(c, [&]() -> int {
        std::unique_ptr<Batch> b = c->queue.wait(ticket);
        if (!b) {
            c->err = "unknown batch ticket";
            return XFG_INVALID_ARGUMENT;
        }
        if (b->err) std::rethrow_exception(b->err);
        // device records: the text of what the record kernel found, as the host path words it at submission
        if (b->records.p) {
            HIPCHK(hipSetDevice(c->device));
            for (size_t k = 0; k < b->jobs.size(); k++)
                if (record_refusal(b->st[k])) c->err = record_text_of(b->records.p + k, b->st[k], true);
        }
        for (size_t k = 0; k < b->jobs.size(); k++) {
            b->statuses[b->which[k]] = b->st[k];
            note_status(c, *b, k);
        }
        // caller-supplied traces: what the check found, decoded (the cell of a failed assertion is read
        // from the caller's buffer, which stays theirs until here)
        if (!b->keys.empty()) {
            if (b->trace.on_device()) HIPCHK(hipSetDevice(c->device));
            for (size_t k = 0; k < b->jobs.size(); k++) {
                const xfg_trace_fault f = trace_fault_of(b->keys[k], b->jobs[k].air, b->trace, k, &c->err);
                if (b->faults) b->faults[b->which[k]] = f;
            }
        }
        return XFG_OK;
    });
}

int xfg_prove_batch(xfg_ctx* c, uint32_t count, const xfg_burn_inputs* inputs, uint64_t trace_length,
                    const xfg_options* opts, uint8_t* const* outs, size_t* out_lens, int* statuses) {
    uint64_t t = 0;
    const int r = xfg_prove_batch_submit(c, count, inputs, trace_length, opts, outs, out_lens, statuses, &t);
    return wait_submitted(c, r, t);
}

// XFG_TRACE_ON_DEVICE, XFG_RECORDS_ON_DEVICE: p (`noun` in the texts) must be device memory of the context's device
// that this process's HIP runtime allocated, and the allocation must hold all `bytes` (the lanes read that range).
// False, with what is wrong in c->err, otherwise. Asks the runtime only: nothing is launched or copied
static bool device_range_ok(xfg_ctx* c, const void* p, size_t bytes, const char* noun, const char* too_small) {
    static const char* const UNKNOWN = " is not a device pointer known to the library's HIP runtime";
    hipPointerAttribute_t a{};
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        c->err = std::string(noun) + UNKNOWN;
    } else if (a.type != hipMemoryTypeDevice || a.device != c->device) {
        c->err = std::string(noun) + " is not device memory of the context's device";
    } else if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        c->err = std::string(noun) + UNKNOWN;
    } else if ((const char*)p + bytes > (const char*)base + size) {
        c->err = too_small;
    } else {
        return true;
    }
    return false;
}
static bool device_traces_ok(xfg_ctx* c, const void* traces, size_t bytes) {
    return device_range_ok(c, traces, bytes, "traces", "the device allocation is smaller than [count][7][n] traces");
}
// `count` records, which the record kernel reads as 8-byte words
static bool device_records_ok(xfg_ctx* c, const xfg_burn_record* records, uint32_t count) {
    if ((uintptr_t)records % alignof(xfg_burn_record)) {
        c->err = "records is not 8-byte aligned";
        return false;
    }
    return device_range_ok(c, records, (size_t)count * sizeof(xfg_burn_record), "records",
                           "the device allocation is smaller than 128 * count bytes of records");
}

// the dense layout passes for every n and count that the checks in front of it let through (submit_trace_batch:
// n <= 2^21 and count < 2^32, 7 n count < 2^56; check_traces: n <= 2^32 and count < 2^16, 7 n count < 2^51)
static const char* const EXTENT_REFUSAL = "trace layout: the extent of the traces overflows or is above 2^58 words";

// xfg_prove_trace_batch_submit (L: the dense layout) and xfg_prove_trace_batch_strided_submit
static int submit_trace_batch(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                              const TraceLayout& L, const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags,
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
    std::vector<AirConst> ha;
    if (int st = guarded(c, [&] { return airs_of(c, airs, count, ha) ? XFG_OK : XFG_INVALID_ARGUMENT; })) return st;
    const bool dev = (flags & XFG_TRACE_ON_DEVICE) != 0;
    u64 extent = 0;  // words from the first cell to the last
    if (!trace_extent(L, count, n, &extent)) {
        c->err = EXTENT_REFUSAL;
        return XFG_INVALID_ARGUMENT;
    }
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        if (dev && !device_traces_ok(c, traces, (size_t)extent * 8)) return XFG_INVALID_ARGUMENT;
        std::unique_ptr<Batch> bp(new Batch());
        bp->jobs.resize(count);
        bp->which.resize(count);
        bp->refused.assign(count, 0);
        bp->keys.assign(count, TRACE_KEY_VALID);
        for (uint32_t i = 0; i < count; i++) {
            bp->jobs[i].air = ha[i];
            bp->which[i] = i;
            statuses[i] = XFG_OK;
        }
        if (!dev) {
            // all_canonical per proof on the host pool (the submitting thread starts every batch's latency)
            u64* keys = bp->keys.data();
            host_pool().parallel_for((int)count, [&](int i) {
                keys[i] = host_noncanonical_key(traces + (size_t)i * L.trace_stride, L, n);
            });
            for (uint32_t i = 0; i < count; i++)
                if (keys[i] != TRACE_KEY_VALID) {
                    bp->refused[i] = statuses[i] = XFG_INVALID_ARGUMENT;
                    c->err = "trace element is not a canonical field element";
                }
            c->stage_traces = true;
        }
        bp->trace.kind = dev ? TraceSrc::DEVICE : TraceSrc::HOST_STAGED;
        bp->trace.p = traces;
        bp->trace.layout = L;
        bp->trace.validate = (flags & XFG_TRACE_VALIDATE) != 0;
        bp->faults = faults;
        *ticket = submit_batch(c, std::move(bp), n, o, count, outs, out_lens, statuses,
                               split_units(c, (int)count, o.beta));
        return XFG_OK;
    });
}

int xfg_prove_trace_batch_submit(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                                 const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags,
                                 uint8_t* const* outs, size_t* out_lens, int* statuses, xfg_trace_fault* faults,
                                 uint64_t* ticket) {
    return submit_trace_batch(c, count, traces, width, n, dense_layout(n), airs, opts, flags, outs, out_lens, statuses,
                              faults, ticket);
}

int xfg_prove_trace_batch(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                          const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags, uint8_t* const* outs,
                          size_t* out_lens, int* statuses, xfg_trace_fault* faults) {
    uint64_t t = 0;
    const int r = xfg_prove_trace_batch_submit(c, count, traces, width, n, airs, opts, flags, outs, out_lens, statuses,
                                               faults, &t);
    return wait_submitted(c, r, t);
}

int xfg_prove_trace_batch_strided_submit(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n,
                                         const xfg_trace_layout* layout, const xfg_air_consts* airs,
                                         const xfg_options* opts, uint32_t flags, uint8_t* const* outs, size_t* out_lens,
                                         int* statuses, xfg_trace_fault* faults, uint64_t* ticket) {
    return submit_trace_batch(c, count, traces, 7, n, layout_of(layout, n), airs, opts, flags, outs, out_lens, statuses,
                              faults, ticket);
}

int xfg_prove_trace_batch_strided(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n,
                                  const xfg_trace_layout* layout, const xfg_air_consts* airs, const xfg_options* opts,
                                  uint32_t flags, uint8_t* const* outs, size_t* out_lens, int* statuses,
                                  xfg_trace_fault* faults) {
    uint64_t t = 0;
    const int r = xfg_prove_trace_batch_strided_submit(c, count, traces, n, layout, airs, opts, flags, outs, out_lens,
                                                       statuses, faults, &t);
    return wait_submitted(c, r, t);
}

// xfg_check_traces (L: the dense layout) and xfg_check_traces_strided
static int check_traces(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n, const TraceLayout& L,
                        const xfg_air_consts* airs, uint32_t flags, xfg_trace_fault* faults) {
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
    std::vector<AirConst> ha;
    if (int st = guarded(c, [&] { return airs_of(c, airs, count, ha) ? XFG_OK : XFG_INVALID_ARGUMENT; })) return st;
    TraceSrc src;
    src.kind = (flags & XFG_TRACE_ON_DEVICE) ? TraceSrc::DEVICE : TraceSrc::HOST_STAGED;
    src.p = traces;
    src.layout = L;
    u64 extent = 0;
    if (!trace_extent(L, count, n, &extent)) {
        c->err = EXTENT_REFUSAL;
        return XFG_INVALID_ARGUMENT;
    }
    return on_lane0(c, [&](Lane* lane) -> int {
        if (src.on_device() && !device_traces_ok(c, traces, (size_t)extent * 8)) return XFG_INVALID_ARGUMENT;
        const int logn = (int)ilog2(n);
        lane->air.ensure(count);
        lane->tkeys.ensure(count);
        HIPCHK(hipMemcpy(lane->air.p, ha.data(), count * sizeof(AirConst), hipMemcpyHostToDevice));
        if (src.on_device()) {
            // no copy: the ingest's first pass, constraints included, straight on the caller's buffer (only read);
            // its column classes go to the lane's buffers and are not used here
            lane->const_col.ensure(const_flag_bytes((size_t)count * 7));
            lane->const_val.ensure((size_t)count * 7);
            launch_trace_ingest_probe(StridedRows{traces, L}, lane->air.p, (int)count, logn, true, lane->tkeys.p,
                                      lane->const_col.p, lane->const_val.p, lane->stream);
        } else {
            // host traces: the kernel works on the lane's dense copy (it canonicalises what it reports as >= p)
            const size_t cells = (size_t)count * 7 * n;
            lane->trace.ensure(cells);
            if (is_dense(L, n)) {  // uploaded as they lie (a gather first: a tenth of the rate, profiles/r21)
                HIPCHK(hipMemcpyAsync(lane->trace.p, traces, cells * 8, hipMemcpyHostToDevice, lane->stream));
            } else {  // gathered, one trace per task
                const std::unique_ptr<u64[]> dense(new u64[cells]);
                host_pool().parallel_for((int)count, [&](int i) {
                    gather_trace(traces + (size_t)i * L.trace_stride, L, n, dense.get() + (size_t)i * 7 * n);
                });
                HIPCHK(hipMemcpy(lane->trace.p, dense.get(), cells * 8, hipMemcpyHostToDevice));
            }
            launch_trace_check(lane->trace.p, lane->air.p, lane->tkeys.p, logn, (int)count, true, lane->stream);
        }
        std::vector<u64> keys(count);
        HIPCHK(hipMemcpyAsync(keys.data(), lane->tkeys.p, count * 8, hipMemcpyDeviceToHost, lane->stream));
        HIPCHK(hipStreamSynchronize(lane->stream));
        for (uint32_t i = 0; i < count; i++) faults[i] = trace_fault_of(keys[i], ha[i], src, i, &c->err);
        return XFG_OK;
    });
}

int xfg_check_traces(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n, const xfg_air_consts* airs,
                     uint32_t flags, xfg_trace_fault* faults) {
    return check_traces(c, count, traces, n, dense_layout(n), airs, flags, faults);
}

int xfg_check_traces_strided(xfg_ctx* c, uint32_t count, const uint64_t* traces, uint64_t n,
                             const xfg_trace_layout* layout, const xfg_air_consts* airs, uint32_t flags,
                             xfg_trace_fault* faults) {
    return check_traces(c, count, traces, n, layout_of(layout, n), airs, flags, faults);
}

int xfg_prove_records_submit(xfg_ctx* c, uint32_t count, const xfg_burn_record* records, uint64_t trace_length,
                             const xfg_options* opts, uint32_t flags, uint8_t* const* outs, size_t* out_lens,
                             int* statuses, uint64_t* ticket) {
    if (!c) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    if (!records || !opts || !out_lens || !statuses || !ticket || count == 0) {
        c->err = count == 0 ? "empty batch" : "null argument";
        return XFG_INVALID_ARGUMENT;
    }
    *ticket = 0;
    if (flags & ~XFG_RECORDS_ON_DEVICE) {
        c->err = "unknown record flag";
        return XFG_INVALID_ARGUMENT;
    }
    const u64 n = trace_length ? trace_length : 64;
    const Opts o = to_opts(opts);
    if (int st = check_request(c, n, o)) return st;
    if (!(flags & XFG_RECORDS_ON_DEVICE)) {
        auto marshal_one = [records](uint32_t i, AirConst& a, std::string& err) { return marshal_record(records[i], a, err); };
        return submit_statements(c, count, marshal_one, true, n, o, outs, out_lens, statuses, ticket);
    }
    return guarded(c, [&]() -> int {
        HIPCHK(hipSetDevice(c->device));
        if (!device_records_ok(c, records, count)) return XFG_INVALID_ARGUMENT;
        // every record keeps its slot: the units' kernels validate and marshal them, nothing is read here
        std::unique_ptr<Batch> bp(new Batch());
        bp->jobs.resize(count);
        bp->which.resize(count);
        for (uint32_t i = 0; i < count; i++) {
            bp->which[i] = i;
            statuses[i] = XFG_OK;
        }
        bp->records.p = records;
        *ticket = submit_batch(c, std::move(bp), n, o, count, outs, out_lens, statuses, split_units(c, (int)count, o.beta));
        return XFG_OK;
    });
}

int xfg_prove_records(xfg_ctx* c, uint32_t count, const xfg_burn_record* records, uint64_t trace_length,
                      const xfg_options* opts, uint32_t flags, uint8_t* const* outs, size_t* out_lens, int* statuses) {
    uint64_t t = 0;
    const int r = xfg_prove_records_submit(c, count, records, trace_length, opts, flags, outs, out_lens, statuses, &t);
    return wait_submitted(c, r, t);
}

int xfg_air_consts_from_records(xfg_ctx* c, uint32_t count, const xfg_burn_record* records, uint32_t flags,
                                xfg_air_consts* airs_out, int* statuses) {
    const bool dev = (flags & XFG_RECORDS_ON_DEVICE) != 0;
    if (c) c->err.clear();
    if (!records || !airs_out || !statuses || count == 0 || (flags & ~XFG_RECORDS_ON_DEVICE) || (dev && !c)) {
        if (c) c->err = count == 0 ? "empty batch" : "null argument or unknown record flag";
        return XFG_INVALID_ARGUMENT;
    }
    std::vector<AirConst> airs(count);
    if (!dev) {
        std::string err;
        for (uint32_t i = 0; i < count; i++) {
            if ((statuses[i] = marshal_record(records[i], airs[i], err)) && c) c->err = err;
            air_out(airs[i], &airs_out[i]);
        }
        return XFG_OK;
    }
    return on_lane0(c, [&](Lane* lane) -> int {
        if (!device_records_ok(c, records, count)) return XFG_INVALID_ARGUMENT;
        lane->air.ensure(count);
        lane->dcoin.ensure(count);
        lane->rstatus.ensure(count);
        // the coins are not returned: any context will do
        xfg_options any;
        xfg_default_options(&any);
        launch_burn_marshal(records, (int)count, coin_context(64, to_opts(&any)), lane->air.p, lane->dcoin.p,
                            lane->rstatus.p, lane->stream);
        HIPCHK(hipMemcpyAsync(airs.data(), lane->air.p, count * sizeof(AirConst), hipMemcpyDeviceToHost, lane->stream));
        HIPCHK(hipMemcpyAsync(statuses, lane->rstatus.p, count * sizeof(int), hipMemcpyDeviceToHost, lane->stream));
        HIPCHK(hipStreamSynchronize(lane->stream));
        for (uint32_t i = 0; i < count; i++) {
            if (statuses[i]) c->err = record_text_of(records + i, statuses[i], true);
            air_out(airs[i], &airs_out[i]);
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
        xfg_burn_record r{};
        r.burn_amount = r.mint_amount = REC_STANDARD_BURN;
        for (int i = 0; i < 32; i++) r.tx_prefix_hash[i] = (uint8_t)(i + 1);
        r.recipient[0] = 1;
        r.secret[0] = 2;
        r.network_id = 1;
        r.target_chain_id = 42161;
        r.commitment_version = 1;
        AirConst a;
        std::string err;
        if (marshal_record(r, a, err)) return XFG_PROVER_ERROR;
        // every lane proves one full unit, twice (lane-pinned units)
        ensure_workers(c);
        const int nl = (int)c->workers.size(), U = std::min<int>((int)count, unit_size(o.beta));
        for (int pass = 0; pass < 2; pass++) {
            std::unique_ptr<Batch> bp(new Batch());
            bp->jobs.resize((size_t)nl * U);
            for (auto& j : bp->jobs) j.air = a;
            bp->trace.size_staging = c->stage_traces;
            std::vector<Unit> units;
            for (int l = 0; l < nl; l++) units.push_back(Unit{l * U, (l + 1) * U, l});
            std::unique_ptr<Batch> b = c->queue.wait(submit_batch(c, std::move(bp), n, o, 0, nullptr, nullptr, nullptr, units));
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
    // each lane's flag follows where the lane is taken: a worker's pick, on_lane0
    c->queue.set_whole_units(enabled != 0);
    return XFG_OK;
}

int xfg_stage_times(const xfg_ctx* c, double* ms, const char** names, int max) {
    if (!c) return 0;
    int k = std::min<int>(max, ST_COUNT);
    const int last = c->queue.last_lane();
    for (int i = 0; i < k; i++) {
        if (ms) ms[i] = c->lanes.empty() ? 0.0 : c->lanes[last]->stage_ms[i];
        if (names) names[i] = STAGE_NAMES[i];
    }
    return k;
}

}  // extern "C"
