/*
 * xfg_stark.h -- C ABI of the MI355X-native XFG burn-proof STARK prover (libxfgstark.so).
 *
 * Drop-in boundary for the reference's proving path. Rust is not available in this build
 * environment, so the host side above this ABI is C++ (inside the .so) and the reference-side
 * binding a Rust maintainer would add is shown in INTEGRATION.md. Every entry point replaces a
 * reference interface:
 *
 *   xfg_prove_burn_mint  <- XfgBurnMintProver::prove_burn_mint      src/burn_mint_prover.rs:62-129
 *                           (validate_inputs :132-180, secret_to_field_element :195-208,
 *                            compute_recipient_hash :211-221, air.prove(trace) :124-126)
 *   xfg_prove_trace      <- <XfgBurnMintAir as winterfell::Prover>::prove(trace)
 *                           src/burn_mint_air.rs:479-531 (ExecutionTrace-level entry; trace layout
 *                           of build_trace :442-476, column-major)
 *   xfg_prove_trace_batch <- the same for many traces at once, with Trace::validate (which Prover::prove runs
 *                           in debug builds) on request; xfg_check_traces is that check alone
 *   xfg_prove_batch      <- the serial loops of the reference callers (e.g. benchmark harness
 *                           src/benchmarks/mod.rs:301-342, BatchBurnMintVerifier's pattern
 *                           src/burn_mint_verifier.rs:326-338) -- independent proofs, one launch set
 *   xfg_prove_records    <- the same loops for statements that arrive as fixed-size packed records, in host
 *                           memory or in device memory (validated, marshalled and hashed on the device)
 *   xfg_default_options  <- XfgBurnMintProver::new(_) ProofOptions::new(42, 8, 4, None, 8, 31)
 *                           src/burn_mint_prover.rs:27-41 (argument order: queries, blowup,
 *                           grinding, extension, FRI folding, FRI remainder max degree)
 *   xfg_proof_size_bound <- XfgBurnMintProver::get_proof_size  src/burn_mint_prover.rs:224-227
 *   xfg_last_error       <- XfgStarkError::CryptoError(String) text  src/burn_mint_prover.rs:143-177
 *
 * Output bytes are the proof's `StarkProof::to_bytes()` serialisation as restated in DESIGN.md
 * ("Proof format"); the caller owns all host buffers, the library owns device memory (pooled per
 * context). `out == NULL` (or *out_len too small) returns the required size in *out_len.
 * A context is bound to one HIP device; it owns XFG_LANES (default 7) lanes, each a HIP stream with
 * its workspace and a host worker thread; the per-proof host work of the lanes (transcript replay,
 * opening plans, serialisation) runs on a process-wide pool of XFG_HOST_THREADS (default 8) threads.
 * Submit from one thread per context.
 */
#ifndef XFG_STARK_H
#define XFG_STARK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct xfg_ctx xfg_ctx;

typedef enum {
    XFG_OK = 0,
    XFG_INVALID_BURN_AMOUNT = 1, /* burn not 8,000,000 or 8,000,000,000 atomic units */
    XFG_MINT_MISMATCH = 2,       /* mint != burn (1:1) */
    XFG_ZERO_TX_HASH = 3,        /* u64 LE of tx_prefix_hash[0..8] == 0 */
    XFG_BAD_RECIPIENT_LEN = 4,   /* recipient address not 20 bytes */
    XFG_SHORT_SECRET = 5,        /* secret shorter than 8 bytes (reference: error <4, panic 4..7) */
    XFG_PROVER_ERROR = 6,        /* Winterfell prover error / options outside the supported set (blowup
                                    factor not a power of two in [2, 128]; at blowup 32, 64 or 128 an LDE
                                    domain trace_length * blowup above 2^24, the message naming both and
                                    the limit; FRI folding factor not 2, 4, 8 or 16; a last FRI layer
                                    smaller than the blowup -- folding factors 2, 4, 16 at any blowup, every
                                    factor at blowup 32, 64, 128; an NTT size without a kernel); also a
                                    proof whose bounded
                                    proof-of-work search on the device found no nonce up to
                                    2^(grinding_factor + 8) ("proof-of-work search exhausted", probability
                                    e^-256; the other proofs of the batch are unaffected) */
    XFG_DEVICE_ERROR = 7,        /* HIP runtime failure */
    XFG_BUFFER_TOO_SMALL = 8,
    XFG_INVALID_ARGUMENT = 9,
    XFG_VERIFY_FAILED = 10,      /* proof rejected (verifier) or not a well-formed proof (parser) */
    XFG_INVALID_TRACE = 11       /* trace does not satisfy the AIR (only reported when validation is requested) */
} xfg_status;

/* winterfell::ProofOptions (0.8) */
typedef struct {
    uint32_t num_queries;
    uint32_t blowup_factor;   /* a power of two in [2, 128]; above 16: trace_length * blowup_factor <= 2^24 */
    uint32_t grinding_factor;
    uint32_t field_extension; /* 1 = FieldExtension::None */
    uint32_t fri_folding_factor; /* 2, 4, 8 or 16 */
    uint32_t fri_remainder_max_degree;
} xfg_options;

/* arguments of prove_burn_mint (src/burn_mint_prover.rs:62-72) */
typedef struct {
    uint64_t burn_amount;
    uint64_t mint_amount;
    uint8_t tx_prefix_hash[32];
    const uint8_t* recipient_address;
    size_t recipient_len;
    const uint8_t* secret;
    size_t secret_len;
    uint32_t network_id;
    uint32_t target_chain_id;
    uint32_t commitment_version;
} xfg_burn_inputs;

/* AIR instance for ExecutionTrace-level proving: BurnMintPublicInputs::to_elements
 * (src/burn_mint_air.rs:54-71) + the two Keccak-derived constants (:124-133, :174-202) */
typedef struct {
    uint64_t pub_inputs[12];
    uint64_t nullifier;
    uint64_t commitment;
} xfg_air_consts;

xfg_ctx* xfg_ctx_create(int device_id);
void xfg_ctx_destroy(xfg_ctx* ctx);
int xfg_default_options(xfg_options* out);
/* length of the error text of the last failing call on ctx (copied NUL-terminated into buf) */
int xfg_last_error(const xfg_ctx* ctx, char* buf, size_t len);
/* the largest proof the prover emits for (trace_length, opts): a tight upper bound computed section
 * by section (every proof fits; configs[2]: 98.8 KB for ~78 KB proofs), so callers can size fixed
 * per-proof output slots, e.g. the exchange records of a sharded run; 0 for unsupported shapes */
size_t xfg_proof_size_bound(uint64_t trace_length, const xfg_options* opts);

/* prove_burn_mint; trace_length 0 -> 64 (the reference's fixed TraceInfo::new(7, 64)) */
int xfg_prove_burn_mint(xfg_ctx* ctx, const xfg_burn_inputs* in, uint64_t trace_length, const xfg_options* opts,
                        uint8_t* out, size_t* out_len);
/* prove over a caller-supplied execution trace, column-major [width][n], width must be 7; trace cells
 * and AIR constants must be canonical field elements (< p), else XFG_INVALID_ARGUMENT */
int xfg_prove_trace(xfg_ctx* ctx, const uint64_t* trace, uint32_t width, uint64_t n, const xfg_air_consts* air,
                    const xfg_options* opts, uint8_t* out, size_t* out_len);
/* batch of independent proofs on this context's device; statuses[i] per proof, returns XFG_OK if
 * the batch ran (individual proofs may still carry validation errors) */
int xfg_prove_batch(xfg_ctx* ctx, uint32_t count, const xfg_burn_inputs* inputs, uint64_t trace_length,
                    const xfg_options* opts, uint8_t* const* outs, size_t* out_lens, int* statuses);

/* asynchronous form of xfg_prove_batch for pipelined callers (a proving service, bench.py):
 * inputs are validated and marshalled before this returns (statuses[i] of invalid inputs are set
 * now); outs / out_lens / statuses must stay valid until xfg_batch_wait(ticket) returns. Batches
 * submitted back to back share the context's lane workers, so the host-side tail of one (query
 * openings, serialisation) overlaps the kernels of the next. */
int xfg_prove_batch_submit(xfg_ctx* ctx, uint32_t count, const xfg_burn_inputs* inputs, uint64_t trace_length,
                           const xfg_options* opts, uint8_t* const* outs, size_t* out_lens, int* statuses,
                           uint64_t* ticket);
/* blocks until the batch is proven and its outputs written; returns like xfg_prove_batch */
int xfg_batch_wait(xfg_ctx* ctx, uint64_t ticket);

/* ---- batches of caller-supplied execution traces, optionally validated on the device ----
 * What Trace::validate (winter-air 0.8, run by Prover::prove in debug builds) reports first for a trace:
 * the assertions in the order of the AIR, then the transition constraints step by step (steps
 * 0 .. n-2: the last step has no transition), constraint by constraint. */
typedef struct {
    uint32_t kind;     /* 0 = trace is valid, 1 = assertion, 2 = transition constraint, 3 = a cell is not a
                          canonical field element (>= p): the first such cell in step, then column order */
    uint32_t index;    /* assertion number 0..7 (order of the AIR: columns 0..6 at step 0, then column 4 at
                          step n-1) or transition constraint number 0..6; kind 3: 0 */
    uint32_t column;   /* assertions and kind 3: the column of the cell; transitions: 0 */
    uint64_t step;
    uint64_t expected; /* assertions: asserted value; otherwise 0 */
    uint64_t found;    /* assertions and kind 3: the trace cell; transitions: 0 */
} xfg_trace_fault;

#define XFG_TRACE_VALIDATE   1u  /* run the check; invalid traces get XFG_INVALID_TRACE and no proof */
#define XFG_TRACE_ON_DEVICE  2u  /* `traces` is a device pointer on the context's device */

/* the check alone on `count` (<= 65535) traces [count][7][n], column-major as for xfg_prove_trace, n a
 * power of two >= 8; synchronous, on lane 0 (refused while batches are pending). flags: 0 or
 * XFG_TRACE_ON_DEVICE. Returns XFG_OK when the check ran; faults[i] then says what trace i violates
 * (kind 0: nothing). The traces are only read. */
int xfg_check_traces(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint64_t n, const xfg_air_consts* airs,
                     uint32_t flags, xfg_trace_fault* faults);
/* xfg_prove_trace for `count` independent traces [count][7][n] with their AIR constants airs[count],
 * through the lanes like xfg_prove_batch: units of 32 proofs, each reading its own slice of `traces`.
 * width, options and AIR constants are checked as by xfg_prove_trace; a refused call launches nothing.
 * Host traces (no XFG_TRACE_ON_DEVICE) are checked for canonical cells before the call returns and go
 * up through pinned staging owned by the lanes; the staging is sized by the first such batch a lane
 * proves, or by xfg_prepare once the context has been given a host-trace batch. Device traces are copied
 * device-to-device on the lane's stream: the caller guarantees that the data is complete (every
 * producing stream synchronised) before the call; their cells are checked for canonicity on the device.
 * The caller's traces are never written. A proof whose trace holds a cell >= p gets
 * statuses[i] = XFG_INVALID_ARGUMENT, the others are unaffected.
 * XFG_TRACE_VALIDATE: each trace is checked on the lane's stream behind its upload; a trace that
 * violates the AIR gets statuses[i] = XFG_INVALID_TRACE, out_lens[i] = 0 and no proof (this takes
 * precedence over the XFG_PROVER_ERROR its DEEP degree may also earn); xfg_last_error carries
 * Trace::validate's message for the last such proof ("trace does not satisfy assertion
 * main_trace(column, step) == expected" / "main transition constraint index did not evaluate to ZERO
 * at step step"). The other proofs are byte-identical to proving them alone. Without the flag any
 * canonical trace is proven, as by xfg_prove_trace.
 * faults (may be NULL): faults[i] for every proof when the batch has been waited for (kind 0 unless
 * statuses[i] is XFG_INVALID_TRACE, or XFG_INVALID_ARGUMENT for a cell >= p).
 * Returns XFG_OK if the batch ran, like xfg_prove_batch. */
int xfg_prove_trace_batch(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                          const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags, uint8_t* const* outs,
                          size_t* out_lens, int* statuses, xfg_trace_fault* faults);
/* asynchronous form, waited for with xfg_batch_wait(ticket): traces, outs, out_lens, statuses and
 * faults stay the caller's, valid and unchanged, until the wait returns (airs only until this call
 * returns). statuses[i] of proofs refused here (host cell >= p) are set now. */
int xfg_prove_trace_batch_submit(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint32_t width, uint64_t n,
                                 const xfg_air_consts* airs, const xfg_options* opts, uint32_t flags,
                                 uint8_t* const* outs, size_t* out_lens, int* statuses, xfg_trace_fault* faults,
                                 uint64_t* ticket);

/* ---- the same three entries for traces in any strided layout, row-major included ----
 * where cell (trace i, column c, step s) lies: traces[i*trace_stride + c*col_stride + s*row_stride], in
 * 8-byte words. Any values, 0 included (a broadcast view); the cells may overlap, they are only read.
 * dense column-major = {7n, n, 1}; row-major = {7n, 1, 7}; rows padded to 8 words = {8n, 1, 8} */
typedef struct { uint64_t trace_stride, col_stride, row_stride; } xfg_trace_layout;

/* Each returns what its namesake without _strided returns on the dense array M[i][c][s] = the cell the layout
 * names (there is no width argument: a layout names seven columns): return value, statuses, out_lens, faults,
 * proof bytes and the xfg_last_error text; `found` of a fault is read from the caller's buffer through the
 * layout. Flags, limits and the pending-batch rule are those of the namesake. layout == NULL, or the dense
 * layout spelled out, is the namesake itself.
 * Device traces in another layout are not copied: one pass over the caller's buffer checks them and
 * classifies their columns, a second writes the columns that need a transform into the lane's workspace.
 * Host traces in another layout are checked through the strides and gathered into the lanes' pinned staging.
 * Refused with XFG_INVALID_ARGUMENT, nothing launched: what the namesake refuses; an extent -- the words from
 * the first cell to the last, (count-1)*trace_stride + 6*col_stride + (n-1)*row_stride + 1 -- that overflows
 * 64 bits or is above 2^58; for device traces an extent past the end of the allocation */
int xfg_check_traces_strided(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint64_t n,
                             const xfg_trace_layout* layout, const xfg_air_consts* airs, uint32_t flags,
                             xfg_trace_fault* faults);
int xfg_prove_trace_batch_strided(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint64_t n,
                                  const xfg_trace_layout* layout, const xfg_air_consts* airs, const xfg_options* opts,
                                  uint32_t flags, uint8_t* const* outs, size_t* out_lens, int* statuses,
                                  xfg_trace_fault* faults);
/* waited for with xfg_batch_wait(ticket) */
int xfg_prove_trace_batch_strided_submit(xfg_ctx* ctx, uint32_t count, const uint64_t* traces, uint64_t n,
                                         const xfg_trace_layout* layout, const xfg_air_consts* airs,
                                         const xfg_options* opts, uint32_t flags, uint8_t* const* outs,
                                         size_t* out_lens, int* statuses, xfg_trace_fault* faults, uint64_t* ticket);

/* ---- batches of burn statements as packed records, in host or in device memory ----
 * One statement as a fixed-size little-endian record of 128 bytes: what a queue, a collective or a Rust service
 * hands over, with no pointers in it. A record always carries a 20-byte recipient and a 32-byte secret, so the
 * statuses XFG_BAD_RECIPIENT_LEN and XFG_SHORT_SECRET cannot occur for one. reserved must be zero. */
typedef struct {
    uint64_t burn_amount;        /* offset 0 */
    uint64_t mint_amount;        /* 8 */
    uint8_t tx_prefix_hash[32];  /* 16 */
    uint8_t recipient[20];       /* 48 */
    uint8_t secret[32];          /* 68 */
    uint32_t network_id;         /* 100 */
    uint32_t target_chain_id;    /* 104 */
    uint32_t commitment_version; /* 108 */
    uint8_t reserved[16];        /* 112: zero, else XFG_INVALID_ARGUMENT for that record */
} xfg_burn_record;

#define XFG_RECORDS_ON_DEVICE 1u /* `records` is a device pointer on the context's device */

/* xfg_prove_batch for `count` records: statuses, proof bytes and the xfg_last_error text are what xfg_prove_batch
 * gives for the same statements (a record is checked in its order: burn amount, mint amount, tx hash, then the
 * reserved bytes); out_lens[i] of an invalid record is set to 0. trace_length 0 -> 64.
 * Host records (flags 0) are validated and marshalled on the host pool before the call returns.
 * XFG_RECORDS_ON_DEVICE: nothing is copied to the host and no statement is touched by it before the launch:
 * each unit of 32 proofs starts its chain with a kernel that validates and marshals its records, computes the
 * four Keccak-256 hashes of each statement and seeds its transcript; the AIR constants and statuses come back
 * with the unit's transcript inputs. An invalid record keeps its slot in its unit and gets no proof; the other
 * proofs are byte-identical to proving them alone. The records must be memory of the context's device that this
 * process's HIP runtime allocated, hold 128 * count bytes and be 8-byte aligned; the caller guarantees that they
 * are complete (every producing stream synchronised) before the call. They are only read.
 * Refused with XFG_INVALID_ARGUMENT, nothing launched: count 0, a null pointer, an unknown flag, device records
 * that fail the above. Returns XFG_OK if the batch ran, like xfg_prove_batch. */
int xfg_prove_records(xfg_ctx* ctx, uint32_t count, const xfg_burn_record* records, uint64_t trace_length,
                      const xfg_options* opts, uint32_t flags, uint8_t* const* outs, size_t* out_lens, int* statuses);
/* asynchronous form, waited for with xfg_batch_wait(ticket): records, outs, out_lens and statuses stay the
 * caller's, valid and unchanged, until the wait returns. statuses[i] of invalid host records are set now, those
 * of device records by the wait */
int xfg_prove_records_submit(xfg_ctx* ctx, uint32_t count, const xfg_burn_record* records, uint64_t trace_length,
                             const xfg_options* opts, uint32_t flags, uint8_t* const* outs, size_t* out_lens,
                             int* statuses, uint64_t* ticket);
/* the statement of each record as the verifiers take it: airs_out[i] and statuses[i] (the validation status; the
 * constants of an invalid record are marshalled all the same). Host records are computed on the host and ctx may
 * be NULL; with XFG_RECORDS_ON_DEVICE the prover's kernel runs on lane 0 (refused while batches are pending) */
int xfg_air_consts_from_records(xfg_ctx* ctx, uint32_t count, const xfg_burn_record* records, uint32_t flags,
                                xfg_air_consts* airs_out, int* statuses);

/* allocate every device / pinned-host workspace and load all code objects for batches of
 * `count` proofs of this shape (setup, not a prove; later calls never allocate) */
int xfg_prepare(xfg_ctx* ctx, uint32_t count, uint64_t trace_length, const xfg_options* opts);

/* AIR constants from raw inputs (marshalling + Keccak, host); returns a validation status */
int xfg_burn_air_consts(const xfg_burn_inputs* in, xfg_air_consts* out);

/* ---- proofs: parsing and verification (host; no device needed) ---- */
/* header of a parsed proof (StarkProof::from_bytes, winter-air 0.8) */
typedef struct {
    uint32_t trace_width;
    uint64_t trace_length;
    xfg_options options;
    uint32_t num_unique_queries;
    uint32_t num_fri_layers;
    uint32_t remainder_len;     /* FRI remainder coefficients (E elements, not coordinates) */
    uint64_t pow_nonce;
    uint8_t trace_root[32];
    uint8_t constraint_root[32];
    uint64_t ood_trace[14];     /* T_c(z), T_c(z g) interleaved (first coordinates with an extension) */
    uint64_t ood_composition;   /* H(z) */
    size_t size;                /* bytes consumed == len for a well-formed proof */
} xfg_proof_info;

/* StarkProof::from_bytes <- src/burn_mint_prover.rs:224-227 (to_bytes), src/bin/xfg-stark-cli.rs:533-558
 * structural parse of proof bytes; XFG_VERIFY_FAILED + ProofDeserializationError text on bad input */
int xfg_proof_parse(const uint8_t* proof, size_t len, xfg_proof_info* info, char* err, size_t err_len);

/* winterfell::verify::<XfgBurnMintAir, Blake3_256, DefaultRandomCoin> with
 * AcceptableOptions::OptionSet([*acceptable])  <- XfgBurnMintVerifier::verify_with_public_inputs /
 * verify_with_winterfell, src/burn_mint_verifier.rs:186-203, 265-283 (the reference passes a one-element
 * set, :271; xfg_verify_acceptable takes the whole policy argument). The statement is the AIR
 * constants (12 public inputs + nullifier + commitment, see xfg_burn_air_consts). XFG_OK = accepted;
 * XFG_VERIFY_FAILED = rejected, err receives the VerifierError (Debug form, e.g.
 * "InconsistentOodConstraintEvaluations"). */
int xfg_verify(const uint8_t* proof, size_t len, const xfg_air_consts* air, const xfg_options* acceptable, char* err,
               size_t err_len);
/* BatchBurnMintVerifier::verify_batch <- src/burn_mint_verifier.rs:386-408 (and batch_verify
 * :326-338): results[i] = xfg_verify status of proof i; `threads` host threads (0 = all cores) */
int xfg_verify_batch(uint32_t count, const uint8_t* const* proofs, const size_t* lens, const xfg_air_consts* airs,
                     const xfg_options* acceptable, int* results, uint32_t threads);

/* batched verification on the context's GPU: the host replays each transcript (threads), the device
 * recomputes every Merkle opening (leaf hashes, then one launch per tree level for all proofs) and
 * runs the per-query DEEP / FRI / remainder checks. results[i] as xfg_verify. */
int xfg_verify_batch_gpu(xfg_ctx* ctx, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                         const xfg_air_consts* airs, const xfg_options* acceptable, int* results);

/* ---- the verifiers' policy argument: winterfell::AcceptableOptions (winter-verifier 0.8) ----
 * Which proofs a verifier takes is the verifying side's decision: a set of option sets, or a minimum
 * conjectured security level. Kind 2 is reserved for AcceptableOptions::MinProvenSecurity, which is not
 * offered (its bound is a floating-point search over list-decoding parameters that cannot be restated
 * reliably here); kind 2 and every other unknown kind is refused. */
#define XFG_ACCEPT_OPTION_SET 0u               /* AcceptableOptions::OptionSet */
#define XFG_ACCEPT_MIN_CONJECTURED_SECURITY 1u /* AcceptableOptions::MinConjecturedSecurity */
typedef struct {
    uint32_t kind;
    uint32_t min_security;      /* bits, kind 1 */
    const xfg_options* options; /* kind 0: num_options entries, 1..32 */
    uint32_t num_options;
} xfg_acceptable;
/* StarkProof::security_level(conjectured = true) of a proof of this shape (winter-air 0.8
 * get_conjectured_security for the 64-bit field and Blake3_256): min(min(64 field_extension -
 * log2(trace_length blowup_factor), log2(blowup_factor) num_queries [+ grinding_factor when that product is at
 * least 80]) - 1, 128). The cap of 128 needs the cubic extension and is never reached here.
 * XFG_INVALID_ARGUMENT for a null pointer and for a shape outside the supported set (xfg_options, and a trace
 * length that is no power of two in [8, 2^21]) */
int xfg_security_level(uint64_t trace_length, const xfg_options* opts, uint32_t* bits);
/* xfg_verify, xfg_verify_batch and xfg_verify_batch_gpu under a policy; each of the three above is its
 * namesake here with the one-element set {*acceptable}: same verdicts, same error texts.
 * The order of the checks, as in Winterfell: (1) StarkProof::from_bytes errors; (2) the policy, on the
 * options and trace length the proof states, before its transcript is touched -- a set answers
 * "UnacceptableProofOptions" unless one member equals all six option fields, a minimum answers
 * "InsufficientConjecturedSecurity(<required>, <the proof's>)", and a proof that is below the minimum and
 * tampered with as well reports the policy error; (3) the library's own limits, which also answer
 * "UnacceptableProofOptions": the cubic field extension, a last FRI layer below the blowup factor, and the
 * LDE size limits of xfg_options. Under a minimum-security policy (3) rejects proofs that Winterfell would
 * go on to verify.
 * Refused with XFG_INVALID_ARGUMENT, nothing verified and nothing launched: a null policy, a kind other than
 * 0 or 1, kind 0 with null options or with num_options 0 or above 32 (and what the namesake refuses).
 * On the GPU one batch may hold proofs of any mix of options the policy takes, every folding factor included:
 * results[i] belongs to proofs[i] whatever their order. */
int xfg_verify_acceptable(const uint8_t* proof, size_t len, const xfg_air_consts* air,
                          const xfg_acceptable* acceptable, char* err, size_t err_len);
int xfg_verify_batch_acceptable(uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                                const xfg_air_consts* airs, const xfg_acceptable* acceptable, int* results,
                                uint32_t threads);
int xfg_verify_batch_gpu_acceptable(xfg_ctx* ctx, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                                    const xfg_air_consts* airs, const xfg_acceptable* acceptable, int* results);

/* ---- instrumentation (benchmarks / parity tests) ---- */
/* host BLAKE3 of the library (any length), for self-tests */
int xfg_selftest_blake3(const uint8_t* in, size_t len, uint8_t out[32]);
/* host-side field arithmetic of the library (mul, add, sub) for self-tests; canonical inputs */
int xfg_selftest_field(uint64_t a, uint64_t b, uint64_t* out3);
/* per-stage device milliseconds of the last prove call when timing is enabled (returns count) */
int xfg_set_timing(xfg_ctx* ctx, int enabled);
int xfg_stage_times(const xfg_ctx* ctx, double* ms, const char** names, int max);
/* times `iters` launches of the trace LDE kernels (7 columns x count proofs, resident device
 * buffers, HIP events on the context stream); returns average ms per launch set in *avg_ms.
 * blowup 2..128, above 16 with n * blowup <= 2^24 (else XFG_INVALID_ARGUMENT), as xfg_debug_lde */
int xfg_bench_lde(xfg_ctx* ctx, uint32_t count, uint64_t n, uint32_t blowup, uint32_t iters, double* avg_ms);
/* in-pipeline trace-LDE timing: HIP events around the trace LDE launch set of every proof unit
 * (on the lane stream that launches it). enabled = 1 resets and starts; enabled = 0 stops. The
 * totals so far (sum of launch-set durations, launch sets, polynomials transformed: constant columns,
 * which skip the transform, are not counted) are returned either way. */
int xfg_lde_probe(xfg_ctx* ctx, int enabled, double* total_ms, uint64_t* launch_sets, uint64_t* polys);
/* kernel-level parity hooks (host buffers in/out) */
/* forward LDE: coef [npoly][n] -> out [npoly][blowup n] in natural order, out[p][t + blowup m] =
 * P_p(7 w_N^(t + blowup m)), N = blowup n. blowup a power of two in 2..128; 32, 64 and 128 run as blowup / 16
 * blowup-16 transforms of twisted coefficients and need n * blowup <= 2^24 (else XFG_INVALID_ARGUMENT) */
int xfg_debug_lde(xfg_ctx* ctx, const uint64_t* coef, uint32_t npoly, uint64_t n, uint32_t blowup, uint64_t* out);
int xfg_debug_interpolate(xfg_ctx* ctx, const uint64_t* evals, uint32_t npoly, uint64_t n, int offset7,
                          uint64_t* out);
/* the prover's constant-column detection alone: trace [count][width][n] -> flags_out [count][width],
 * 1 where the column holds one value in every row, else 0 */
int xfg_debug_const_columns(xfg_ctx* ctx, const uint64_t* trace, uint32_t count, uint32_t width, uint64_t n,
                            uint8_t* flags_out);
/* the detection as the prover runs it on a unit of `count` traces, trace [count][7][n] ->
 * classes_out [count][7]: 0 a live column (it is transformed), 1 a constant one, 2 one that equals the same
 * column of trace 0 element for element (its planes are those of trace 0's column). A constant column
 * is 1 whatever it equals, trace 0's columns are never 2, and with count = 1 nothing is.
 * vals_out [count][7] (or NULL): element 0 of every column, the value of a constant one */
int xfg_debug_col_classes(xfg_ctx* ctx, const uint64_t* trace, uint32_t count, uint64_t n, uint8_t* classes_out,
                          uint64_t* vals_out);
/* a synthetic row generator for xfg_debug_trace_probe, one pattern per column c. With v = the instance's
 * pub_inputs[c] and f(row) = 3 row + c (64-bit wrapping), kind[c] is
 *   0  v in every row (constant per instance)
 *   1  f(row): every instance the same, not constant
 *   2  f(row) + v: a function of row and instance
 *   3  v, but v + 1 at row[c]: constant except at one row
 *   4  f(row), but f(row) + 1 at row[c] of the instances whose pub_inputs[7] equals `proof` */
typedef struct xfg_probe_pattern {
    uint32_t kind[7];
    uint32_t reserved;
    uint64_t row[7];
    uint64_t proof;
} xfg_probe_pattern;
/* the front end of a unit of `count` generated traces as the prover's chain runs it, without the
 * transforms: the trace buffer [count][7][n] is set to 0xFF bytes, the columns are classified from the rows
 * as the generator returns them (no trace in memory), and the generator then writes the live columns only.
 * generator 0: the burn AIR's rows from airs [count] (pattern unused, may be NULL); 1: the synthetic
 * generator of `pattern`. classes_out and vals_out [count][7] as for xfg_debug_col_classes, which they
 * equal on the same trace materialised; trace_out [count][7][n]: the buffer as left, the planes of
 * constant (1) and shared (2) columns still 0xFF bytes.
 * Refused with XFG_INVALID_ARGUMENT: a null pointer, count 0 or count * 7 > 65535, n no power of two in
 * [8, 2^24], an AIR constant that is not canonical, a generator other than 0 or 1, a kind above 4 */
int xfg_debug_trace_probe(xfg_ctx* ctx, uint32_t count, uint64_t n, const xfg_air_consts* airs, uint32_t generator,
                          const xfg_probe_pattern* pattern, uint8_t* classes_out, uint64_t* vals_out,
                          uint64_t* trace_out);
/* the front end of a unit of `count` device traces in a strided layout as the prover's chain runs it, without
 * the transforms: buf (host memory, buf_words words) is uploaded as it is into a device buffer of exactly that
 * size, the lane's trace buffer [count][7][n] is set to 0xFF bytes, and the two ingest launches run on lane 0:
 * one pass over the buffer for the check's words and the column classes, one that writes the canonical live
 * columns. The hook always takes these kernels, for the dense layout and layout == NULL (dense) too.
 * validate != 0: the AIR's assertions and constraints are checked besides the canonicity of the cells.
 * classes_out and vals_out [count][7] as for xfg_debug_col_classes (on the canonical cells); faults_out [count]
 * as xfg_check_traces_strided fills them (`found` read from buf through the layout); trace_out [count][7][n]: the
 * buffer as left, the planes of constant (1) and shared (2) columns still 0xFF bytes.
 * Refused with XFG_INVALID_ARGUMENT: a null pointer (layout excepted), count 0 or count * 7 > 65535, n no power
 * of two in [8, 2^24], an AIR constant that is not canonical, an extent that overflows, is above 2^58 or
 * above buf_words */
int xfg_debug_trace_ingest(xfg_ctx* ctx, uint32_t count, uint64_t n, const uint64_t* buf, uint64_t buf_words,
                           const xfg_trace_layout* layout, const xfg_air_consts* airs, int validate,
                           uint8_t* classes_out, uint64_t* vals_out, xfg_trace_fault* faults_out, uint64_t* trace_out);
/* xfg_debug_lde / xfg_debug_interpolate with a caller-supplied flag vector skip [npoly]: polynomials
 * with a non-zero flag take no transform and are filled in as constants (coefficient / evaluation 0 of
 * the input is the value), as the prover does for the columns it detects. The caller vouches that a
 * flagged polynomial is constant. Both set their device output and intermediate buffers to 0xFF bytes
 * (no field element) before they launch, so nothing an earlier call left there can pass for output. */
int xfg_debug_lde_skip(xfg_ctx* ctx, const uint64_t* coef, uint32_t npoly, uint64_t n, uint32_t blowup,
                       const uint8_t* skip, uint64_t* out);
int xfg_debug_interpolate_skip(xfg_ctx* ctx, const uint64_t* evals, uint32_t npoly, uint64_t n, int offset7,
                               const uint8_t* skip, uint64_t* out);
/* the inverse transform as the prover launches it for the composition polynomial and the FRI remainder:
 * only the first `keep` coefficients of each polynomial are written, `keep` words apart. evals
 * [npoly][n] -> out [npoly][keep] followed by 8 guard words. The device buffer is set to 0xFF bytes (no
 * field element) before the launch and npoly * keep + 8 words of it are copied back, so a store past
 * `keep` shows in the next polynomial's words or in the guard. 1 <= keep <= n, else XFG_INVALID_ARGUMENT */
int xfg_debug_interpolate_keep(xfg_ctx* ctx, const uint64_t* evals, uint32_t npoly, uint64_t n, uint64_t keep,
                               int offset7, uint64_t* out);
/* Goldilocks primitive self test on the device: out[i] = op(a[i], b[i]) with op 0 mul, 1 add,
 * 2 sub, 3 canonical(a), 4 a * 2^(b mod 96), 5 a + (b mod 2^32) * (2^32 - 1), 6 a - b with one
 * borrow fold (the weak subtraction of the NTT butterflies), 7 a + b with one carry fold (the weak
 * addition of the NTT butterflies, b < p), 8 a * b through the interleaved pair multiply (gl_mul2:
 * both a * b and b * a computed, all ones returned if they differ).
 * Ops 9..12 read consecutive elements as pairs, x = (a[2i], a[2i+1]), y = (b[2i], b[2i+1]), and write
 * out[2i], out[2i+1] (count must be even): 9 one gl_mul2 on the unrelated products a[2i] * b[2i] and
 * a[2i+1] * b[2i+1] (any u64 operands), and on canonical operands 10 e2_mul(x, y) in the quadratic
 * extension, 11 e2_mulb(x, b[2i]), 12 e2_inv(x) ((0, 0) for x = (0, 0)) */
int xfg_debug_field(xfg_ctx* ctx, uint32_t op, uint64_t count, const uint64_t* a, const uint64_t* b, uint64_t* out);
/* OOD evaluation + DEEP quotient kernels of the prover on `count` instances: coef [count][7][n],
 * hcoef [count][n] (trace / composition coefficients), zpts [count][2] = (z, z g), coeffs
 * [count][8] = 7 trace DEEP coefficients + the composition one; ood_out [count][15] (T_c(z),
 * T_c(zg) interleaved, H(z)), deep_out [count][n] (DEEP composition coefficients).
 * This is xfg_debug_ood_deep_e with ext = 1 and no coin step, and refuses what that entry refuses */
int xfg_debug_ood_deep(xfg_ctx* ctx, uint32_t count, uint64_t n, const uint64_t* coef, const uint64_t* hcoef,
                       const uint64_t* zpts, const uint64_t* coeffs, uint64_t* ood_out, uint64_t* deep_out);
/* the same kernels in the field of extension degree ext (1 or 2), E elements as ext consecutive words:
 * coef [count][7][n] (base field), hcoef [count][ext][n] coordinate planes, zpts [count][2][ext] = (z, z g),
 * ood_out [count][15][ext], deep_out [count][ext][n] coordinate planes.
 * coin_seeds == NULL: coeffs [count][8][ext] = a_0..a_6, gamma; the entry forms the DEEP parameters
 * (1 / z, 1 / (z g), c1, c2) on the host from the frame the device returned, and the frame is reduced by
 * the 64-thread block of a launch without transcript step. ginv and the outputs from dp_out on are unused.
 * coin_seeds != NULL: the launches of the prover. The frame is reduced by the 128-thread block that
 * then runs the DEEP transcript step of instance b on the coin (coin_seeds [count][8] LE u32 words,
 * coin_counters [count]): reseed with the hashes of the frame, draw a_0..a_6 and gamma, and write the DEEP
 * parameters with 1 / (z g) = (1 / z) ginv; the quotient kernels consume what it wrote. coeffs is unused.
 * Out: dp_out [count][28] = a_0..a_6, gamma, z, z g, 1 / z, 1 / (z g), c1, c2 as 14 elements of 2 words
 * (second word 0 when ext = 1); seeds_out [count][8] and counters_out [count], the coins afterwards;
 * fail_out [count], cleared before the launches: 1 where a draw ran out of its tries or z = 0 (1 / z is
 * then returned as 0 and that instance's deep_out is meaningless).
 * Refused with XFG_INVALID_ARGUMENT before anything is allocated or launched: ext other than 1 or 2, n no
 * power of two in [8, 2^21], count 0 or above 65535, a word that is not below p, and without coin step
 * z = 0 or z g = 0. Every device output is set to 0xFF bytes before the launches */
int xfg_debug_ood_deep_e(xfg_ctx* ctx, uint32_t count, uint64_t n, uint32_t ext, const uint64_t* coef,
                         const uint64_t* hcoef, const uint64_t* zpts, const uint64_t* coeffs,
                         const uint32_t* coin_seeds, const uint64_t* coin_counters, uint64_t ginv, uint64_t* ood_out,
                         uint64_t* deep_out, uint64_t* dp_out, uint32_t* seeds_out, uint64_t* counters_out,
                         int* fail_out);
/* xfg_debug_ood_deep_e on trace coefficients behind a column descriptor, as the prover runs the two
 * kernels: flags [count][7] with 1 for a constant column (its polynomial is the constant vals [count][7])
 * and 2 for a column whose coefficients are those of instance 0's same column (never for instance 0
 * itself); such a column's plane of the uploaded coef is set to 0xFF bytes on the device before the
 * launches, so a kernel that still reads it shows. The caller vouches for what the flags say.
 * flags = vals = NULL: xfg_debug_ood_deep_e itself, the dense kernels */
int xfg_debug_ood_deep_const(xfg_ctx* ctx, uint32_t count, uint64_t n, uint32_t ext, const uint64_t* coef,
                             const uint8_t* flags, const uint64_t* vals, const uint64_t* hcoef, const uint64_t* zpts,
                             const uint64_t* coeffs, const uint32_t* coin_seeds, const uint64_t* coin_counters,
                             uint64_t ginv, uint64_t* ood_out, uint64_t* deep_out, uint64_t* dp_out,
                             uint32_t* seeds_out, uint64_t* counters_out, int* fail_out);
/* constraint evaluation kernel of the prover on `count` instances, through the calls prove_lane
 * makes, through the same helper (launch_trace_lde in lane_unit.hip: column interpolation, trace LDE at
 * `blowup` -- 2..128, above 16 with n * blowup <= 2^24; then the host-built divisor table, the kernel):
 * trace [count][7][n] canonical, airs [count], coeffs [count][15][ext] = 7 transition, 7 step-0
 * boundary and the final-step boundary coefficient, E elements (ext 1 or 2 coordinates each);
 * ce [count][ext][2n] coordinate planes in natural CE-domain order (index i <-> x = 7 w_2n^i) */
int xfg_debug_constraint_eval(xfg_ctx* ctx, uint32_t count, uint64_t n, uint32_t blowup, uint32_t ext,
                              const uint64_t* trace, const xfg_air_consts* airs, const uint64_t* coeffs,
                              uint64_t* ce);
/* FRI fold kernel (folding factor 8, domain offset 7) on `count` layers of D = 2^(logn + logbeta)
 * E values: vals [count][ext][D] coordinate planes, natural order, or coset-major (natural index K
 * stored at (K mod beta) n + K / beta, the layout of the first layer) when coset_major != 0;
 * alpha [count][ext] (the entry forms alpha * 7^-1 on the host); out [count][ext][D / 8].
 * All inputs canonical; D >= 16 */
int xfg_debug_fri_fold(xfg_ctx* ctx, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                       const uint64_t* vals, const uint64_t* alpha, uint64_t* out);
/* the same for folding factor fold = 2, 4, 8 or 16: out [count][ext][D / fold], D >= 2 fold
 * (xfg_debug_fri_fold is this entry with fold = 8) */
int xfg_debug_fri_fold_f(xfg_ctx* ctx, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                         uint32_t fold, const uint64_t* vals, const uint64_t* alpha, uint64_t* out);
/* device Fiat-Shamir draws (DefaultRandomCoin<Blake3_256>::draw::<E>) from the coin (seed as 8 LE
 * u32 words, counter): k <= 64 draws of E (ext 1 or 2) by one wave -- the prover's coefficient and
 * DEEP draws -- and one at a time -- its FRI alpha draws. Besides the >= p rule, a candidate whose
 * counter c (1 <= c <= 256) has bit c - 1 of reject[4] set is rejected, to exercise the retries.
 * out_wave / out_seq [k][2] (second coordinate 0 when ext = 1), counters[2] = each coin's counter
 * afterwards, ok[2] = 1 when no draw ran out of its 1000 tries */
int xfg_debug_coin_draws(xfg_ctx* ctx, const uint32_t seed[8], uint64_t counter, uint32_t k, uint32_t ext,
                         const uint64_t reject[4], uint64_t* out_wave, uint64_t* out_seq, uint64_t counters[2],
                         int ok[2]);
/* Merkle commitment of `count` LDEs as the prover runs it (leaf kernel, then the tree up to the root,
 * no transcript step), every stored node copied back. lde [count][nc][blowup][n], coset-major as
 * xfg_debug_lde's device output (row m of coset t at [t][m]); nc = 1, 2 or 7 columns, blowup 2..16 (the
 * prover's instantiations for blowup 32, 64 and 128 are not reachable through this hook),
 * 8 <= n <= 2^24, both powers of two, count <= 65535. nodes_out [count][2n][32 bytes]: each proof's heap (slot 1 = root,
 * slot i = H(slot 2i || slot 2i+1)); slots [1, n) are defined -- the levels below them live in
 * registers only -- and every other slot is returned as 0xFF bytes. local_out [nentries][2 blowup][32]:
 * the local heaps the opening kernel recomputes for rows entries[e] = proof << log2(n) | row (slot 1 =
 * the row's node n + row of the full tree, leaf of coset t at blowup + t; slot 0 is 0xFF bytes) */
int xfg_debug_merkle_lde(xfg_ctx* ctx, uint32_t count, uint32_t nc, uint64_t n, uint32_t blowup, const uint64_t* lde,
                         const uint64_t* entries, uint64_t nentries, uint8_t* nodes_out, uint8_t* local_out);
/* xfg_debug_merkle_lde for an LDE with constant columns, as the prover commits to its trace LDE:
 * flags [count][nc] (non-zero: the column holds vals [count][nc]'s value at every point) go to the leaf
 * and opening kernels, which take a flagged column from them and do not read its plane. The flagged
 * planes of the uploaded lde are set to 0xFF bytes on the device before the launches, so a kernel that
 * still reads one hashes a word that is no field element. nc must be 7; blowup 2..128.
 * flags = vals = NULL: the dense kernels on the lde as uploaded (xfg_debug_merkle_lde with blowup up to 128) */
int xfg_debug_merkle_lde_const(xfg_ctx* ctx, uint32_t count, uint32_t nc, uint64_t n, uint32_t blowup,
                               const uint64_t* lde, const uint8_t* flags, const uint64_t* vals,
                               const uint64_t* entries, uint64_t nentries, uint8_t* nodes_out, uint8_t* local_out);
/* on != 0: from now on every unit sets its whole trace LDE buffer and its trace coefficient buffer to 0xFF
 * bytes before the transforms. The planes of constant columns, and of columns shared with the unit's first
 * proof, are never written, and without this one that a previous unit left there can hold the right value
 * by accident. A unit whose traces the prover generates also sets its trace buffer to 0xFF bytes before the
 * generator runs, which writes the live columns only. Refused while batches are pending */
int xfg_debug_poison_lde(xfg_ctx* ctx, int on);
/* Merkle commitment of `count` FRI layers (leaf i = the 8 E values at natural indices i + k rows,
 * k < 8, rows = D / 8), vals, the layout arguments and their checks as for xfg_debug_fri_fold; count <= 65535.
 * nodes_out [count][2 rows][32 bytes]: the whole heap, slots [1, 2 rows); slot 0 is 0xFF bytes */
int xfg_debug_merkle_fri(xfg_ctx* ctx, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                         const uint64_t* vals, uint8_t* nodes_out);
/* the same for folding factor fold = 2, 4, 8 or 16: leaf i = the fold E values at natural indices
 * i + k rows, k < fold, rows = D / fold, D >= 2 fold (xfg_debug_merkle_fri is this entry with fold = 8) */
int xfg_debug_merkle_fri_f(xfg_ctx* ctx, uint32_t count, uint32_t ext, uint32_t logn, uint32_t logbeta, int coset_major,
                           uint32_t fold, const uint64_t* vals, uint8_t* nodes_out);
/* the prover's proof-of-work search alone: for each of count seeds (8 LE u32 words) the smallest nonce
 * in [first_nonce, max_nonce] whose BLAKE3(seed || nonce_le8) has >= grind trailing zero bits in its
 * first 8 LE bytes; 0 where there is none. chunk_log / blocks = 0 take grind_plan's values, otherwise
 * they force the geometry (chunk_log 6..16, blocks 1..4096); max_nonce 0 = the prover's bound */
int xfg_debug_grind(xfg_ctx* ctx, uint32_t count, const uint32_t* seeds, uint32_t grind, uint64_t first_nonce,
                    uint64_t max_nonce, uint32_t chunk_log, uint32_t blocks, uint64_t* nonces_out);
/* GRIND_DEVICE_MIN, and how many proofs' nonces this context has searched on the device / on the host */
int xfg_grind_probe(const xfg_ctx* ctx, uint32_t* device_min, uint64_t* device_searches, uint64_t* host_searches);
/* the Keccak-256 of the record kernel alone (the permutation spread over the lanes of a wave): `count` single-block
 * messages msgs [count][136] of lens[i] <= 135 bytes each (the bytes past a message's length are ignored),
 * padded as Keccak pads (0x01 .. 0x80, one byte 0x81 at length 135; not SHA-3's 0x06) -> out [count][32].
 * Refused with XFG_INVALID_ARGUMENT: a null pointer, count 0 or above 65535, a length above 135 */
int xfg_debug_keccak256(xfg_ctx* ctx, uint32_t count, const uint8_t* msgs, const uint32_t* lens, uint8_t* out);
/* xfg_verify_batch_gpu (the same body, same rules for pending batches) with what the device decided:
 * flags[i] = the 64-bit word the two verifier kernels set for proof i (bit l < 24: layer l folding,
 * 32 + l: layer l commitment, 61 / 62: constraint / trace commitment, 63: remainder folding), 0 for a
 * proof rejected before it was planned; errs + i * err_stride = the VerifierError text of proof i as
 * xfg_verify reports it ("" when accepted), cut to err_stride - 1 characters */
int xfg_debug_verify_batch_gpu(xfg_ctx* ctx, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                               const xfg_air_consts* airs, const xfg_options* acceptable, int* results,
                               uint64_t* flags, char* errs, size_t err_stride);
/* the same for xfg_verify_batch_gpu_acceptable: the policy in place of the options. flags[i] and errs + i *
 * err_stride belong to proofs[i], wherever the device's per-folding-factor ranges put its queries */
int xfg_debug_verify_batch_gpu_acceptable(xfg_ctx* ctx, uint32_t count, const uint8_t* const* proofs,
                                          const size_t* lens, const xfg_air_consts* airs,
                                          const xfg_acceptable* acceptable, int* results, uint64_t* flags, char* errs,
                                          size_t err_stride);

#ifdef __cplusplus
}
#endif
#endif
