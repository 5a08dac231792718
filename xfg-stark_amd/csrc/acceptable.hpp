// Which proof options a verifier takes: the options and the library's own limits on them (check_options), a
// proof's conjectured security level, the verifiers' policy argument (winterfell::AcceptableOptions) and its
// check, and the order in which a GPU batch of mixed folding factors lays out its queries.
// Pure functions, no HIP and no std containers in the interface (tests/sanitize/acceptable.cpp compiles this
// header with a plain host compiler).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/xfg_stark.h"

namespace xfg {

static inline bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// ------------------------------------------------------------------ options
struct Opts {
    uint64_t q, beta, grind, ext, fold, remdeg;
};
static inline Opts to_opts(const xfg_options* o) {
    return Opts{o->num_queries, o->blowup_factor, o->grinding_factor, o->field_extension, o->fri_folding_factor,
                o->fri_remainder_max_degree};
}
static inline bool same_opts(const Opts& a, const Opts& b) {
    return a.q == b.q && a.beta == b.beta && a.grind == b.grind && a.ext == b.ext && a.fold == b.fold &&
           a.remdeg == b.remdeg;
}
// blowup 32, 64, 128 (LDEs composed of blowup-16 transforms): n * beta is limited to the largest LDE proven
// at blowup 16, 2^20 x 16
constexpr uint64_t WIDE_LDE_MAX = 1ULL << 24;
static inline bool wide_lde_too_large(uint64_t n, uint64_t beta) { return beta > 16 && n > WIDE_LDE_MAX / beta; }
// check_options' answer to that rule (check_request names the sizes when it is this one that failed)
constexpr const char* WIDE_LDE_REFUSAL = "blowup factors above 16 need an LDE domain of at most 2^24 points";
// ProofOptions::new validation (winter-air 0.8) + what this GPU path implements
static inline const char* check_options(uint64_t n, const Opts& o) {
    if (!is_pow2(n) || n < 8) return "trace length must be a power of two and at least 8";
    if (n > (1ULL << 21)) return "trace length above 2^21 is not supported";
    if (!is_pow2(o.beta) || o.beta < 2 || o.beta > 128) return "blowup factor must be a power of two in [2, 128]";
    if (o.q < 1 || o.q > 255) return "number of queries must be in [1, 255]";
    if (o.grind > 32) return "grinding factor cannot be greater than 32";
    if (o.ext != 1 && o.ext != 2) return "field extension must be None (1) or Quadratic (2)";
    if (o.fold != 2 && o.fold != 4 && o.fold != 8 && o.fold != 16) return "FRI folding factor must be 2, 4, 8 or 16";
    if (o.remdeg > 255 || !is_pow2(o.remdeg + 1)) return "FRI remainder max degree must be one less than a power of two";
    if (o.q >= n * o.beta) return "number of queries must be smaller than the LDE domain size";
    if (wide_lde_too_large(n, o.beta)) return WIDE_LDE_REFUSAL;
    return nullptr;
}

// ------------------------------------------------------------------ security level
// RECALLED: winter-air 0.8 get_conjectured_security (src/proof/mod.rs of that crate, not vendored in the
// reference), which StarkProof::security_level(conjectured = true) returns, for this field (64 bits per
// extension degree) and hash (Blake3_256: 128 bits of collision resistance):
//   field_security = 64 ext - log2(n blowup)
//   query_security = log2(blowup) num_queries, plus grinding_factor when that product is at least 80
//                    (GRINDING_CONTRIBUTION_FLOOR)
//   level          = min(min(field_security, query_security) - 1, 128)
// The policy check runs on a proof's options before check_options has seen them, so every value a parsed
// header can hold (one byte per option, logn <= 32, ext 1..3) gives a defined result: the logarithms round
// down, log2(0) counts as 0, and a difference that would go below 0 is 0.
constexpr uint32_t GRINDING_CONTRIBUTION_FLOOR = 80, HASH_COLLISION_RESISTANCE = 128;
static inline uint32_t floor_log2(uint64_t x) { return x ? 63u - (uint32_t)__builtin_clzll(x) : 0u; }
static inline uint32_t conjectured_security(uint64_t n, const Opts& o) {
    const uint64_t field_bits = 64 * o.ext, lde_bits = (uint64_t)floor_log2(n) + floor_log2(o.beta);
    const uint64_t field_security = field_bits > lde_bits ? field_bits - lde_bits : 0;
    uint64_t query_security = (uint64_t)floor_log2(o.beta) * o.q;
    if (query_security >= GRINDING_CONTRIBUTION_FLOOR) query_security += o.grind;
    const uint64_t m = field_security < query_security ? field_security : query_security;
    const uint64_t level = m ? m - 1 : 0;
    return (uint32_t)(level < HASH_COLLISION_RESISTANCE ? level : HASH_COLLISION_RESISTANCE);
}

// ------------------------------------------------------------------ the policy
// winterfell::AcceptableOptions as the verifiers hold it: xfg_acceptable with its option sets copied
constexpr uint32_t ACCEPT_MAX_OPTIONS = 32;
struct Acceptable {
    uint32_t kind = XFG_ACCEPT_OPTION_SET, min_security = 0, count = 0;
    Opts set[ACCEPT_MAX_OPTIONS];
};
// the one-element set the entries without a policy argument stand for
static inline Acceptable acceptable_one(const Opts& o) {
    Acceptable a;
    a.count = 1;
    a.set[0] = o;
    return a;
}
// false for what the entries refuse with XFG_INVALID_ARGUMENT: a null policy, an unknown kind (2, reserved for
// MinProvenSecurity, included), a set without options or with 0 or more than 32 of them
static inline bool make_acceptable(const xfg_acceptable* p, Acceptable& a) {
    if (!p) return false;
    a = Acceptable{};
    a.kind = p->kind;
    if (p->kind == XFG_ACCEPT_MIN_CONJECTURED_SECURITY) {
        a.min_security = p->min_security;
        return true;
    }
    if (p->kind != XFG_ACCEPT_OPTION_SET || !p->options || p->num_options < 1 || p->num_options > ACCEPT_MAX_OPTIONS)
        return false;
    a.count = p->num_options;
    for (uint32_t i = 0; i < a.count; i++) a.set[i] = to_opts(p->options + i);
    return true;
}
// AcceptableOptions::validate on a proof of trace length n with options o: "" when the policy takes it, else
// the VerifierError in Debug form (a literal, or text written into buf)
constexpr size_t POLICY_ERROR_LEN = 64;
static inline const char* policy_error(const Acceptable& a, uint64_t n, const Opts& o, char buf[POLICY_ERROR_LEN]) {
    if (a.kind == XFG_ACCEPT_MIN_CONJECTURED_SECURITY) {
        const uint32_t level = conjectured_security(n, o);
        if (level >= a.min_security) return "";
        snprintf(buf, POLICY_ERROR_LEN, "InsufficientConjecturedSecurity(%u, %u)", a.min_security, level);
        return buf;
    }
    for (uint32_t i = 0; i < a.count; i++)
        if (same_opts(a.set[i], o)) return "";
    return "UnacceptableProofOptions";
}

// ------------------------------------------------------------------ a GPU batch's queries by folding factor
// vfield_kernel<LOGF> is one instantiation per folding factor, so the batch's query records lie in four
// contiguous ranges, LOGF = 1..4 in this order: range r is [begin[r], begin[r + 1]), begin[0] = 0, begin[4] =
// the number of records; any of them may be empty.
struct FoldRanges {
    uint64_t begin[5];
};
// item i has nq[i] records and folding factor 2^logf[i]; logf[i] = 0 (or nq[i] = 0): the item is not planned
// and has none. first[i] = where item i's records start: within a range the items keep their input order.
// A logf above 4 is refused (false), nothing written
static inline bool bucket_queries(uint32_t count, const uint32_t* nq, const uint8_t* logf, uint64_t* first,
                                  FoldRanges& R) {
    uint64_t size[5] = {0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < count; i++) {
        if (logf[i] > 4) return false;
        size[logf[i]] += logf[i] ? nq[i] : 0;
    }
    R.begin[0] = 0;
    for (int r = 0; r < 4; r++) R.begin[r + 1] = R.begin[r] + size[r + 1];
    uint64_t next[5] = {0, R.begin[0], R.begin[1], R.begin[2], R.begin[3]};
    for (uint32_t i = 0; i < count; i++) {
        first[i] = next[logf[i]];
        next[logf[i]] += logf[i] ? nq[i] : 0;
    }
    return true;
}

}  // namespace xfg
