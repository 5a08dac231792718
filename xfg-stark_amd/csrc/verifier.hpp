// Proof parsing and verification state shared by the host verifier (verifier.cpp) and the batched
// GPU verifier (verify_kernels.hip + xfg_verify_batch_gpu in verify_batch_gpu.hip).
#pragma once
#include <string>
#include <vector>

#include "host_common.hpp"
#include "kernels.hpp"
#include "verify_checks.hpp"

namespace xfg {

struct Span {  // bytes inside the proof
    const uint8_t* p = nullptr;
    size_t n = 0;
    u64 elem(size_t i) const {
        u64 v;
        memcpy(&v, p + 8 * i, 8);
        return v;
    }
};
// BatchMerkleProof::serialize_nodes: u8 vector count, then per vector u8 count + digests (kept as
// pointers into the proof bytes)
struct Paths {
    std::vector<const uint8_t*> ptr;
    std::vector<uint32_t> cnt;
};

// StarkProof fields in wire order (DESIGN.md "Proof format")
struct ParsedProof {
    const uint8_t* base = nullptr;  // the proof bytes every Span / Paths pointer points into
    u64 width = 0, aux = 0, logn = 0;
    Opts o{};
    u64 num_unique = 0;
    std::vector<Digest> com;  // trace root, constraint root, FRI layer roots, remainder commitment
    const uint8_t* com_p = nullptr;  // the commitments' bytes in the proof
    Span trace_rows, constraint_rows, ood, hz, fri_rem;
    Span trace_paths_raw, constraint_paths_raw, ood_raw;  // byte vectors as StarkProof::read_from keeps them
    std::vector<Span> fri_vals, fri_paths_raw;
    // filled by parse_contents
    Paths trace_paths, constraint_paths;
    std::vector<Paths> fri_paths;
    u64 partitions = 0, nonce = 0;
    size_t size = 0;
};
// StarkProof::from_bytes, structural: "" on success, else the ProofDeserializationError text
std::string parse_proof(const uint8_t* bytes, size_t len, ParsedProof& pf);
// the sections' contents (VerifierChannel::new, after the options check)
std::string parse_contents(ParsedProof& pf);

// everything the query checks need, after the transcript has been replayed
struct VState {
    ParsedProof pf;
    int de = 1;  // extension degree of E
    u64 N = 0, beta = 0;
    unsigned nl = 0;       // FRI layers of the options (<= VMAXL)
    std::vector<u64> pos;  // unique query positions (sorted)
    VFieldProof f{};       // z, zg, hz, gam, dc, ood, falpha, de, logN; the rest is plan_proof's
};
// parse, the caller's policy (acceptable.hpp policy_error), the library's own option limits, transcript replay,
// OOD consistency, proof of work, query positions: "" when the proof may proceed to the query checks, else the
// VerifierError. Everything behind the policy check reads the proof's own options (st.pf.o)
std::string verify_transcript(const uint8_t* bytes, size_t len, const AirConst& air, const Acceptable& acceptable,
                              VState& st);

AirConst air_of(const xfg_air_consts* a);

// ---- the query checks: one plan per proof, two executors. plan_proof lists the proof's 2 + nl batch
// Merkle openings and its queries as records of blob offsets (verify_checks.hpp). The batched GPU
// verifier uploads many proofs' records and runs vtree_kernel (one workgroup per opening: leaf hashes,
// BatchMerkleProof::get_root level by level, root comparison) and vfield_kernel<LOGF> (one thread per
// query: query_bits). A batch may mix folding factors: its query records lie in four contiguous ranges, one
// per factor 2, 4, 8, 16 (acceptable.hpp bucket_queries), and launch_verify launches one instantiation per
// non-empty range; the tree records are per-tree generic and stay in input order. The host verifier walks
// the same records serially over the proof's own bytes (verify_queries_host), with the instantiation of the
// proof's own factor. Both hand their flag word to finish_proof.
// one proof's part of a batch (blob offsets already global; tree / vector / proof indices local)
struct VerifyPlan {
    std::vector<VTree> trees;
    std::vector<VTreeLeaf> tleaves;
    std::vector<VVec> vecs;
    VFieldProof fproof{};
    std::vector<VFieldQuery> fqueries;
    // where the FRI structure first breaks: layer l's value section has the wrong size (l < nl), the
    // remainder has the wrong length (nl), nowhere (-1). Only what comes before the break is planned:
    // the trace and constraint openings, the layers below l (fproof.nl), the remainder if nothing broke
    int broken = -1;
};
// plan one proof whose transcript replayed fine, its bytes at blob offset blob_off. The two executors
// treat a break differently: the host runs what was planned and reports the break at its place in the
// check order (after every opening and fold that comes before it); the GPU verifier does not send a
// broken proof to the device and reports the break first, with flag word 0
void plan_proof(const VState& st, size_t blob_off, VerifyPlan& plan);
// flag bits (of what was planned) and the recorded break to the VerifierError: the first failing check
// in the order trace opening, constraint opening, per layer (section size, opening, fold), remainder
// length, remainder commitment (checked here), remainder evaluation; "" if none
std::string finish_proof(const VState& st, int broken, u64 flags);
// the query checks on the host: plan_proof over the proof's own bytes, every opening, every query
std::string verify_queries_host(const VState& st);

// fq: the batch's query records, range r = [ranges.begin[r], ranges.begin[r + 1]) those of folding factor 2^(r + 1);
// an empty range launches nothing (nor do zero trees)
void launch_verify(const uint8_t* blob, const VTree* trees, u64 ntrees, const VTreeLeaf* tleaves, const VVec* vecs,
                   const VFieldProof* fp, const VFieldQuery* fq, const FoldRanges& ranges, u64* flags, hipStream_t s);

}  // namespace xfg
