// CPU driver for the prover's host-only proof assembly (xfg-stark_amd/csrc/proof_assembly.hpp):
// plan_queries -> concat_indices -> serialize_proof for B proofs over synthetic memory, built
// host-only with AddressSanitizer + UndefinedBehaviorSanitizer (xfg-stark_amd/Makefile target
// `sanitize`; run by tests/test_sanitize.py on the CPU). The transcript replay is not under test.
//
// Synthetic memory: the value gathered from source s (0 trace LDE, 1 composition LDE, 2 + l FRI
// layer l) at index i is (s << 56) | i; a stored digest carries (source, index) in its words; the
// recomputed-subtree digest at slot e * 2 beta + local carries (tree, proof, row, local) of entry e
// of the concatenated entry list. The gathers are done here from the index buffer exactly where
// launch_gather_set and launch_open_rows place their output, in buffers of exactly the planned
// sizes. The emitted bytes are parsed back (parse_proof / parse_contents, the parser behind
// xfg_proof_parse) and every opened value and digest is decoded and checked against the position it
// must come from; the expected digest set of a batch opening is derived here by marking ancestors.
// Exit status 0 = all as expected.
//
// usage: assemble_proof n beta q ext B remdeg
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "../../xfg-stark_amd/csrc/proof_assembly.hpp"
#include "../../xfg-stark_amd/csrc/verifier.hpp"

using namespace xfg;

#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            fprintf(stderr, "FAILED %s: ", #cond); \
            fprintf(stderr, __VA_ARGS__);       \
            fprintf(stderr, "\n");              \
            return false;                       \
        }                                       \
    } while (0)

enum { STORED = 1, RECOMPUTED = 2 };
static Digest stored_digest(u64 source, u64 index) {
    Digest d{};
    d.w[0] = STORED;
    d.w[1] = (uint32_t)source;
    d.w[2] = (uint32_t)index;
    d.w[3] = (uint32_t)(index >> 32);
    return d;
}
static Digest recomputed_digest(u64 tree, u64 proof, u64 row, u64 local) {
    Digest d{};
    d.w[0] = RECOMPUTED;
    d.w[1] = (uint32_t)tree;
    d.w[2] = (uint32_t)proof;
    d.w[3] = (uint32_t)row;
    d.w[4] = (uint32_t)local;
    return d;
}
static u64 value_of(u64 source, u64 index) { return (source << 56) | index; }

// siblings of path nodes that are not themselves on a path, levels 1 .. depth, of an L-leaf tree
// (heap indices, leaf i = L + i)
static std::vector<u64> expected_siblings(const std::vector<u64>& leaves, u64 L) {
    std::set<u64> on;
    for (u64 p : leaves)
        for (u64 h = L + p; h >= 1; h >>= 1) on.insert(h);
    std::vector<u64> out;
    for (u64 h : on)
        if (h >= 2 && !on.count(h ^ 1)) out.push_back(h ^ 1);
    std::sort(out.begin(), out.end());
    return out;
}

struct Shape {
    int B;
    Opts o;
    ProofShape sh;
};

// heap indices of the digests of one serialised opening, each decoded by `decode` (false: malformed)
template <class F>
static bool opened_nodes(const Paths& paths, F decode, std::vector<u64>& out) {
    out.clear();
    for (size_t i = 0; i < paths.ptr.size(); i++)
        for (uint32_t k = 0; k < paths.cnt[i]; k++) {
            Digest d;
            memcpy(d.w, paths.ptr[i] + 32 * k, 32);
            u64 h = 0;
            if (!decode(d, h)) return false;
            out.push_back(h);
        }
    std::sort(out.begin(), out.end());
    return true;
}

static bool check_proof(const Shape& S, int b, const ProofJob& j) {
    const ProofShape& sh = S.sh;
    const u64 n = sh.n, beta = sh.beta, N = sh.N;
    const int DE = sh.DE, logbeta = sh.logbeta;
    ParsedProof pf;
    std::string e = parse_proof(j.bytes.data(), j.bytes.size(), pf);
    CHECK(e.empty(), "proof %d: %s", b, e.c_str());
    e = parse_contents(pf);
    CHECK(e.empty(), "proof %d: %s", b, e.c_str());
    CHECK(j.bytes.size() <= proof_size_bound(sh, S.o), "proof %d: %zu bytes", b, j.bytes.size());
    const std::vector<u64>& pos = j.pos;
    CHECK(std::is_sorted(pos.begin(), pos.end()) && std::adjacent_find(pos.begin(), pos.end()) == pos.end(),
          "proof %d", b);
    CHECK(pf.num_unique == pos.size() && pf.logn == (u64)sh.logn && pf.fri_vals.size() == sh.nl, "proof %d", b);
    CHECK(pf.nonce == j.nonce && pf.fri_rem.n == sh.rem_len * 8 * DE, "proof %d", b);
    // trace and constraint values
    CHECK(pf.trace_rows.n == pos.size() * 7 * 8 && pf.constraint_rows.n == pos.size() * DE * 8, "proof %d", b);
    for (size_t i = 0; i < pos.size(); i++) {
        const u64 k = pos[i], t = k & (beta - 1), m = k >> logbeta;
        for (int c = 0; c < 7; c++)
            CHECK(pf.trace_rows.elem(i * 7 + c) == value_of(0, (((u64)b * 7 + c) * beta + t) * n + m),
                  "proof %d position %zu column %d", b, i, c);
        for (int c = 0; c < DE; c++)
            CHECK(pf.constraint_rows.elem(i * DE + c) == value_of(1, (((u64)b * DE + c) * beta + t) * n + m),
                  "proof %d position %zu coordinate %d", b, i, c);
    }
    // trace / constraint tree openings
    const std::vector<u64> want = expected_siblings(pos, N);
    std::vector<u64> got;
    for (int tree = 0; tree < 2; tree++) {
        auto decode = [&](const Digest& d, u64& h) {
            if (d.w[0] == STORED) {
                const u64 idx = (u64)d.w[2] | ((u64)d.w[3] << 32);
                h = idx - (u64)b * 2 * n;
                return d.w[1] == (uint32_t)tree && idx >= (u64)b * 2 * n && h < n;
            }
            if (d.w[0] != RECOMPUTED || d.w[1] != (uint32_t)tree || d.w[2] != (uint32_t)b) return false;
            const u64 m = d.w[3], local = d.w[4];
            if (m >= n || local < 1 || local >= 2 * beta) return false;
            const unsigned dep = 63 - (unsigned)__builtin_clzll(local);
            h = ((n + m) << dep) + (local - (1ULL << dep));
            return true;
        };
        CHECK(opened_nodes(tree ? pf.constraint_paths : pf.trace_paths, decode, got), "proof %d tree %d", b, tree);
        CHECK(got == want, "proof %d tree %d: %zu digests, %zu expected", b, tree, got.size(), want.size());
    }
    // FRI layers
    std::vector<u64> fp = pos;
    for (unsigned l = 0; l < sh.nl; l++) {
        const u64 rows = sh.D[l] / 8;
        std::vector<u64> folded;  // p mod rows, in order of first appearance
        for (u64 p : fp)
            if (std::find(folded.begin(), folded.end(), p % rows) == folded.end()) folded.push_back(p % rows);
        fp = folded;
        CHECK(pf.fri_vals[l].n == fp.size() * 8 * DE * 8, "proof %d layer %u", b, l);
        for (size_t i = 0; i < fp.size(); i++)
            for (u64 k = 0; k < 8; k++)
                for (int c = 0; c < DE; c++) {
                    const u64 K = fp[i] + k * rows;
                    const u64 idx = l == 0 ? (((u64)b * DE + c) * beta + (K & (beta - 1))) * n + (K >> logbeta)
                                           : ((u64)b * DE + c) * sh.D[l] + K;
                    CHECK(pf.fri_vals[l].elem((i * 8 + k) * DE + c) == value_of(2 + l, idx),
                          "proof %d layer %u position %zu", b, l, i);
                }
        auto decode = [&](const Digest& d, u64& h) {
            const u64 idx = (u64)d.w[2] | ((u64)d.w[3] << 32);
            h = idx - (u64)b * 2 * rows;
            return d.w[0] == STORED && d.w[1] == 2 + l && idx >= (u64)b * 2 * rows && h < 2 * rows;
        };
        CHECK(opened_nodes(pf.fri_paths[l], decode, got), "proof %d layer %u", b, l);
        CHECK(got == expected_siblings(fp, rows), "proof %d layer %u: %zu digests", b, l, got.size());
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: %s n beta q ext B remdeg\n", argv[0]);
        return 2;
    }
    const u64 n = strtoull(argv[1], nullptr, 10);
    const Opts o{(u64)atoi(argv[3]), (u64)atoi(argv[2]), 4, (u64)atoi(argv[4]), 8, (u64)atoi(argv[6])};
    const int B = atoi(argv[5]);
    if (const char* m = check_options(n, o)) {
        fprintf(stderr, "bad options: %s\n", m);
        return 2;
    }
    if (B < 1) return 2;
    const Shape S{B, o, ProofShape(n, o)};
    const ProofShape& sh = S.sh;
    const int DE = sh.DE;

    // the replay's outputs plan_queries reads: a non-zero DEEP coefficient n - 2, canonical remainders
    std::vector<u64> dn2((size_t)B * DE, 1), rem((size_t)B * DE * sh.rem_len);
    for (size_t i = 0; i < rem.size(); i++) rem[i] = (0x9E3779B97F4A7C15ULL * (i + 1)) % P;
    ReplayView rv{};
    rv.dn2h = dn2.data();
    rv.remh = rem.data();

    std::vector<ProofJob> jobs(B);
    for (int b = 0; b < B; b++) {  // coins seeded from distinct fixed public inputs, as a unit's are
        ProofJob& j = jobs[b];
        memset(&j.air, 0, sizeof j.air);
        for (int k = 0; k < 12; k++) j.air.pub[k] = 1000 * (u64)(b + 1) + k;
        u64 e[20];
        context_elements(n, o, e);
        memcpy(e + 8, j.air.pub, 12 * 8);
        j.coin.init(e, 20);
        j.commitments.assign(32 * (2 + sh.nl), (uint8_t)(b + 1));  // trace, composition and layer roots
        for (int k = 0; k < 15 * DE; k++) j.ood[k] = 77 + k;
    }

    std::vector<LaneLayout> lay(B);
    for (int b = 0; b < B; b++) plan_queries(jobs[b], b, sh, o, rv, lay[b]);
    OpeningIndex ix;
    concat_indices(lay, B, sh, ix);

    // the gathers, from the index buffer alone
    const size_t nopen = ix.nent * 2 * sh.beta;
    if (ix.allidx.size() != ix.nvals + ix.ndig + ix.nent || ix.vseg.size() != 2 + sh.nl ||
        ix.dseg.size() != 2 + sh.nl) {
        fprintf(stderr, "index buffer lay-out inconsistent\n");
        return 1;
    }
    std::vector<u64> gv(ix.nvals);
    std::vector<Digest> gd(ix.ndig + 2 * nopen);
    size_t vo = 0, dof = 0;
    for (size_t k = 0; k < ix.vseg.size(); k++)
        for (size_t i = 0; i < ix.vseg[k].second; i++) gv[vo++] = value_of(k, ix.allidx[ix.vseg[k].first + i]);
    for (size_t k = 0; k < ix.dseg.size(); k++)
        for (size_t i = 0; i < ix.dseg[k].second; i++) gd[dof++] = stored_digest(k, ix.allidx[ix.dseg[k].first + i]);
    if (vo != ix.nvals || dof != ix.ndig) {
        fprintf(stderr, "segments do not cover the value / digest buffers\n");
        return 1;
    }
    const u64* ent = ix.allidx.data() + ix.nvals + ix.ndig;
    for (int tree = 0; tree < 2; tree++)
        for (size_t e = 0; e < ix.nent; e++)
            for (u64 local = 0; local < 2 * sh.beta; local++)
                gd[ix.ndig + tree * nopen + e * 2 * sh.beta + local] =
                    recomputed_digest(tree, ent[e] >> sh.logn, ent[e] & (n - 1), local);

    size_t total = 0;
    for (int b = 0; b < B; b++) {
        serialize_proof(jobs[b], b, B, sh, o, lay[b], ix, gv.data(), gd.data());
        if (jobs[b].status != XFG_OK) {
            fprintf(stderr, "proof %d: status %d\n", b, jobs[b].status);
            return 1;
        }
        if (!check_proof(S, b, jobs[b])) return 1;
        total += jobs[b].bytes.size();
    }
    printf("assembled %d proofs, %zu bytes, %zu values, %zu digests, %zu subtree entries: ok\n", B, total, ix.nvals,
           ix.ndig, ix.nent);
    return 0;
}
