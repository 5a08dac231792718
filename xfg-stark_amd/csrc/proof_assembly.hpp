// The host half of one proof unit, free of any HIP runtime call (compiles host-only, like
// verifier.cpp): the shape of a proof, the transcript replay, the query / opening plans, the lay-out
// of the gather indices and the serialiser (StarkProof::to_bytes). lane_unit.hip runs these between its
// launch sets; tests/sanitize/assemble_proof.cpp runs them on the CPU over synthetic memory.
#pragma once
#include <stdexcept>
#include <utility>
#include <vector>

#include "host_common.hpp"
#include "kernels.hpp"

namespace xfg {

// everything (n, options) fix about a proof's sizes: LDE domain, FRI layer domains D[0..nl]
// (D[0] = N), remainder length D[nl] / blowup
struct ProofShape {
    u64 n, beta, N, rem_len;
    int logn, logbeta;
    int DE;  // extension degree: E-valued data is DE coordinate planes
    unsigned nl;
    std::vector<u64> D;
    ProofShape(u64 n_, const Opts& o)
        : n(n_), beta(o.beta), N(n_ * o.beta), logn((int)ilog2(n_)), logbeta((int)ilog2(o.beta)), DE((int)o.ext),
          nl(num_fri_layers(n_ * o.beta, o)), D(nl + 1) {
        D[0] = N;
        for (unsigned l = 1; l <= nl; l++) D[l] = D[l - 1] / o.fold;
        rem_len = D[nl] >> logbeta;
    }
};

struct ProofJob {
    AirConst air;
    Coin coin;
    std::vector<uint8_t> commitments;
    u64 ood[30];           // 15 E elements ([T_c(z), T_c(zg)] x 7, H(z)), DE coordinates each
    std::vector<u64> rem;  // FRI remainder, E elements
    u64 nonce = 0;
    std::vector<u64> pos;
    std::vector<uint8_t> bytes;
    int status = XFG_OK;
    bool pow_exhausted = false;  // status XFG_PROVER_ERROR because the bounded device search found no nonce
};

// ------------------------------------------------------------------ byte writer
struct BW {
    std::vector<uint8_t>& b;  // caller-owned scratch, reused across proofs (never shrunk)
    size_t o = 0;
    explicit BW(std::vector<uint8_t>& buf) : b(buf) {}
    void reserve(size_t k) {
        if (b.size() < k) b.resize(k);
    }
    uint8_t* at(size_t k) {  // k bytes at the cursor (grows geometrically; callers pre-size)
        if (o + k > b.size()) b.resize(std::max(2 * b.size(), o + k));
        uint8_t* q = b.data() + o;
        o += k;
        return q;
    }
    void put(const void* p, size_t k) { memcpy(at(k), p, k); }
    void u8(u64 v) { *at(1) = (uint8_t)v; }
    void u16(u64 v) { uint16_t x = (uint16_t)v; put(&x, 2); }  // little-endian host
    void u32(u64 v) { uint32_t x = (uint32_t)v; put(&x, 4); }
    void u64_(u64 v) { put(&v, 8); }
    void u64s(const u64* v, size_t k) { put(v, 8 * k); }
    size_t len_slot() { at(4); return o; }          // u32 byte length of what follows
    void len_patch(size_t end_of_slot) {
        uint32_t x = (uint32_t)(o - end_of_slot);
        memcpy(b.data() + end_of_slot - 4, &x, 4);
    }
    void trim() { b.resize(o); }  // the buffer is the output (the proof's own bytes)
};

// one proof's opening plan (plan_queries): the batch openings of the LDE trees and the FRI
// layers, and its gather indices per source (values: trace LDE, composition LDE, FRI layers;
// digests: trace / composition tree nodes, FRI layer nodes) and recomputed-subtree rows
struct LaneLayout {
    BatchOpening op;                     // trace / constraint trees (same positions)
    std::vector<int64_t> ref;            // per node: >= 0 stored ordinal, < 0 -(open slot + 1), slots from this proof's first
    std::vector<BatchOpening> fops;      // FRI layers
    std::vector<std::vector<u64>> fpos;
    std::vector<u64> vlde, vh, dt, dh, oent;
    std::vector<std::vector<u64>> vf, df;
};

// the replay's inputs as the chain's last kernel packed them (host pointers into the pinned block)
struct ReplayView {
    const Digest* roots;    // [trace, composition, FRI 0..nl-1][B]
    const u64* ood;         // [B][15][DE]
    const u64* co;          // composition coefficients [B][15][DE]
    const DeepParams* dps;  // [B]
    const u64* falpha;      // [layer][B][DE]
    const int* ffail;       // [B]
    const u64* remh;        // remainder planes [B][DE][rem_len]
    const u64* dn2h;        // DEEP coefficient n - 2, [B][DE]
};

// one index buffer for a unit's gathers: a segment per source (values: trace LDE, composition LDE,
// FRI layers; then as many digest segments), the proofs' lists end to end inside each segment, then
// the recomputed-subtree entries. vcur / dcur[k * B + b]: where proof b's values / digests of
// segment k start in the gathered values / digests; ent0[b]: proof b's first entry
struct OpeningIndex {
    std::vector<u64> allidx;
    std::vector<std::pair<size_t, size_t>> vseg, dseg;  // (offset, count)
    std::vector<size_t> vcur, dcur;
    std::vector<int64_t> ent0;
    size_t nvals = 0, ndig = 0, nent = 0;
};

// host replay of the transcript: commitments into the proof and the coin advanced exactly as the
// device coin was; the device's coefficient, z and DEEP draws (and its rejections) must agree.
// g: the trace domain generator
static inline void replay_transcript(ProofJob& j, int b, int B, const ProofShape& sh, u64 g, const ReplayView& rv) {
    const int DE = sh.DE;
    bool failed = false, same = true;
    auto commit = [&](const Digest& r) {
        uint8_t rb[32];
        digest_bytes(r, rb);
        j.commitments.insert(j.commitments.end(), rb, rb + 32);
        j.coin.reseed(r);
    };
    auto draw = [&](const u64* dev) {  // dev: the device's value (DE coordinates) or null
        u64 a[2] = {0, 0};
        if (!j.coin.draw_e(a, DE)) failed = true;
        for (int d = 0; dev && d < DE; d++) same &= a[d] == dev[d];
        return a[0] | a[1];
    };
    const DeepParams& dp = rv.dps[b];
    const Digest* froots = rv.roots + 2 * B;
    commit(rv.roots[b]);
    for (int k = 0; k < 15; k++) draw(rv.co + ((size_t)b * 15 + k) * DE);  // composition coefficients
    commit(rv.roots[B + b]);
    if (draw(dp.z) == 0) failed = true;  // z = 0: no DEEP quotient
    memcpy(j.ood, &rv.ood[(size_t)b * 15 * DE], 15 * DE * 8);  // [15][DE]
    j.coin.reseed(hash_elements(j.ood, 14 * DE));  // interleaved T_i(z), T_i(zg), E elements
    j.coin.reseed(hash_elements(j.ood + 14 * DE, DE));
    for (int k = 0; k < 7; k++) draw(dp.a[k]);
    draw(dp.gamma);
    for (unsigned l = 0; l < sh.nl; l++) {
        commit(froots[(size_t)l * B + b]);
        draw(rv.falpha + ((size_t)l * B + b) * DE);  // FRI alpha (the fold used alpha * 7^-1 of it)
    }
    // the DEEP parameters the device derived from z and the frame: z g, 1 / z, 1 / (z g), and the
    // OOD sums c1 = gamma H(z) + sum a_k T_k(z), c2 = sum a_k T_k(z g)
    if (!failed) {
        auto e = [&](const u64* v) { return E2{v[0], DE == 2 ? v[1] : 0}; };
        auto ood_e = [&](int q) { return E2{j.ood[q * DE], DE == 2 ? j.ood[q * DE + 1] : 0}; };
        const E2 z = e(dp.z), zg = e(dp.zg), one = e2(1);
        E2 c1 = e2_mul(e(dp.gamma), ood_e(14)), c2{0, 0};
        for (int k = 0; k < 7; k++) {
            c1 = e2_add(c1, e2_mul(e(dp.a[k]), ood_e(2 * k)));
            c2 = e2_add(c2, e2_mul(e(dp.a[k]), ood_e(2 * k + 1)));
        }
        same &= e2_eq(zg, e2_mulb(z, g)) && e2_eq(e2_mul(z, e(dp.zinv)), one) &&
                e2_eq(e2_mul(zg, e(dp.zginv)), one) && e2_eq(c1, e(dp.c1)) && e2_eq(c2, e(dp.c2));
    }
    if (failed) j.status = XFG_PROVER_ERROR;
    if (failed != (rv.ffail[b] != 0) || !same) throw std::runtime_error("device / host transcript diverged");
}

// plan_queries in three steps, so that the prover can put the device's proof-of-work search
// (grind.hip, from GRIND_DEVICE_MIN on) in the place of the host's:
// (a) plan_commit_remainder: degree check, remainder commitment, reseed -- j.coin.seed is then the seed
//     the nonce is searched for
static inline void plan_commit_remainder(ProofJob& j, int b, const ProofShape& sh, const ReplayView& rv, LaneLayout& L) {
    const u64 rem_len = sh.rem_len;
    const int DE = sh.DE;
    const unsigned nl = sh.nl;
    L.ref.clear();
    L.fops.clear();
    L.fpos.clear();
    for (auto* v : {&L.vlde, &L.vh, &L.dt, &L.dh, &L.oent}) v->clear();
    L.vf.resize(nl);
    L.df.resize(nl);
    if (rv.dn2h[(size_t)b * DE] == 0 && rv.dn2h[(size_t)b * DE + DE - 1] == 0)
        j.status = XFG_PROVER_ERROR;  // assert_eq!(trace_length - 2, degree)
    j.rem.resize(rem_len * DE);  // E elements, coordinates interleaved
    for (u64 i = 0; i < rem_len; i++)
        for (int k = 0; k < DE; k++) j.rem[i * DE + k] = rv.remh[((size_t)b * DE + k) * rem_len + i];
    Digest rc = hash_elements(j.rem.data(), rem_len * DE);
    uint8_t rb[32];
    digest_bytes(rc, rb);
    j.commitments.insert(j.commitments.end(), rb, rb + 32);
    j.coin.reseed(rc);
}
// trailing zero bits of the first 8 LE bytes of BLAKE3(seed || nonce_le8): a nonce passes with >= grind
static inline unsigned pow_zeros(const Digest& seed, u64 nonce) {
    const Digest h = merge_with_int(seed, nonce);
    return tz64((u64)h.w[0] | ((u64)h.w[1] << 32));
}
// the host's search: the smallest nonce >= 1 that passes, one hash at a time
static inline u64 host_grind(const Digest& seed, u64 grind) {
    u64 nonce = 1;
    while (pow_zeros(seed, nonce) < grind) nonce++;
    return nonce;
}
// (b) plan_openings: the nonce into the transcript, query positions, and proof b's gather lists:
// LDE trees store heap levels >= log2(beta) (indices < 2n); lower nodes of an opened row are
// recomputed by launch_open_rows (local heap: 2 * beta slots per row)
static inline void plan_openings(ProofJob& j, int b, const ProofShape& sh, const Opts& o, u64 nonce, LaneLayout& L) {
    const u64 n = sh.n, beta = sh.beta, N = sh.N;
    const int DE = sh.DE, logn = sh.logn, logbeta = sh.logbeta;
    const unsigned nl = sh.nl;
    const u64 stored_lim = n, LB = beta;  // stored: heap levels >= log2(beta) + 1
    j.nonce = nonce;
    j.coin.reseed_int(nonce);
    std::vector<u64> pos(o.q);
    for (u64 i = 0; i < o.q; i++) {
        Digest h = j.coin.next();
        pos[i] = ((u64)h.w[0] | ((u64)h.w[1] << 32)) & (N - 1);
    }
    std::sort(pos.begin(), pos.end());
    pos.erase(std::unique(pos.begin(), pos.end()), pos.end());
    j.pos = pos;
    for (u64 k : pos) {
        u64 t = k & (beta - 1), m = k >> logbeta;
        for (int col = 0; col < 7; col++) L.vlde.push_back((((u64)b * 7 + col) * beta + t) * n + m);
        for (int k = 0; k < DE; k++) L.vh.push_back((((u64)b * DE + k) * beta + t) * n + m);
    }
    // rows whose subtrees are recomputed: every queried row and its sibling row (the sibling's
    // subtree top, heap level log2(beta), is no longer stored)
    std::vector<u64> rows_b;
    for (u64 k : pos) {
        rows_b.push_back(k >> logbeta);
        rows_b.push_back((k >> logbeta) ^ 1);
    }
    std::sort(rows_b.begin(), rows_b.end());
    rows_b.erase(std::unique(rows_b.begin(), rows_b.end()), rows_b.end());
    for (u64 m : rows_b) L.oent.push_back(((u64)b << logn) | m);
    plan_batch_opening(pos, N, L.op);
    int64_t stored_ord = 0;
    L.op.each([&](u64 h) {
        if (h < stored_lim) {
            L.dt.push_back((u64)b * 2 * n + h);
            L.dh.push_back((u64)b * 2 * n + h);
            L.ref.push_back(stored_ord++);
        } else {
            // open slot relative to this proof's first entry (rebased once the entries of
            // the proofs before it are counted)
            unsigned lvl = (unsigned)(logn + logbeta) - (63 - __builtin_clzll(h));  // 0 = leaves
            u64 off = h - (N >> lvl), span = logbeta - lvl;
            u64 m = off >> span, local = (1ULL << span) + (off & ((1ULL << span) - 1));
            u64 e = (u64)(std::lower_bound(rows_b.begin(), rows_b.end(), m) - rows_b.begin());
            L.ref.push_back(-(int64_t)(e * 2 * LB + local) - 1);
        }
    });
    std::vector<u64> fp = pos;
    for (unsigned l = 0; l < nl; l++) {
        u64 rows = sh.D[l] / o.fold;
        fp = fold_positions(fp, rows);
        L.fpos.push_back(fp);
        auto& vf = L.vf[l];
        vf.clear();
        for (u64 i : fp)
            for (u64 k = 0; k < o.fold; k++) {
                const u64 K = i + k * rows;
                for (int cc = 0; cc < DE; cc++) {
                    if (l == 0)
                        vf.push_back((((u64)b * DE + cc) * beta + (K & (beta - 1))) * n + (K >> logbeta));
                    else
                        vf.push_back(((u64)b * DE + cc) * sh.D[l] + K);
                }
            }
        L.fops.emplace_back();
        plan_batch_opening(fp, rows, L.fops.back());
        auto& df = L.df[l];
        df.clear();
        L.fops.back().each([&](u64 x) { df.push_back((u64)b * 2 * rows + x); });
    }
}
// degree check, remainder commitment, grinding on the host, query positions, and proof b's gather lists
static inline void plan_queries(ProofJob& j, int b, const ProofShape& sh, const Opts& o, const ReplayView& rv,
                                LaneLayout& L) {
    plan_commit_remainder(j, b, sh, rv, L);
    plan_openings(j, b, sh, o, host_grind(j.coin.seed, o.grind), L);
}

// lays the B proofs' gather lists end to end (serial; ix's vectors are the lane's, so steady-state
// units do not allocate)
static inline void concat_indices(const std::vector<LaneLayout>& lay, int B, const ProofShape& sh, OpeningIndex& ix) {
    auto& allidx = ix.allidx;
    allidx.clear();
    ix.vseg.clear();
    ix.dseg.clear();
    const int NS = 2 + (int)sh.nl;  // value segments (same count of digest segments)
    ix.vcur.assign((size_t)NS * B, 0);
    ix.dcur.assign((size_t)NS * B, 0);
    auto seg_of = [&](int k, bool dig, int b) -> const std::vector<u64>& {
        const LaneLayout& L = lay[b];
        if (!dig) return k == 0 ? L.vlde : (k == 1 ? L.vh : L.vf[k - 2]);
        return k == 0 ? L.dt : (k == 1 ? L.dh : L.df[k - 2]);
    };
    for (int dig = 0; dig < 2; dig++)
        for (int k = 0; k < NS; k++) {
            auto& seg = dig ? ix.dseg : ix.vseg;
            auto& cur = dig ? ix.dcur : ix.vcur;
            seg.push_back({allidx.size(), 0});
            for (int b = 0; b < B; b++) {
                const auto& v = seg_of(k, dig, b);
                cur[(size_t)k * B + b] = allidx.size() - (dig ? ix.vseg.back().first + ix.vseg.back().second : 0);
                allidx.insert(allidx.end(), v.begin(), v.end());
            }
            seg.back().second = allidx.size() - seg.back().first;
        }
    ix.nvals = ix.dseg.front().first;
    ix.ndig = allidx.size() - ix.nvals;
    ix.nent = 0;
    ix.ent0.resize(B);
    for (int b = 0; b < B; b++) {
        ix.ent0[b] = (int64_t)ix.nent;
        allidx.insert(allidx.end(), lay[b].oent.begin(), lay[b].oent.end());
        ix.nent += lay[b].oent.size();
    }
}

// StarkProof::to_bytes (DESIGN.md "Proof format") of proof b into j.bytes. gv / gd: the gathered
// values and digests; gd holds the ndig stored digests, then the recomputed subtrees of the trace
// tree and of the composition tree (nent * 2 * beta slots each)
static inline void serialize_proof(ProofJob& j, int b, int B, const ProofShape& sh, const Opts& o,
                                   const LaneLayout& Lb, const OpeningIndex& ix, const u64* gv, const Digest* gd) {
    const int DE = sh.DE;
    const unsigned nl = sh.nl;
    const u64 LB = sh.beta, rem_len = sh.rem_len;
    const size_t nopen = ix.nent * 2 * LB;
    const Digest* open_t = gd + ix.ndig;
    const Digest* open_h = gd + ix.ndig + nopen;
    const size_t eoff = (size_t)ix.ent0[b] * 2 * LB;  // this proof's first recomputed-subtree slot
    auto write_paths = [&](BW& w, const BatchOpening& op, size_t cursor) {
        size_t slot = w.len_slot();
        w.u8(op.size());
        for (size_t i = 0; i < op.size(); i++) {
            w.u8(op.len[i]);
            w.put(&gd[cursor], 32 * op.len[i]);
            cursor += op.len[i];
        }
        w.len_patch(slot);
    };
    auto write_lde_paths = [&](BW& w, size_t cursor, const Digest* open) {
        size_t slot = w.len_slot();
        w.u8(Lb.op.size());
        size_t r = 0;
        for (size_t i = 0; i < Lb.op.size(); i++) {
            w.u8(Lb.op.len[i]);
            uint8_t* q = w.at(32 * Lb.op.len[i]);
            for (size_t k = 0; k < Lb.op.len[i]; k++, r++) {
                int64_t ref = Lb.ref[r];
                memcpy(q + 32 * k, (ref >= 0 ? gd[cursor++] : open[(size_t)(-ref - 1) + eoff]).w, 32);
            }
        }
        w.len_patch(slot);
    };
    const u64 nu = j.pos.size();
    BW w(j.bytes);
    w.reserve(j.commitments.size() + nu * 8 * (7 + DE + o.fold * DE * nl) + (2 + nl) * nu * 32 * ilog2(sh.N) +
              rem_len * 8 * DE + 1024);
    // Context
    w.u8(7); w.u8(0); w.u8(sh.logn); w.u16(0);
    w.u8(8); w.u64_(P);
    w.u8(o.q); w.u8(o.beta); w.u8(o.grind); w.u8(o.ext); w.u8(o.fold); w.u8(o.remdeg);
    w.u8(nu);
    w.u16(j.commitments.size());
    w.put(j.commitments.data(), j.commitments.size());
    // trace queries
    w.u8(1);
    w.u32(nu * 7 * 8);
    w.u64s(&gv[ix.vcur[b]], nu * 7);
    write_lde_paths(w, ix.dcur[b], open_t);
    // constraint queries
    w.u32(nu * 8 * DE);
    w.u64s(&gv[ix.vcur[(size_t)B + b]], nu * DE);
    write_lde_paths(w, ix.dcur[(size_t)B + b], open_h);
    // OOD frame (E elements)
    w.u16(1 + 14 * 8 * DE);
    w.u8(2);
    w.u64s(j.ood, 14 * DE);
    w.u16(8 * DE);
    w.u64s(j.ood + 14 * DE, DE);
    // FRI proof
    w.u8(nl);
    for (unsigned l = 0; l < nl; l++) {
        u64 nk = Lb.fpos[l].size();
        w.u32(nk * o.fold * 8 * DE);
        w.u64s(&gv[ix.vcur[(size_t)(2 + l) * B + b]], nk * o.fold * DE);
        write_paths(w, Lb.fops[l], ix.dcur[(size_t)(2 + l) * B + b]);
    }
    w.u16(rem_len * 8 * DE);
    w.u64s(j.rem.data(), rem_len * DE);
    w.u8(0);
    w.u64_(j.nonce);
    w.trim();
}

// Bytes of one serialised batch opening of `nu` leaves of an L-leaf tree (the u32 length, the u8
// vector count, one u8 length per vector, the digests): plan_batch_opening emits at most one node per
// distinct tree node at each level, so level j (2^j nodes) contributes at most min(nu, 2^j) digests.
static inline size_t opening_bound(u64 L, u64 nu) {
    size_t s = 4 + 1 + nu;
    for (unsigned j = 1; j <= ilog2(L); j++) s += 32 * std::min<u64>(nu, 1ULL << j);
    return s;
}

// The largest StarkProof::to_bytes serialize_proof emits for a shape, section by section as it
// writes them, with nu = min(q, N) unique queries (xfg_proof_size_bound). Tight (configs[2]: 98.8 KB
// against ~78 KB proofs), so a fixed-size exchange record per proof costs little (bench.py).
static inline size_t proof_size_bound(const ProofShape& sh, const Opts& o) {
    const u64 N = sh.N, nu = std::min<u64>(o.q, N);
    const unsigned nl = sh.nl;
    const size_t de = sh.DE == 2 ? 2 : 1;
    const u64 rem_len = std::max<u64>(sh.rem_len, 1);
    size_t s = 7 + 9 + 6 + 1;                            // Context, num_unique_queries
    s += 2 + 32 * (size_t)(3 + nl);                      // commitments: trace, composition, layers, remainder
    s += 1 + 4 + nu * 7 * 8 + opening_bound(N, nu);      // trace queries
    s += 4 + nu * 8 * de + opening_bound(N, nu);         // constraint queries
    s += 2 + 1 + 14 * 8 * de + 2 + 8 * de;               // OOD frame
    s += 1;                                              // FRI layer count
    for (unsigned l = 0; l < nl; l++) s += 4 + nu * o.fold * 8 * de + opening_bound(sh.D[l + 1], nu);
    s += 2 + rem_len * 8 * de + 1 + 8;                   // remainder, partitions, pow nonce
    return s + 64;
}

}  // namespace xfg
