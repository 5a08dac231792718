// Host side of the batched GPU verifier (xfg_verify_batch_gpu): transcripts and plans per proof on
// the host pool (verifier.cpp), one staging upload, the two kernels of verify_kernels.hip on lane
// 0's stream, verdicts by finish_proof: the host verifier's check order, except that a broken FRI
// structure is reported before anything the device would have checked (verifier.hpp plan_proof).
// The caller's policy (acceptable.hpp) is checked per proof in verify_transcript; the planned proofs may
// then have any mix of options, and the device sees their queries grouped by folding factor.
#include <algorithm>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "dispatch.hpp"
#include "host_pool.hpp"
#include "prover_internal.hpp"

using namespace xfg;

// the body of xfg_verify_batch_gpu, xfg_debug_verify_batch_gpu and their _acceptable forms; flags_out /
// errs are the debug entries' outputs (null: not wanted)
static int verify_batch_gpu(xfg_ctx* c, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                            const xfg_air_consts* airs, const Acceptable& acc, int* results, uint64_t* flags_out,
                            char* errs, size_t err_stride) {
    if (!c || !proofs || !lens || !airs || !results) return XFG_INVALID_ARGUMENT;
    c->err.clear();
    return on_lane0(c, [&](Lane* L0) -> int {
        HostTrace ht;
        ht.mark("start");
        // per-proof transcript states and plan fragments are kept in the context between calls
        // (reset in place: a large batch would otherwise allocate and free ~10^5 small blocks)
        auto& V = c->vb;
        if (V.st.size() < count) V.st.resize(count);
        if (V.frag.size() < count) V.frag.resize(count);
        std::vector<VState>& st = V.st;
        std::vector<std::string> err(count);
        // per-proof host phases on the host pool (spawning 16 threads per phase cost more than the
        // phases' own work at 64 proofs); a proof per task
        auto parallel = [&](const std::function<void(uint32_t)>& f) {
            host_pool().parallel_for((int)count, [&](int i) { f((uint32_t)i); });
        };
        // 1. transcripts (host threads)
        parallel([&](uint32_t i) {
            if (!proofs[i]) {
                err[i] = "null proof";
                return;
            }
            try {
                err[i] = verify_transcript(proofs[i], lens[i], air_of(&airs[i]), acc, st[i]);
            } catch (const std::exception& e) {
                err[i] = std::string("ProofDeserializationError(\"") + e.what() + "\")";
            }
        });
        ht.mark("transcripts");
        // 2. plan: per-proof fragments (openings, queries) built in parallel; blob offsets by prefix
        //    sum of the accepted proofs' lengths. A proof whose FRI structure is broken is not sent to
        //    the device: its flag word stays 0 and finish_proof reports the break
        std::vector<size_t> boff(count + 1, 0);
        for (uint32_t i = 0; i < count; i++) boff[i + 1] = boff[i] + (err[i].empty() ? lens[i] : 0);
        std::vector<VerifyPlan>& frag = V.frag;
        parallel([&](uint32_t i) {
            if (err[i].empty()) plan_proof(st[i], boff[i], frag[i]);
        });
        ht.mark("plan_fragments");
        // 3. concatenate into one pinned staging region (parallel fill) and one DMA. Trees, leaves, vectors
        //    and proof records lie in input order; the query records lie by folding factor, one contiguous
        //    range per vfield_kernel instantiation (bucket_queries: input order within a range)
        struct Off {
            size_t t = 0, lf = 0, v = 0, fp = 0;
        };
        std::vector<Off> fo(count + 1);
        std::vector<int> planned(count, -1);
        std::vector<uint32_t> nq(count, 0);
        std::vector<uint8_t> logf(count, 0);  // 0: not planned
        for (uint32_t i = 0; i < count; i++) {
            const VerifyPlan& f = frag[i];
            const bool ok = err[i].empty() && f.broken < 0;
            Off& a = fo[i];
            Off& b = fo[i + 1];
            b.t = a.t + (ok ? f.trees.size() : 0);
            b.lf = a.lf + (ok ? f.tleaves.size() : 0);
            b.v = a.v + (ok ? f.vecs.size() : 0);
            b.fp = a.fp + (ok ? 1 : 0);
            if (ok) {
                planned[i] = (int)a.fp;
                nq[i] = (uint32_t)f.fqueries.size();
                logf[i] = (uint8_t)fold_log2((long long)st[i].pf.o.fold);  // 1..4 (check_options)
            }
        }
        const Off& E = fo[count];
        std::vector<uint64_t> q0(count, 0);  // item i's first query record
        FoldRanges ranges;
        if (!bucket_queries(count, nq.data(), logf.data(), q0.data(), ranges))
            throw std::logic_error("verify_batch_gpu: a planned proof without a folding-factor kernel");
        const size_t nqueries = (size_t)ranges.begin[4];
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_blob = 0, o_t = al(boff[count]), o_lf = al(o_t + E.t * sizeof(VTree)),
                     o_v = al(o_lf + E.lf * sizeof(VTreeLeaf)), o_fp = al(o_v + E.v * sizeof(VVec)),
                     o_fq = al(o_fp + E.fp * sizeof(VFieldProof)), total_b = al(o_fq + nqueries * sizeof(VFieldQuery));
        uint8_t* H = V.stage.ensure(total_b);
        VTree* ht_ = (VTree*)(H + o_t);
        VTreeLeaf* hlf = (VTreeLeaf*)(H + o_lf);
        VVec* hv = (VVec*)(H + o_v);
        VFieldProof* hfp = (VFieldProof*)(H + o_fp);
        VFieldQuery* hfq = (VFieldQuery*)(H + o_fq);
        parallel([&](uint32_t i) {
            if (planned[i] < 0) return;
            memcpy(H + o_blob + boff[i], proofs[i], lens[i]);
            const VerifyPlan& f = frag[i];
            const Off& a = fo[i];
            for (size_t k = 0; k < f.trees.size(); k++) {
                VTree t = f.trees[k];
                t.leaf0 += (uint32_t)a.lf;
                t.vec0 += (uint32_t)a.v;
                t.proof = (uint32_t)a.fp;
                ht_[a.t + k] = t;
            }
            memcpy(hlf + a.lf, f.tleaves.data(), f.tleaves.size() * sizeof(VTreeLeaf));
            memcpy(hv + a.v, f.vecs.data(), f.vecs.size() * sizeof(VVec));
            hfp[a.fp] = f.fproof;
            for (size_t k = 0; k < f.fqueries.size(); k++) {
                hfq[q0[i] + k] = f.fqueries[k];
                hfq[q0[i] + k].proof = (uint32_t)a.fp;
            }
        });
        ht.mark("plan_merge");
        std::vector<u64> flags(E.fp, 0);
        if (E.fp > 0) {
            hipStream_t s = L0->stream;
            V.dstage.ensure(total_b);
            V.flags.ensure(E.fp);
            HIPCHK(hipMemcpyAsync(V.dstage.p, H, total_b, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(V.flags.p, 0, E.fp * 8, s));
            ht.mark("upload_enqueue");
            uint8_t* D = V.dstage.p;
            launch_verify(D + o_blob, (const VTree*)(D + o_t), E.t, (const VTreeLeaf*)(D + o_lf), (const VVec*)(D + o_v),
                          (const VFieldProof*)(D + o_fp), (const VFieldQuery*)(D + o_fq), ranges, V.flags.p, s);
            HIPCHK(hipMemcpyAsync(flags.data(), V.flags.p, flags.size() * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            ht.mark("device");
        }
        // 4. verdicts (finish_proof)
        parallel([&](uint32_t i) {
            if (err[i].empty())
                err[i] = finish_proof(st[i], frag[i].broken, planned[i] >= 0 ? flags[planned[i]] : 0);
            results[i] = proofs[i] ? (err[i].empty() ? XFG_OK : XFG_VERIFY_FAILED) : XFG_INVALID_ARGUMENT;
            if (flags_out) flags_out[i] = planned[i] >= 0 ? flags[planned[i]] : 0;
            if (errs && err_stride) {
                const size_t k = std::min(err_stride - 1, err[i].size());
                memcpy(errs + i * err_stride, err[i].data(), k);
                errs[i * err_stride + k] = 0;
            }
        });
        ht.mark("finish");
        ht.dump((int)count);
        return XFG_OK;
    });
}

extern "C" int xfg_verify_batch_gpu(xfg_ctx* c, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                                    const xfg_air_consts* airs, const xfg_options* acceptable, int* results) {
    if (!acceptable) return XFG_INVALID_ARGUMENT;
    return verify_batch_gpu(c, count, proofs, lens, airs, acceptable_one(to_opts(acceptable)), results, nullptr,
                            nullptr, 0);
}
extern "C" int xfg_verify_batch_gpu_acceptable(xfg_ctx* c, uint32_t count, const uint8_t* const* proofs,
                                               const size_t* lens, const xfg_air_consts* airs,
                                               const xfg_acceptable* acceptable, int* results) {
    Acceptable a;
    if (!make_acceptable(acceptable, a)) return XFG_INVALID_ARGUMENT;
    return verify_batch_gpu(c, count, proofs, lens, airs, a, results, nullptr, nullptr, 0);
}

extern "C" int xfg_debug_verify_batch_gpu(xfg_ctx* c, uint32_t count, const uint8_t* const* proofs, const size_t* lens,
                                          const xfg_air_consts* airs, const xfg_options* acceptable, int* results,
                                          uint64_t* flags, char* errs, size_t err_stride) {
    if (!flags || !errs || !err_stride || !acceptable) return XFG_INVALID_ARGUMENT;
    return verify_batch_gpu(c, count, proofs, lens, airs, acceptable_one(to_opts(acceptable)), results, flags, errs,
                            err_stride);
}
extern "C" int xfg_debug_verify_batch_gpu_acceptable(xfg_ctx* c, uint32_t count, const uint8_t* const* proofs,
                                                     const size_t* lens, const xfg_air_consts* airs,
                                                     const xfg_acceptable* acceptable, int* results, uint64_t* flags,
                                                     char* errs, size_t err_stride) {
    Acceptable a;
    if (!flags || !errs || !err_stride || !make_acceptable(acceptable, a)) return XFG_INVALID_ARGUMENT;
    return verify_batch_gpu(c, count, proofs, lens, airs, a, results, flags, errs, err_stride);
}
