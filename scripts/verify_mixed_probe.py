"""Batch verification of proofs of mixed options on the GPU: `per` proofs per folding factor (2, 4, 8, 16; the
reference options otherwise, n = 2^16), made by the prover, verified in one xfg_verify_batch_gpu_acceptable
call under the set of the four option sets, against the same proofs in four homogeneous xfg_verify_batch_gpu
calls (their times added). Best of `reps`; with XFG_TRACE=1 the GPU path prints its host phase times.
usage: python3 scripts/verify_mixed_probe.py [per] [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xfg-stark_amd"), ROOT]
import xfgstark  # noqa: E402
import synthetic  # noqa: E402

per = int(sys.argv[1]) if len(sys.argv) > 1 else 16
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << 16
FACTORS = (2, 4, 8, 16)


def options(fold):
    o = xfgstark.ProofOptions.reference()
    o.fri_folding_factor = fold
    return o


pr = xfgstark.XfgBurnMintProver()
groups = {}
for j, fold in enumerate(FACTORS):
    kws = [synthetic.burn_inputs(1000 * j + i) for i in range(per)]
    pr._options = options(fold)
    proofs = [p.to_bytes() for p in pr.prove_batch(kws, trace_length=n)]
    groups[fold] = [(p, xfgstark.air_consts(**kw)) for p, kw in zip(proofs, kws)]
mixed = [groups[fold][i] for i in range(per) for fold in FACTORS]  # neighbours have different factors
policy = xfgstark.AcceptableOptions.option_set([options(f) for f in FACTORS])
one_call = xfgstark.XfgBurnMintVerifier(acceptable=policy)
per_factor = {f: xfgstark.XfgBurnMintVerifier(proof_options=options(f)) for f in FACTORS}


def timed(fn):
    t = time.perf_counter()
    ok = fn()
    dt = time.perf_counter() - t
    assert all(ok)
    return dt


best_mixed = min(timed(lambda: one_call.batch_verify(mixed, gpu=pr)) for _ in range(reps))
best_split = min(sum(timed(lambda f=f: per_factor[f].batch_verify(groups[f], gpu=pr)) for f in FACTORS)
                 for _ in range(reps))
best_host = min(timed(lambda: one_call.batch_verify(mixed, threads=16)) for _ in range(reps))
count = per * len(FACTORS)
for name, dt in (("one mixed call", best_mixed), ("four homogeneous calls", best_split), ("host, 16 threads", best_host)):
    print(f"{name}: {count / dt:.0f} proofs/s ({dt * 1e3:.2f} ms per {count})", flush=True)
print(json.dumps({"proofs": count, "per_factor": per, "log_n": 16, "reps": reps,
                  "mixed_one_call_proofs_per_s": round(count / best_mixed, 1),
                  "four_calls_proofs_per_s": round(count / best_split, 1),
                  "host_16_threads_proofs_per_s": round(count / best_host, 1)}))
pr.close()
