"""Host verifier alone, no GPU: `distinct` oracle-made configs[2] proofs (n = 2^16, reference options)
repeated to `count` items through batch_verify(..., threads=1), proofs/s, best of `reps`.
usage: python3 scripts/verify_host_probe.py [count] [reps] [distinct]   (XFG_LIB selects the build)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xfg-stark_amd"), os.path.join(ROOT, "tests"), ROOT]
import xfgstark  # noqa: E402
import oracle_lib as O  # noqa: E402
import synthetic  # noqa: E402

count = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
distinct = int(sys.argv[3]) if len(sys.argv) > 3 else 8
n = 1 << 16
items = []
for i in range(distinct):
    kw = synthetic.burn_inputs(i)
    st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
    st2, proof = O.prove(air, n, O.options())
    assert st == 0 and st2 == 0
    items.append((proof, xfgstark.air_consts(**kw)))
items = [items[i % distinct] for i in range(count)]
v = xfgstark.XfgBurnMintVerifier()
best = None
for _ in range(reps):
    t = time.perf_counter()
    ok = v.batch_verify(items, threads=1)
    dt = time.perf_counter() - t
    assert all(ok)
    best = dt if best is None else min(best, dt)
print(f"host threads=1: {count / best:.0f} proofs/s ({best * 1e3:.2f} ms per {count})", flush=True)
