"""Throughput of the headline shape (64 proofs per step, n = 2^16, reference options, `depth` steps in flight as
bench.py keeps them) with the statements arriving three ways:

  batch         submit_batch on the 64 statements as dicts (xfg_prove_batch_submit: ctypes structs, validation,
                marshalling and Keccak on the host pool at every submission)
  records       submit_records on a resident device tensor of the same 64 statements as packed records
                (xfg_prove_records_submit, XFG_RECORDS_ON_DEVICE: the record kernel at the head of every unit)
  records_host  submit_records on the same records as a host array

One mode per process, so that `batch` can be run on another build of the library through XFG_LIB (the parent
commit's, which has no record entries) and the processes interleaved on one card:

    for i in 1 2 3; do XFG_LIB=parent.so python3 scripts/records_bench.py batch; python3 scripts/records_bench.py records; done

Prints one JSON line: mode, steps, proofs_per_s, the library, and `checked`: the proofs of the first step equal
prove_batch's bytes.

usage: python3 scripts/records_bench.py MODE [timed steps, default 20] [warm-up steps, 7] [depth, 6]"""
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xfg-stark_amd"), ROOT]
import torch  # noqa: E402  (before xfgstark: one HIP runtime in the process, see submit_records)

torch.cuda.init()
import synthetic  # noqa: E402
import xfgstark  # noqa: E402

COUNT, N = 64, 1 << 16


def pipelined(submit, steps, depth):
    pending = collections.deque()
    t0 = time.perf_counter()
    for _ in range(steps):
        pending.append(submit())
        if len(pending) >= depth:
            done = pending.popleft().result()
            assert all(isinstance(p, xfgstark.StarkProof) for p in done)
    while pending:
        done = pending.popleft().result()
        assert all(isinstance(p, xfgstark.StarkProof) for p in done)
    return steps * COUNT / (time.perf_counter() - t0)


def main():
    mode = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    depth = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    pr = xfgstark.XfgBurnMintProver()
    inputs = [synthetic.burn_inputs(i) for i in range(COUNT)]
    if mode == "batch":
        def submit():
            return pr.submit_batch(inputs, N)
    else:
        records = xfgstark.pack_records(inputs)
        if mode == "records":
            records = torch.from_numpy(records).to("cuda:0")
            torch.cuda.synchronize()
        elif mode != "records_host":
            raise SystemExit(__doc__)

        def submit():
            return pr.submit_records(records, N)
    pr.prepare(COUNT, N, buffers=depth + 1)
    want = [p.to_bytes() for p in pr.prove_batch(inputs, N)]
    checked = [p.to_bytes() for p in submit().result()] == want
    pipelined(submit, warmup, depth)
    rate = pipelined(submit, steps, depth)
    print(json.dumps({"mode": mode, "steps": steps, "depth": depth, "proofs_per_s": round(rate, 1),
                      "lib": os.path.basename(os.path.dirname(xfgstark.LIB_PATH)) + "/" + os.path.basename(xfgstark.LIB_PATH),
                      "checked": checked}), flush=True)
    pr.close()
    if not checked:
        raise SystemExit("the proofs differ from prove_batch's")


if __name__ == "__main__":
    main()
