"""Throughput of proving caller-supplied traces at the benchmark shape (64 proofs per batch, n = 2^16,
blowup 8, reference options, valid traces of synthetic.burn_inputs' AIRs), `depth` batches in flight as
bench.py keeps them:

  a  the loop of xfg_prove_trace (one trace per call, the only way before xfg_prove_trace_batch)
  b  prove_traces from a host array
  c  prove_traces from a device tensor
  cv c with validate=True (XFG_TRACE_VALIDATE)
  d  prove_batch on the same inputs (traces generated on the device): the ceiling
  e1 the traces held on the device as rows [64][2^16][7]: permute(0, 2, 1).contiguous() inside the timed loop
     (a second copy of the traces, a temporary of 64 x 7 x 2^16 x 8 bytes per batch), then submit_traces: what
     a producer of rows has to do with a library that takes the dense layout only
  e2 the same rows passed as the view rows.permute(0, 2, 1): read where they lie (xfg_prove_trace_batch_strided);
     left out when the library loaded through XFG_LIB has no such entry
  k  check_traces on the 64 device-resident traces of c, a host clock around `batches` calls one after the other
     (the call synchronises): traces/s
  kh k on the host array of b, at most 24 calls

The modes alternate `rounds` times in one process on one card; one JSON line per mode and round, then a
summary line per mode (median, min, max proofs/s). Then, in timing mode (one 64-proof unit, HIP events
around the stages), the first stage -- upload, check, interpolation and LDE of the trace -- of c and of
cv: their difference is the check kernel's time for 64 traces.

usage: python3 scripts/trace_batch_bench.py [batches per round, default 24] [rounds, 3] [depth, 6]
                                            [modes, comma-separated first letters, default all: a,b,c,cv,d,e1,e2,k,kh]"""
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xfg-stark_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before xfgstark: one HIP runtime in the process, see prove_traces)

torch.cuda.init()
import synthetic  # noqa: E402
import xfgstark  # noqa: E402

COUNT, LOGN = 64, 16
N = 1 << LOGN


def build_traces(airs):
    """build_trace of the reference AIR (src/burn_mint_air.rs:442-476): every column its asserted
    constant, column 4 the state floor(4 step / n)"""
    tr = np.empty((len(airs), 7, N), dtype=np.uint64)
    state = (4 * np.arange(N, dtype=np.uint64)) >> np.uint64(LOGN)
    for i, (pub, nullifier, commitment) in enumerate(airs):
        for c, v in enumerate((pub[0], pub[1], pub[2], pub[3], 0, nullifier, commitment)):
            tr[i, c] = v
        tr[i, 4] = state
    return tr


def pipelined(submit, batches, depth):
    """proofs/s of `batches` submissions with `depth` in flight; every result is collected and checked"""
    pending = collections.deque()
    t0 = time.perf_counter()
    for _ in range(batches):
        pending.append(submit())
        if len(pending) >= depth:
            done = pending.popleft().result()
            assert all(isinstance(p, xfgstark.StarkProof) for p in done)
    while pending:
        done = pending.popleft().result()
        assert all(isinstance(p, xfgstark.StarkProof) for p in done)
    return batches * COUNT / (time.perf_counter() - t0)


def main():
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    depth = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
    strided = "xfg_prove_trace_batch_strided_submit" not in xfgstark._abi.MISSING
    pr = xfgstark.XfgBurnMintProver()
    inputs = [synthetic.burn_inputs(i) for i in range(COUNT)]
    airs = [xfgstark.air_consts(**kw) for kw in inputs]
    host = build_traces(airs)
    dev = torch.from_numpy(host.view(np.int64)).to("cuda:0")
    rows = dev.permute(0, 2, 1).contiguous()  # [64][2^16][7], as a step function writes them
    torch.cuda.synchronize()
    assert pr.check_traces(dev, airs) == [None] * COUNT
    pr.prepare(COUNT, N, buffers=depth + 1)

    def single_loop():
        t0 = time.perf_counter()
        for i in range(COUNT):
            pr.prove_trace(host[i], *airs[i])
        return COUNT / (time.perf_counter() - t0)

    calls = {"a_prove_trace_loop": 1, "kh_check_host": min(batches, 24)}  # submissions per round; else `batches`

    def check_loop(traces, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            assert pr.check_traces(traces, airs) == [None] * COUNT
        return reps * COUNT / (time.perf_counter() - t0)

    modes = collections.OrderedDict([
        ("a_prove_trace_loop", lambda: single_loop()),
        ("b_host_array", lambda: pipelined(lambda: pr.submit_traces(host, airs), batches, depth)),
        ("c_device_tensor", lambda: pipelined(lambda: pr.submit_traces(dev, airs), batches, depth)),
        ("cv_device_validate", lambda: pipelined(lambda: pr.submit_traces(dev, airs, validate=True), batches, depth)),
        ("d_prove_batch", lambda: pipelined(lambda: pr.submit_batch(inputs, N), batches, depth)),
        ("e1_rows_permute_copy", lambda: pipelined(lambda: pr.submit_traces(rows.permute(0, 2, 1).contiguous(), airs),
                                                   batches, depth)),
        ("e2_rows_view", lambda: pipelined(lambda: pr.submit_traces(rows.permute(0, 2, 1), airs), batches, depth)),
        ("k_check_device", lambda: check_loop(dev, batches)),
        ("kh_check_host", lambda: check_loop(host, calls["kh_check_host"])),
    ])
    if not strided:
        del modes["e2_rows_view"]
    if only:
        modes = collections.OrderedDict((k, v) for k, v in modes.items() if k.split("_")[0] in only)
    # the same proofs whichever way the traces arrive
    want = [p.to_bytes() for p in pr.prove_batch(inputs, N)]
    for how in (host, dev):
        for validate in (False, True):
            assert [p.to_bytes() for p in pr.prove_traces(how, airs, validate=validate)] == want
    assert [p.to_bytes() for p in pr.prove_traces(rows.permute(0, 2, 1).contiguous(), airs)] == want
    if strided:
        for validate in (False, True):
            assert [p.to_bytes() for p in pr.prove_traces(rows.permute(0, 2, 1), airs, validate=validate)] == want
    pr.prepare(COUNT, N)  # the context has seen host traces: the lanes' pinned staging is sized now
    for name, run in modes.items():  # warm every path once
        run() if name.startswith(("a_", "k")) else pipelined(
            {"b": lambda: pr.submit_traces(host, airs), "c": lambda: pr.submit_traces(dev, airs),
             "cv": lambda: pr.submit_traces(dev, airs, validate=True),
             "d": lambda: pr.submit_batch(inputs, N),
             "e1": lambda: pr.submit_traces(rows.permute(0, 2, 1).contiguous(), airs),
             "e2": lambda: pr.submit_traces(rows.permute(0, 2, 1), airs)}[name.split("_")[0]], depth + 1, depth)
    rates = collections.defaultdict(list)
    for r in range(rounds):
        for name, run in modes.items():
            v = run()
            rates[name].append(v)
            print(json.dumps({"round": r, "mode": name, "proofs_per_s": round(v, 1)}), flush=True)
    for name, v in rates.items():
        print(json.dumps({"mode": name, "median": round(statistics.median(v), 1), "min": round(min(v), 1),
                          "max": round(max(v), 1), "batches": calls.get(name, batches),
                          "depth": depth}), flush=True)
    bytes_per_batch = host.nbytes
    if "b_host_array" in rates:
        print(json.dumps({"trace_bytes_per_batch": bytes_per_batch,
                          "b_upload_GBps": round(statistics.median(rates["b_host_array"]) / COUNT * bytes_per_batch / 1e9, 2)}),
              flush=True)
    if only and not {"c", "cv"} <= set(only):
        pr.close()
        return
    # the check kernel's own time: stage 0 of one 64-proof unit with and without the check
    pr.set_timing(True)
    stage = {"c": [], "cv": []}
    for _ in range(6):
        for key, validate in (("c", False), ("cv", True)):
            pr.prove_traces(dev, airs, validate=validate)
            t = pr.stage_times()
            stage[key].append((t["trace_lde"], sum(v for k, v in t.items() if not k.startswith("host"))))
    pr.set_timing(False)
    for key in ("c", "cv"):
        lde = sorted(s[0] for s in stage[key][1:])
        chain = sorted(s[1] for s in stage[key][1:])
        print(json.dumps({"timing_mode": key, "stage0_ms_median": round(statistics.median(lde), 4),
                          "stage0_ms_min": round(lde[0], 4), "device_chain_ms_median": round(statistics.median(chain), 3)}),
              flush=True)
    pr.close()


if __name__ == "__main__":
    main()
