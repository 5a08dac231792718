"""Proof size and throughput against the blowup factor at equal query security, and the LDE's time per output
point at the wide blowups.

  proofs  for each (blowup, queries) pair -- by default the reference shape n = 2^16 at 126 bits from the
          queries, 8:42 32:26 64:21 128:18, grinding 4 -- `batches` batches of `count` proofs with `depth` in
          flight, `rounds` times: proofs/s (median, min, max) and the proof bytes (min, mean, max)
  lde     xfg_bench_lde at n = 2^16: count x 7 polynomials at blowup 16, count / 2 at 32, count / 4 at 64 (the
          same number of output points), ns per output point. With XFG_LIB naming another build of the library
          the same script measures that build (a build without the wide blowups reports them as refused).

One JSON line per measurement.

usage: python3 scripts/blowup_bench.py [proofs|lde|all] [--pairs 8:42,32:26,64:21,128:18] [--logn 16]
                                       [--count 64] [--batches 12] [--rounds 3] [--depth 6] [--iters 20]"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "xfg-stark_amd"), ROOT]
import synthetic  # noqa: E402
import xfgstark  # noqa: E402


def proofs(args):
    n = 1 << args.logn
    inputs = [synthetic.burn_inputs(i) for i in range(args.count)]
    for pair in args.pairs.split(","):
        beta, q = (int(v) for v in pair.split(":"))
        pr = xfgstark.XfgBurnMintProver(proof_options=xfgstark.ProofOptions(q, beta, 4, 1, 8, 31))
        try:
            pr.prepare(args.count, n, buffers=args.depth + 1)
            sizes = [len(p.to_bytes()) for p in pr.prove_batch(inputs, n)]
            rates = []
            for _ in range(args.rounds):
                pending = collections.deque()
                t0 = time.perf_counter()
                for _ in range(args.batches):
                    pending.append(pr.submit_batch(inputs, n))
                    if len(pending) >= args.depth:
                        pending.popleft().result()
                while pending:
                    pending.popleft().result()
                rates.append(args.batches * args.count / (time.perf_counter() - t0))
            print(json.dumps({"what": "proofs", "n": n, "blowup": beta, "queries": q, "query_bits": q * (beta.bit_length() - 1),
                              "proof_bytes_min": min(sizes), "proof_bytes_mean": round(statistics.mean(sizes), 1),
                              "proof_bytes_max": max(sizes), "size_bound": pr.proof_size_bound(n),
                              "proofs_per_s_median": round(statistics.median(rates), 1), "proofs_per_s_min": round(min(rates), 1),
                              "proofs_per_s_max": round(max(rates), 1), "count": args.count, "batches": args.batches,
                              "depth": args.depth}), flush=True)
        finally:
            pr.close()


def lde(args):
    n = 1 << args.logn
    pr = xfgstark.XfgBurnMintProver()
    try:
        for beta in (16, 32, 64):
            count = max(1, args.count * 16 // beta)
            try:
                ms = [pr.bench_lde(count, n, beta, args.iters) for _ in range(3)]
            except xfgstark.XfgStarkError as e:
                print(json.dumps({"what": "lde", "n": n, "blowup": beta, "refused": e.status}), flush=True)
                continue
            points = count * 7 * n * beta
            print(json.dumps({"what": "lde", "n": n, "blowup": beta, "polys": count * 7, "output_points": points,
                              "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                              "ns_per_point": round(statistics.median(ms) * 1e6 / points, 5),
                              "lib": os.environ.get("XFG_LIB", "")}), flush=True)
    finally:
        pr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=["proofs", "lde", "all"])
    ap.add_argument("--pairs", default="8:42,32:26,64:21,128:18")
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if args.what in ("lde", "all"):
        lde(args)
    if args.what in ("proofs", "all"):
        proofs(args)


if __name__ == "__main__":
    main()
