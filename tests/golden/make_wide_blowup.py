"""Writes tests/golden/wide_blowup_proofs.json: length and SHA-256 of the CPU oracle's proofs at the blowup
32 / 128 shapes whose oracle run is too slow to repeat next to the GPU tests (wide_blowup_cases.GOLDEN_CASES,
synthetic.burn_inputs(GOLDEN_SEED + i)). Recorded results only; run from the repository root:
    python tests/golden/make_wide_blowup.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import fold_cases as FC  # noqa: E402
import oracle_lib as O  # noqa: E402
import synthetic  # noqa: E402
import wide_blowup_cases as W  # noqa: E402


def main():
    out = []
    for case in W.GOLDEN_CASES:
        opts = FC.oracle_options(case)
        for i in range(W.GOLDEN_PROOFS):
            air = FC.oracle_air(synthetic.burn_inputs(W.GOLDEN_SEED + i))
            st, proof = O.prove(air, case[0], opts)
            assert st == 0 and O.verify(air, proof, opts) == 0
            out.append({"case": list(case), "index": i, "len": len(proof), "sha256": hashlib.sha256(proof).hexdigest()})
            print(out[-1], flush=True)
    with open(os.path.join(HERE, "wide_blowup_proofs.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
