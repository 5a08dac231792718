"""Generator of tests/golden/grind_seeds.json: seeds whose smallest proof-of-work nonce, at a stated
grinding factor, is exactly a chosen value -- the first and last lane of a 256-nonce chunk, the chunk after it,
and chunks a block reaches with its second and third claim (tests/test_grinding_gpu.py).

For a target T at factor g a candidate seed is kept when nonce T passes (one hash, probability 2^-g) and no
nonce below T does (T - 1 hashes, probability (1 - 2^-g)^(T - 1), about a half for the factors chosen below),
so a seed costs a few thousand hashes. Candidates are BLAKE3("grind-fixture/<T>/<counter>"), counter from 0.

Usage: python tests/golden/make_grind_seeds.py   (from the repository root; needs the oracle built)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import grind_ref as G  # noqa: E402
import oracle_lib as O  # noqa: E402

C = 256
# (nonce, grinding factor): the factor grows with the nonce so that about half the candidates whose
# nonce T passes have no earlier one
TARGETS = [(1, 8), (2, 8), (C, 9), (C + 1, 9), (2 * C, 9), (2 * C + 1, 9), (3 * C, 10), (3 * C + 1, 10), (6 * C + 1, 11)]


def find(target, grind):
    k = 0
    while True:
        seed = O.blake3(f"grind-fixture/{target}/{k}".encode())
        k += 1
        if G.zeros(seed, target) >= grind and G.min_nonce(seed, grind, 1, target) == target:
            return seed


def main():
    out = [dict(seed=find(t, g).hex(), grind=g, nonce=t) for t, g in TARGETS]
    with open(os.path.join(HERE, "grind_seeds.json"), "w") as f:
        json.dump(dict(chunk=C, seeds=out), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
