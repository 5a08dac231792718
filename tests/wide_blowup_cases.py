"""The shapes of the blowup 32 / 64 / 128 tests (CPU and GPU) and the oracle's proofs of them, made once per
process and shared by every test that needs them.

TEST INFRASTRUCTURE ONLY. A case is fold_cases' (n, blowup, remainder max degree, queries, fold, ext). Every
listed shape keeps q < N and the last FRI layer at the blowup factor or more (and at 8 points or more): the
shapes the prover takes and the only ones the oracle is called on."""
import functools

import numpy as np

import fold_cases as FC
import oracle_lib as O
import plain_ref as R

WIDE = (32, 64, 128)
MAX_LDE = 1 << 24  # n * blowup of a shape with blowup > 16

# (n, blowup, remainder max degree, queries); at n = 8 the 255 queries open every row of both LDE trees.
# A lone proof with n >= 1024 takes the two-lanes-per-row leaf kernel: (4096, 32), (1024, 64), (1024, 128);
# the smaller n take the one-lane kernel at each of the three factors
SHAPES = [(8, 32, 31, 255), (8, 128, 31, 255), (64, 64, 31, 21), (64, 128, 31, 42), (256, 32, 31, 42),
          (1024, 64, 31, 42), (1024, 128, 31, 42), (4096, 32, 31, 42)]
OTHER_FOLDS = [(64, 64, 31, 21), (1024, 128, 31, 42)]  # also proven with the folding factors 2, 4 and 16


def admitted(n, beta, remdeg, fold):
    """the last-layer rule: the last FRI layer holds the blowup factor or more (and the oracle's 8 points)"""
    return FC.num_layers(n, beta, remdeg, fold)[1] >= max(8, beta)


PROOF_CASES = [s + (8, ext) for s in SHAPES for ext in (1, 2)]
PROOF_CASES += [s + (f, ext) for s in OTHER_FOLDS for f in (2, 4, 16) if admitted(s[0], s[1], s[2], f) for ext in (1, 2)]
assert len(PROOF_CASES) == 16 + 12, "every other folding factor is admitted at both shapes"
for _c in PROOF_CASES:
    assert _c[3] < _c[0] * _c[1] <= MAX_LDE and admitted(_c[0], _c[1], _c[2], _c[4]), _c

# the verifier cases of the CPU test: (n, blowup) x both fields, folding factor 8
VERIFY_CASES = [(8, 32, 31, 42, 8, ext) for ext in (1, 2)] + [(64, 64, 31, 21, 8, ext) for ext in (1, 2)] + \
               [(64, 128, 31, 42, 8, ext) for ext in (1, 2)] + [(256, 32, 31, 42, 8, ext) for ext in (1, 2)]
TAMPER_CASES = [(64, 64, 31, 21, 8, ext) for ext in (1, 2)]

# xfg_proof_size_bound: (n, blowup, queries, ext, remainder max degree)
BOUND_CASES = [(8, 32, 255, 1, 0), (8, 128, 255, 2, 7), (64, 64, 21, 1, 31), (1024, 128, 100, 2, 255), (4096, 32, 42, 1, 31)]

# tests/golden/wide_blowup_proofs.json (tests/golden/make_wide_blowup.py): sizes the oracle is not run at
# next to the GPU; synthetic.burn_inputs(GOLDEN_SEED + i), i < GOLDEN_PROOFS
GOLDEN_SEED, GOLDEN_PROOFS = 7100, 2
GOLDEN_CASES = [(1 << 16, 32, 31, 42, 8, 1), (1 << 12, 128, 31, 24, 8, 2)]

case_id = FC.case_id


def air_struct(air):
    """O.Air from (pub[12], nullifier, commitment)"""
    oa = O.Air()
    for i in range(12):
        oa.pub[i] = air[0][i]
    oa.secret = 0
    oa.nullifier = air[1]
    oa.commitment = air[2]
    return oa


def flat(tr):
    tr = np.asarray(tr, dtype=np.uint64)
    return (O.C.c_uint64 * tr.size)(*[int(v) for v in tr.reshape(-1)])


@functools.lru_cache(maxsize=None)
def false_proof(c):
    """a uniformly random trace (no burn trace: the statement is false), its AIR constants, the oracle's AIR
    and the oracle's proof over that trace -> (trace [7][n] uint64, air tuple, O.Air, proof bytes)"""
    n, beta, remdeg, q, fold, ext = c
    cols, air = R.make_trace("random", n, 8100 + 3 * n + 7 * beta + 11 * fold + ext)
    tr = np.array(cols, dtype=np.uint64)
    oa = air_struct(air)
    st, proof = O.prove(oa, n, FC.oracle_options(c), trace=flat(tr))
    assert st == 0
    return tr, air, oa, proof
