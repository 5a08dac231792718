"""Forged proofs that commit consistently, for the verifier tests (CPU and GPU): the shapes, the fault
lists, the oracle's cheating prover on each (orc_prove_faulty, made once per process and shared) and what
every verifier must answer.

TEST INFRASTRUCTURE ONLY. A forged proof carries one algebraic error that was injected before the values
it alters were hashed, so every commitment check passes and one algebraic check alone (the DEEP value at
the query points, one FRI layer's fold, the remainder evaluation) can reject it. A case is fold_cases'
(n, blowup, remainder max degree, queries, fold, ext)."""
import functools
import os
import random
from concurrent.futures import ThreadPoolExecutor

import fold_cases as FC
import oracle_lib as O
import synthetic

P = 0xFFFFFFFF00000001
# (n, blowup, remainder max degree, queries, fold) -> FRI layers
SHAPES = {
    (8, 8, 7, 7, 8): 0,          # the DEEP value is compared with the remainder directly
    (64, 8, 31, 42, 8): 1,
    (1024, 8, 31, 42, 8): 2,
    (1024, 16, 31, 24, 16): 2,
    (256, 4, 7, 42, 4): 3,
    (256, 8, 7, 42, 2): 5,
    (8192, 8, 0, 42, 2): 13,     # flag bits up to 12
}
for _s, _nl in SHAPES.items():
    _got, _last = FC.num_layers(_s[0], _s[1], _s[2], _s[4])
    assert _got == _nl and _last >= max(8, _s[1]), (_s, _got, _last)
CASES = [s + (ext,) for s in SHAPES for ext in (1, 2)]
case_id = FC.case_id

STATEMENTS = 3  # honest proofs per case, one per statement; the forged proofs rotate over them

LAYER_FOLDING = "FriVerificationFailed(InvalidLayerFolding)"
REMAINDER_FOLDING = "FriVerificationFailed(InvalidRemainderFolding)"
OOD = "InconsistentOodConstraintEvaluations"
BIT_REMAINDER = 1 << 63
COMMITMENT_BITS = ((1 << 63) - 1) ^ ((1 << 32) - 1)  # bits 32..62: what vtree_kernel sets


def layers(c):
    return FC.num_layers(c[0], c[1], c[2], c[4])[0]


def remainder_len(c):
    return FC.num_layers(c[0], c[1], c[2], c[4])[1] // c[1]


def _positions(c):
    """the fault lists of a case, without deltas: [[(kind, index)]]"""
    n, nl, rl = c[0], layers(c), remainder_len(c)
    out = [[(O.FAULT_OOD_NEXT, col)] for col in (0, 3, 4, 6)]
    out += [[(O.FAULT_DEEP_COEF, j)] for j in (0, n - 2)]
    out += [[(O.FAULT_LAYER, l)] for l in sorted({1, nl // 2, nl - 1}) if 1 <= l < nl]
    out += [[(O.FAULT_REMAINDER, k)] for k in sorted({0, rl - 1})]
    if nl >= 2:
        out.append([(O.FAULT_LAYER, 1), (O.FAULT_REMAINDER, 0)])
    return out


def fault_lists(c):
    """[[(kind, index, (d0, d1))]]: every fault list of the case; with the extension each one three
    times, the delta on the first coordinate, on the second alone (what a one-coordinate comparison
    misses) and on both. d walks through 1, p - 1, 2^32 and a random value seeded by the case."""
    n, beta, remdeg, q, fold, ext = c
    rng = random.Random(771 + n + 7 * beta + 3 * remdeg + 11 * fold + ext)
    ds = [1, P - 1, 1 << 32, rng.randrange(2, P - 1)]
    out, k = [], 0
    for fl in _positions(c):
        for form in ("first",) if ext == 1 else ("first", "second", "both"):
            lst = []
            for kind, index in fl:
                d, d2 = ds[k % 4], ds[(k + 1) % 4]
                lst.append((kind, index, {"first": (d, 0), "second": (0, d), "both": (d, d2)}[form]))
                k += 1
            out.append(lst)
    return out


def expected(c, faults):
    """(host verifier error, device flag word) of a proof with these faults; (None, 0) for an honest one"""
    if not faults:
        return None, 0
    nl = layers(c)
    if len(faults) == 2:  # LAYER 1 + REMAINDER 0: the host stops at the first, the device checks every layer
        return LAYER_FOLDING, (1 << 1) | BIT_REMAINDER
    kind, index, _ = faults[0]
    if kind == O.FAULT_OOD_NEXT and index == 4:  # the only next-state value the AIR reads
        return OOD, 0  # rejected while the transcript is replayed: never planned
    if kind == O.FAULT_REMAINDER:
        return REMAINDER_FOLDING, BIT_REMAINDER
    if kind == O.FAULT_LAYER:
        return LAYER_FOLDING, 1 << index
    assert kind in (O.FAULT_OOD_NEXT, O.FAULT_DEEP_COEF)
    return (LAYER_FOLDING, 1) if nl >= 1 else (REMAINDER_FOLDING, BIT_REMAINDER)


def statement_inputs(c, k):
    """burn inputs of statement k of the case"""
    n, beta, remdeg, q, fold, ext = c
    return synthetic.burn_inputs(31000 + 16 * (n + 7 * beta + 3 * remdeg + 11 * fold + ext) + k)


@functools.lru_cache(maxsize=None)
def proofs(c):
    """[(statement k, burn inputs, oracle AIR, fault list, prover status, proof bytes)]: the honest proof
    of each of the STATEMENTS statements (fault list []), then every forged proof of fault_lists(c), forged
    proof i on statement i mod STATEMENTS. The oracle proves on a few threads (it keeps no shared state)."""
    opts = FC.oracle_options(c)
    kws = [statement_inputs(c, k) for k in range(STATEMENTS)]
    airs = [FC.oracle_air(kw) for kw in kws]
    jobs = [(k, []) for k in range(STATEMENTS)] + [(i % STATEMENTS, fl) for i, fl in enumerate(fault_lists(c))]

    def run(job):
        k, fl = job
        st, proof = O.prove_faulty(airs[k], c[0], opts, fl)
        return k, kws[k], airs[k], fl, st, proof
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(run, jobs))


def interleaved(c):
    """proofs(c) reordered so that the honest proofs stand between the forged ones"""
    items = proofs(c)
    honest, forged = items[:STATEMENTS], items[STATEMENTS:]
    step = max(1, len(forged) // STATEMENTS)
    out = []
    for i, it in enumerate(forged):
        if i % step == 0 and i // step < STATEMENTS:
            out.append(honest[i // step])
        out.append(it)
    assert len(out) == len(items)
    return out
