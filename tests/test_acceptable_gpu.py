"""GPU: one xfg_verify_batch_gpu_acceptable call on proofs of mixed options. The batch's query records lie in
four ranges, one per folding factor, and vfield_kernel<LOGF> runs once per non-empty range, so what must hold
is that every item still gets its own verdict, flag word and error text -- the host verifier's under the same
policy -- whatever the mix, the order, and whichever ranges are empty. The oracle makes every proof
(verifier_faults.proofs, fold_cases.oracle_proof); a case is (n, blowup, remainder max degree, queries, fold, ext)."""
import ctypes as C

import pytest

import fold_cases as FC
import verifier_faults as VF
from test_acceptable_cpu import bad_policies, level, options_tuple

pytestmark = pytest.mark.gpu

# all four folding factors and a proof without a FRI layer, both extensions
SHAPES = [(64, 8, 31, 42, 8), (1024, 16, 31, 24, 16), (256, 4, 7, 42, 4), (256, 8, 7, 42, 2), (8, 8, 7, 7, 8)]
CASES = [s + (ext,) for s in SHAPES for ext in (1, 2)]
assert set(CASES) <= set(VF.CASES)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def X():
    import xfgstark
    return xfgstark


def set_verifier(X, cases):
    return X.XfgBurnMintVerifier(acceptable=X.AcceptableOptions.option_set([FC.product_options(X, c) for c in cases]))


def singly(v, items, prover):
    """every item in a call of its own: [(accepted, flag word, error text)]"""
    return [v.debug_batch_verify([it], prover)[0] for it in items]


@pytest.fixture(scope="module")
def mixed(X, prover):
    """the forged and honest proofs of every case, merged round-robin across the cases, and what one debug call
    under the set of the ten option sets answers: (verifier, [(case, faults, prover status)], items, results)"""
    seqs = [[(case,) + it for it in VF.interleaved(case)] for case in CASES]
    merged = [seq[i] for i in range(max(map(len, seqs))) for seq in seqs if i < len(seq)]
    meta = [(case, faults, st) for case, k, kw, air, faults, st, proof in merged]
    items = [(proof, X.air_consts(**kw)) for case, k, kw, air, faults, st, proof in merged]
    v = set_verifier(X, CASES)
    return v, meta, items, v.debug_batch_verify(items, prover)


def test_mixed_forgeries_in_one_call(X, prover, mixed):
    """per item the verdict, flag word and text of verifier_faults.expected, which are the host verifier's under
    the same policy; never a commitment bit; every folding factor has a forged proof with a non-zero flag word"""
    v, meta, items, got = mixed
    assert len(got) == len(items) == sum(len(VF.proofs(c)) for c in CASES)
    assert [c for c, f, st in meta[:len(CASES)]] == CASES  # round-robin: neighbours have different options
    flagged = set()
    for (case, faults, st), item, (ok, flags, err) in zip(meta, items, got):
        assert st == 0  # the oracle's prover made every proof
        want_err, want_flags = VF.expected(case, faults)
        host_ok, host_err, _ = v.verify_with_details(*item)
        assert (host_ok, host_err) == (want_err is None, want_err), (case, faults)
        assert (ok, err) == (host_ok, host_err), (case, faults)
        assert flags & VF.COMMITMENT_BITS == 0, (case, faults, hex(flags))
        assert flags == want_flags, (case, faults, hex(flags), hex(want_flags))
        if faults and flags:
            flagged.add(case[4])
    assert [ok for ok, flags, err in got].count(True) == VF.STATEMENTS * len(CASES)
    assert flagged == {2, 4, 8, 16}
    assert v.batch_verify(items, gpu=prover) == [ok for ok, flags, err in got]


def test_order_of_the_batch(prover, mixed):
    """the same batch reversed: results, flags and texts come back reversed"""
    v, meta, items, got = mixed
    assert v.debug_batch_verify(items[::-1], prover) == got[::-1]
    assert len(set(got)) > 4  # the answers differ, so an order would show


def pick(X, case, want_forged=2):
    """a few items of a case: its honest proofs and the first forged ones whose fault the device sees"""
    out = []
    for k, kw, air, faults, st, proof in VF.proofs(case):
        forged = bool(faults) and VF.expected(case, faults)[1] != 0
        if not faults or (forged and want_forged > 0):
            out.append((proof, X.air_consts(**kw)))
            want_forged -= forged
    return out


def test_empty_middle_ranges(X, prover):
    """only the factors 2 and 16: the ranges of 4 and 8 are empty"""
    cases = [(256, 8, 7, 42, 2, 1), (1024, 16, 31, 24, 16, 2), (256, 8, 7, 42, 2, 2), (1024, 16, 31, 24, 16, 1)]
    groups = [pick(X, c) for c in cases]
    items = [g[i] for i in range(max(map(len, groups))) for g in groups if i < len(g)]
    v = set_verifier(X, CASES)
    got = v.debug_batch_verify(items, prover)
    assert got == singly(v, items, prover)
    assert sum(1 for ok, flags, err in got if flags) == 2 * len(cases) and [g[0] for g in got].count(True) == 3 * len(cases)


def test_only_the_last_range(X, prover):
    """only factor 16: the first three ranges are empty"""
    items = pick(X, (1024, 16, 31, 24, 16, 1)) + pick(X, (1024, 16, 31, 24, 16, 2))
    v = set_verifier(X, CASES)
    got = v.debug_batch_verify(items, prover)
    assert got == singly(v, items, prover)
    assert sum(1 for ok, flags, err in got if flags) == 4 and [g[0] for g in got].count(True) == 6


@pytest.mark.parametrize("fold,ext", [(4, 1), (4, 2), (16, 2)])
def test_range_of_a_single_query(X, prover, fold, ext):
    """one factor's whole range is the one query of a one-query proof, between 42-query proofs of two other
    factors whose ranges are more than one 64-thread block and no multiple of 64"""
    one = (8, 8, 31, 1, fold, ext)
    kw, air, proof = FC.oracle_proof(one)
    assert X.StarkProof.from_bytes(proof).num_unique_queries == 1
    before, after = pick(X, (256, 8, 7, 42, 2, ext)), pick(X, (64, 8, 31, 42, 8, 3 - ext))
    for group in (before, after):
        nq = sum(X.StarkProof.from_bytes(p).num_unique_queries for p, a in group)
        assert nq > 64 and nq % 64 != 0, nq
    items = before + [(proof, X.air_consts(**kw))] + after
    v = set_verifier(X, CASES + [one])
    got = v.debug_batch_verify(items, prover)
    assert got == singly(v, items, prover)
    assert got[len(before)] == (True, 0, None)
    assert sum(1 for ok, flags, err in got if flags) == 4
    # the one-query proof with its remainder's constant term changed: its single thread must see it
    bad = bytearray(proof)
    from test_verifier import _sections
    bad[_sections(proof)["remainder"][0]] ^= 1
    items[len(before)] = (bytes(bad), items[len(before)][1])
    got2 = v.debug_batch_verify(items, prover)
    assert got2[:len(before)] + got2[len(before) + 1:] == got[:len(before)] + got[len(before) + 1:]
    assert got2[len(before)] == singly(v, [items[len(before)]], prover)[0]
    assert got2[len(before)][0] is False and got2[len(before)][1] == VF.BIT_REMAINDER


def test_unplanned_proofs_between_factors(X, prover):
    """two proofs that never reach the device -- one verified against another statement's AIR constants, one
    whose options are outside the set -- between planned proofs of different factors: their flag words are 0
    and their neighbours' answers are what they are alone"""
    f2, f16 = pick(X, (256, 8, 7, 42, 2, 1)), pick(X, (1024, 16, 31, 24, 16, 2))
    f4 = pick(X, (256, 4, 7, 42, 4, 2))
    wrong_air = (f4[0][0], f4[1][1])  # statement 0's proof, statement 1's constants
    assert f4[0][1] != f4[1][1]
    outside = pick(X, (64, 8, 31, 42, 8, 1))[0]
    in_set = [c for c in CASES if c[4] != 8]
    items = f2[:2] + [wrong_air] + f16[-2:] + [outside] + f4 + [outside, wrong_air] + f2[2:]
    v = set_verifier(X, in_set)
    got = v.debug_batch_verify(items, prover)
    assert got == singly(v, items, prover)
    for i, it in enumerate(items):
        if it is wrong_air:
            assert got[i] == (False, 0, VF.OOD)
        if it is outside:
            assert got[i] == (False, 0, "UnacceptableProofOptions")
    assert sum(1 for ok, flags, err in got if flags) >= 4
    assert v.batch_verify(items, gpu=prover) == [g[0] for g in got]
    # nothing planned at all: every range empty, nothing launched
    assert v.debug_batch_verify([outside, wrong_air, outside], prover) == [got[5], got[2], got[5]]


def test_minimum_security_on_the_gpu(X, prover):
    """the honest proofs of every case under a minimum of 99 bits, which the (1024, 16, ..., 24 queries) proofs
    meet in the quadratic extension (99) and miss in the base field (49): verdicts and texts are the host's"""
    v = X.XfgBurnMintVerifier(acceptable=X.AcceptableOptions.min_conjectured_security(99))
    items, want = [], []
    for k in range(VF.STATEMENTS):
        for case in CASES:
            kk, kw, air, faults, st, proof = VF.proofs(case)[k]
            assert kk == k and not faults
            items.append((proof, X.air_consts(**kw)))
            lvl = level(case[0], options_tuple(FC.product_options(X, case)))
            want.append((True, 0, None) if lvl >= 99 else (False, 0, f"InsufficientConjecturedSecurity(99, {lvl})"))
    assert want[CASES.index((1024, 16, 31, 24, 16, 2))][0] and not want[CASES.index((1024, 16, 31, 24, 16, 1))][0]
    got = v.debug_batch_verify(items, prover)
    assert got == want
    assert [(ok, err) for ok, flags, err in got] == [v.verify_with_details(*it)[:2] for it in items]
    assert v.batch_verify(items, gpu=prover) == [w[0] for w in want]


def test_gpu_entries_refuse_bad_policies(X, prover):
    """XFG_INVALID_ARGUMENT, results untouched, and the context still verifies afterwards"""
    lib = X._lib
    v = set_verifier(X, CASES)
    items = pick(X, (64, 8, 31, 42, 8, 1))[:1]
    keep, ptrs, lens, airs, res = v._batch_args(items)
    flags, errs = (C.c_uint64 * 1)(), C.create_string_buffer(256)
    policies, keep2 = bad_policies(X)
    for what, p in policies:
        res[0] = -5
        assert lib.xfg_verify_batch_gpu_acceptable(prover._ctx, 1, ptrs, lens, airs, p, res) == 9, what
        assert lib.xfg_debug_verify_batch_gpu_acceptable(prover._ctx, 1, ptrs, lens, airs, p, res, flags, errs, 256) == 9, what
        assert res[0] == -5, what
    assert v.debug_batch_verify(items, prover) == [(True, 0, None)]
