"""The algebraic checks of the oracle verifier and the host verifier, one at a time (no GPU): forged
proofs of tests/verifier_faults.py, whose single injected error is committed consistently, so that every
commitment check passes and exactly one of the DEEP value, a FRI layer's fold or the remainder evaluation
can reject them. A byte flip in a finished proof never gets that far: a Merkle or transcript check fires
first."""
import pytest

import oracle_lib as O
import verifier_faults as VF
import fold_cases as FC


@pytest.fixture(scope="module")
def X():
    import xfgstark
    return xfgstark


@pytest.mark.parametrize("case", VF.CASES, ids=VF.case_id)
def test_no_fault_is_the_honest_prover(case):
    """orc_prove is the nfaults == 0 call of the fault entry: the same bytes, which orc_verify accepts"""
    opts = FC.oracle_options(case)
    for k, kw, air, faults, st, proof in VF.proofs(case)[:VF.STATEMENTS]:
        assert faults == [] and st == 0
        assert (0, proof) == O.prove(air, case[0], opts)
        assert O.verify(air, proof, opts) == 0


def test_fault_entry_refuses_bad_requests():
    """indices out of range, a zero or non-canonical delta, an unknown kind, more than 4 faults"""
    for case in [(256, 8, 7, 42, 2, 1), (256, 8, 7, 42, 2, 2), (8, 8, 7, 7, 8, 1)]:
        n, nl, rl = case[0], VF.layers(case), VF.remainder_len(case)
        opts, air = FC.oracle_options(case), FC.oracle_air(VF.statement_inputs(case, 0))
        bad = [[(O.FAULT_OOD_NEXT, 7, (1, 0))], [(O.FAULT_DEEP_COEF, n - 1, (1, 0))], [(O.FAULT_LAYER, 0, (1, 0))],
               [(O.FAULT_LAYER, nl, (1, 0))], [(O.FAULT_LAYER, nl + 1, (1, 0))], [(O.FAULT_REMAINDER, rl, (1, 0))],
               [(O.FAULT_OOD_NEXT, 0, (0, 0))], [(O.FAULT_OOD_NEXT, 0, (VF.P, 0))], [(0, 0, (1, 0))], [(5, 0, (1, 0))],
               [(O.FAULT_REMAINDER, 0, (1, 0))] * 5]
        if case[5] == 1:
            bad.append([(O.FAULT_OOD_NEXT, 0, (0, 1))])  # base field: delta[1] is ignored, so this is a zero delta
        for fl in bad:
            assert O.prove_faulty(air, n, opts, fl) == (6, None), (case, fl)


@pytest.mark.parametrize("case", VF.CASES, ids=VF.case_id)
def test_forged_proofs_rejected_by_the_one_check_left(X, case):
    """every forged proof: prover status 0, other bytes than the honest proof of its statement, structurally
    a proof (from_bytes / to_bytes), rejected by orc_verify, and rejected by xfg_verify with exactly the
    error of the one algebraic check that can see the fault -- the host checks each layer's commitment
    before that layer's fold, so the exact folding errors also say that every commitment up to there
    verified; the honest proofs are accepted next to them by both batch entries"""
    opts = FC.oracle_options(case)
    v = X.XfgBurnMintVerifier(proof_options=FC.product_options(X, case))
    seq = VF.interleaved(case)
    honest = {k: proof for k, kw, air, faults, st, proof in seq if not faults}
    assert len(honest) == VF.STATEMENTS and len(seq) > VF.STATEMENTS
    items, want = [], []
    for k, kw, air, faults, st, proof in seq:
        assert st == 0, faults
        xair = X.air_consts(**kw)
        err, _ = VF.expected(case, faults)
        ok, got, size = v.verify_with_details(proof, xair)
        assert (ok, got, size) == (err is None, err, len(proof)), (faults, got)
        assert (O.verify(air, proof, opts) == 0) == (err is None), faults
        if faults:
            assert proof != honest[k], faults
            assert X.StarkProof.from_bytes(proof).to_bytes() == proof
        items.append((proof, xair))
        want.append(err is None)
    assert v.batch_verify(items) == want
    assert v.batch_verify(items, threads=1) == want
