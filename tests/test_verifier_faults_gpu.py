"""GPU: what the batch verifier's kernels decide on forged proofs that commit consistently
(tests/verifier_faults.py; the oracle makes every proof). vfield_kernel's bits -- layer l folding, remainder
folding -- otherwise only ever show together with a commitment bit of vtree_kernel, which is reported
first; here each must stand alone, and the verdict and error text must be the host verifier's."""
import pytest

import fold_cases as FC
import verifier_faults as VF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


@pytest.mark.parametrize("case", VF.CASES, ids=VF.case_id)
def test_device_flags_on_forged_proofs(prover, case):
    """one xfg_debug_verify_batch_gpu call on the honest proofs of three statements interleaved with every
    forged proof of the case (several blocks of vfield_kernel, a flag word per proof): per item the verdict
    and the error text of xfg_verify, and exactly the flag bits of the check that can see the fault -- bit l
    for layer l (bit 0: the DEEP value against layer 0), bit 63 for the remainder, both for the double fault
    (the device checks every layer, the host stops at the first), never a commitment bit (32..62), 0 for the
    honest proofs and for a proof rejected while the transcript is replayed. The public entry agrees."""
    import xfgstark
    v = xfgstark.XfgBurnMintVerifier(proof_options=FC.product_options(xfgstark, case))
    seq = VF.interleaved(case)
    items = [(proof, xfgstark.air_consts(**kw)) for k, kw, air, faults, st, proof in seq]
    assert all(st == 0 for k, kw, air, faults, st, proof in seq)
    got = v.debug_batch_verify(items, prover)
    assert len(got) == len(items)
    for (k, kw, air, faults, st, proof), item, (ok, flags, err) in zip(seq, items, got):
        want_err, want_flags = VF.expected(case, faults)
        host_ok, host_err, _ = v.verify_with_details(*item)
        assert (host_ok, host_err) == (want_err is None, want_err), faults
        assert (ok, err) == (host_ok, host_err), faults
        assert flags & VF.COMMITMENT_BITS == 0, (faults, hex(flags))
        assert flags == want_flags, (faults, hex(flags), hex(want_flags))
    assert v.batch_verify(items, gpu=prover) == [ok for ok, flags, err in got]
    assert [ok for ok, flags, err in got].count(True) == VF.STATEMENTS
