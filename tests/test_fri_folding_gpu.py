"""GPU: FRI folding factors 2, 4 and 16 through every layer the factor 8 goes through -- the fold kernel
against the Lagrange reference of tests/fold_ref.py, every node of the FRI layer commitment against a tree
built from the leaves up, whole proofs byte for byte against the CPU oracle (single, batched, submitted),
the three verifiers on them, the 13-layer two-fold proofs in the GPU batch verifier, and the refusals."""
import random

import numpy as np
import pytest

import fold_cases as FC
import fold_ref as FR
import oracle_lib as O
import plain_ref as R
from test_verifier import _flip, _sections

pytestmark = pytest.mark.gpu
P = R.P
HI = (1 << 64) - (1 << 32)
EDGE = [0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 1 << 63, (1 << 63) - 1, P - 0xFFFFFFFF]
FACTORS = (2, 4, 16)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _layout(D, beta_log_max, coset_major):
    """(logn, logbeta) with 2^(logn + logbeta) = D: natural layers as the prover stores them (logbeta 0),
    coset-major with the largest blowup up to 2^beta_log_max that leaves n >= 1"""
    logD = D.bit_length() - 1
    logbeta = min(beta_log_max, logD - 1) if coset_major else 0
    return logD - logbeta, logbeta


# ---------------------------------------------------------------- fold kernel
def _fold_set(name, D, F, ext, rng):
    """D E-values in natural order for one fold instance"""
    rows = D // F

    def plane(flip):
        if name == "random":
            return [rng.randrange(P) for _ in range(D)]
        if name == "all_pm1":
            return [P - 1] * D
        if name == "all_hi":  # 2^64 - 2^32, the largest canonical value with a zero low word
            return [HI] * D
        if name == "one_per_row":  # row i holds indices i + k rows
            v = [0] * D
            for i in range(rows):
                v[i + rng.randrange(F) * rows] = rng.choice([1, P - 1, HI, rng.randrange(1, P)])
            return v
        if name == "alternating":  # alternates inside a row (k) and from row to row
            return [P - 1 if (K + K // rows + flip) % 2 == 0 else HI for K in range(D)]
        return [rng.choice(EDGE) for _ in range(D)]
    planes = [plane(0), plane(1) if ext == 2 else [0] * D]
    return list(zip(*planes))


def _run_fold(prover, sets, alphas, logn, logbeta, coset_major, ext, F):
    n, beta = 1 << logn, 1 << logbeta
    stored = [R.to_coset_major(s, n, beta) if coset_major else s for s in sets]
    vals = np.array([[[v[c] for v in s] for c in range(ext)] for s in stored], dtype=np.uint64)
    al = np.array([list(a[:ext]) for a in alphas], dtype=np.uint64)
    out = prover.debug_fri_fold(vals, al, logn, logbeta, coset_major, fold=F)
    assert out.shape == (len(sets), ext, (n * beta) // F)
    return out


@pytest.mark.parametrize("mult,coset_major", [(2, False), (2, True), (64, False), (64, True), (256, True), (512, False),
                                              (512, True)])
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("F", FACTORS)
def test_fri_fold_kernel_matches_reference(prover, F, ext, mult, coset_major):
    """fri_fold_kernel<D, LOGF> (size-F inverse DFT, canonicalisation, Horner in E, the 2^-LOGF scaling)
    against the Lagrange interpolation of fold_ref.fold_row, every row. Shapes: D = 2 F (a two-thread
    block), 64 F, 256 F (one full block), 512 F (two blocks); natural, and coset-major at blowup up to 16.
    Inputs: random, all p - 1, all 2^64 - 2^32, one non-zero value per row, alternating p - 1 /
    2^64 - 2^32, picks from EDGE; each with every alpha: random, 1, p - 1 and with an extension (a, 0),
    (0, b), (p - 1, p - 1); two instances per launch"""
    D = mult * F
    logn, logbeta = _layout(D, 4 if mult > 2 else 1, coset_major)
    rng = random.Random(D * 8 + logbeta * 2 + ext + 100003 * F)
    if ext == 2:
        alphas = [(rng.randrange(P), rng.randrange(P)), (1, 0), (P - 1, 0), (rng.randrange(P), 0),
                  (0, rng.randrange(1, P)), (P - 1, P - 1)]
    else:
        alphas = [(rng.randrange(P), 0), (1, 0), (P - 1, 0), (rng.choice(EDGE[4:]), 0)]
    for name in ["random", "all_pm1", "all_hi", "one_per_row", "alternating", "edge"]:
        for k in range(0, len(alphas), 2):
            sets = [_fold_set(name, D, F, ext, rng) for _ in range(2)]
            out = _run_fold(prover, sets, alphas[k:k + 2], logn, logbeta, coset_major, ext, F)
            for b in range(2):
                want = FR.fold_layer(sets[b], D, alphas[k + b], F)
                got = [(int(out[b, 0, i]), int(out[b, 1, i]) if ext == 2 else 0) for i in range(D // F)]
                bad = [i for i in range(D // F) if got[i] != want[i]]
                assert not bad, (name, alphas[k + b], bad[:8], [(got[i], want[i]) for i in bad[:2]])


@pytest.mark.parametrize("ext", [1, 2])
def test_fold_eight_through_the_new_entries_is_the_old_entries(prover, ext):
    """xfg_debug_fri_fold_f / xfg_debug_merkle_fri_f with fold = 8 (what the Python wrappers call) give
    what xfg_debug_fri_fold / xfg_debug_merkle_fri give"""
    import xfgstark as X
    C, u64p, u8p = X.C, X._u64p, X._u8p
    rng = np.random.default_rng(80 + ext)
    for logn, logbeta, cm in [(4, 0, False), (9, 3, True)]:
        D = 1 << (logn + logbeta)
        vals = rng.integers(0, P, size=(2, ext, D), dtype=np.uint64)
        al = rng.integers(0, P, size=(2, ext), dtype=np.uint64)
        new = prover.debug_fri_fold(vals, al, logn, logbeta, cm, fold=8)
        old = np.zeros_like(new)
        st = X._lib.xfg_debug_fri_fold(prover._ctx, 2, ext, logn, logbeta, int(cm), vals.ctypes.data_as(u64p),
                                       al.ctypes.data_as(u64p), old.ctypes.data_as(u64p))
        assert st == 0 and np.array_equal(new, old)
        assert np.array_equal(new, prover.debug_fri_fold(vals, al, logn, logbeta, cm))
        tnew = prover.debug_merkle_fri(vals, logn, logbeta, cm, fold=8)
        told = np.zeros_like(tnew)
        st = X._lib.xfg_debug_merkle_fri(prover._ctx, 2, ext, logn, logbeta, int(cm), vals.ctypes.data_as(u64p),
                                         told.ctypes.data_as(u8p))
        assert st == 0 and np.array_equal(tnew, told)


# ---------------------------------------------------------------- FRI layer commitment
def _field_values(shape, seed):
    """canonical elements, different for every proof (leading axis), with 0 and p - 1 among them"""
    v = np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)
    flat = v.reshape(shape[0], -1)
    flat[:, 0] = 0
    flat[:, 1] = P - 1
    flat[:, -1] = P - 1
    flat[:, -2] = 0
    return v


# (count, ext, rows, coset_major); the 4096-row ones reach the levels between the leaf kernel and the top
# block: four lanes per parent for a lone tree, one lane for 128 trees
TREE_SHAPES = [(3, ext, rows, cm) for ext in (1, 2) for rows in (2, 32, 512, 2048) for cm in (False, True)]
TREE_SHAPES += [(1, 2, 4096, False), (128, 1, 4096, False)]


@pytest.mark.parametrize("count,ext,rows,coset_major", TREE_SHAPES)
@pytest.mark.parametrize("F", FACTORS)
def test_fri_commitment_every_node(prover, F, count, ext, rows, coset_major):
    """fri_leaves_kernel<D, LOGF> and the levels above it: every node of the heap against fold_ref.fri_trees
    (leaves of 16 to 256 bytes)"""
    D = rows * F
    logn, logbeta = _layout(D, 3, coset_major)
    vals = _field_values((count, ext, D), seed=D * 10 + ext * 2 + int(coset_major) + 1000 * F)
    nodes = prover.debug_merkle_fri(vals, logn, logbeta, coset_major, fold=F)
    assert nodes.shape == (count, 2 * rows, 8)
    want = FR.fri_trees(vals, logn, logbeta, coset_major, F)
    for b in range(count):
        bad = np.flatnonzero((nodes[b, 1:] != want[b, 1:]).any(axis=1)) + 1
        assert bad.size == 0, f"proof {b}: {bad.size} of {2 * rows - 1} nodes differ, first at heap slot {bad[0]}"


# ---------------------------------------------------------------- whole proofs
def _use(prover, case):
    import xfgstark
    o = FC.product_options(xfgstark, case)
    prover._options = o
    return o


@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_proof_bytes_match_oracle_and_verify(prover, case):
    """prove_burn_mint under every (shape, factor, field) == the oracle's proof, which xfg_verify, the GPU
    batch verifier and the oracle verifier accept"""
    import xfgstark
    kw, oair, want = FC.oracle_proof(case)
    o = _use(prover, case)
    got = prover.prove_burn_mint(**kw, trace_length=case[0]).to_bytes()
    assert got == want
    assert len(got) <= prover.proof_size_bound(case[0])
    air = xfgstark.air_consts(**kw)
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    ok, err, _ = v.verify_with_details(got, air)
    assert ok, err
    assert v.batch_verify([(got, air)], gpu=prover) == [True]
    assert O.verify(oair, got, FC.oracle_options(case)) == 0


@pytest.mark.parametrize("case", [(1024, 16, 31, 24, 16, 2), (1024, 8, 0, 42, 2, 1)], ids=FC.case_id)
def test_batches_match_oracle_per_proof(prover, case):
    """prove_batch (6 inputs) and a submitted batch collected later, under factors 16 and 2"""
    import synthetic
    n = case[0]
    _use(prover, case)
    opts = FC.oracle_options(case)
    inputs = [synthetic.burn_inputs(7100 + 10 * case[4] + i) for i in range(6)]
    want = []
    for kw in inputs:
        st, pr = O.prove(FC.oracle_air(kw), n, opts)
        assert st == 0
        want.append(pr)
    pending = prover.submit_batch(inputs[::-1], trace_length=n)
    assert [p.to_bytes() for p in prover.prove_batch(inputs, trace_length=n)] == want
    assert [p.to_bytes() for p in pending.result()] == want[::-1]


@pytest.mark.parametrize("case", [s + (2, ext) for s in FC.FACTOR_2_DEEP for ext in (1, 2)], ids=FC.case_id)
def test_gpu_batch_verifier_on_thirteen_layers(prover, case):
    """a two-fold proof of 13 FRI layers (past the 12 the 32-bit flag word held): the GPU batch verifier's
    results are the host verifier's on the valid proof and on one tampered value in layer 0, in layer 12
    and in the remainder, and on a tampered digest of the paths of layers 0 and 6"""
    import xfgstark
    kw, oair, proof = FC.oracle_proof(case)
    o = FC.product_options(xfgstark, case)
    air = xfgstark.air_consts(**kw)
    sec = _sections(proof)
    assert "fri_vals12" in sec and "fri_vals13" not in sec
    items = [(proof, air)]
    for name, off in [("fri_vals0", 3), ("fri_vals12", 3), ("fri_vals12", sec["fri_vals12"][1] - 2), ("remainder", 3),
                      ("fri_paths0", 2 + 5), ("fri_paths6", 2 + 5)]:
        assert sec[name][1] > off
        items.append((_flip(proof, sec[name][0] + off), air))
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    host = v.batch_verify(items)
    assert host == [True] + [False] * (len(items) - 1)
    assert v.batch_verify(items, gpu=prover) == host


# ---------------------------------------------------------------- refusals
def test_factors_outside_the_set_are_refused(prover):
    import xfgstark
    kw = FC.inputs((64, 8, 31, 42, 2, 1))
    for fold in (0, 1, 3, 32):
        o = xfgstark.ProofOptions.reference()
        o.fri_folding_factor = fold
        prover._options = o
        with pytest.raises(xfgstark.XfgStarkError, match="2, 4, 8 or 16") as e:
            prover.prove_burn_mint(**kw, trace_length=64)
        assert e.value.status == 6
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.submit_batch([kw], trace_length=64)
        assert e.value.status == 6


@pytest.mark.parametrize("n,beta,remdeg,fold,last", [(8, 2, 0, 4, 1), (1024, 8, 0, 16, 2)])
def test_a_last_layer_below_the_blowup_is_refused(prover, n, beta, remdeg, fold, last):
    """the product's own rule (D[nl] < blowup: the remainder would have no coefficient); the oracle is not
    asked about such shapes. The message names the sizes"""
    import xfgstark
    assert FC.num_layers(n, beta, remdeg, fold)[1] == last < beta
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.fri_remainder_max_degree, o.fri_folding_factor, o.num_queries = beta, remdeg, fold, 7
    prover._options = o
    kw = FC.inputs((n, beta, remdeg, 7, fold, 1))
    with pytest.raises(xfgstark.XfgStarkError, match=f"last FRI layer of {last}, smaller than the blowup factor {beta}") as e:
        prover.prove_burn_mint(**kw, trace_length=n)
    assert e.value.status == 6
    with pytest.raises(xfgstark.XfgStarkError) as e:
        prover.prove_batch([kw], trace_length=n)
    assert e.value.status == 6


def test_debug_entries_refuse_other_factors_and_short_layers(prover):
    import xfgstark
    al = np.zeros((1, 1), dtype=np.uint64)
    for fold, logD in [(3, 6), (0, 6), (32, 8), (2, 1), (4, 2), (16, 4)]:  # not a factor; D = fold < 2 fold
        vals = np.zeros((1, 1, 1 << logD), dtype=np.uint64)
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.debug_fri_fold(vals, al, logD, 0, False, fold=fold)
        assert e.value.status == 9
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.debug_merkle_fri(vals, logD, 0, False, fold=fold)
        assert e.value.status == 9
    for fold, logD in [(2, 2), (4, 3), (16, 5)]:  # D = 2 fold is served
        vals = np.zeros((1, 1, 1 << logD), dtype=np.uint64)
        assert prover.debug_fri_fold(vals, al, logD, 0, False, fold=fold).shape == (1, 1, 2)
        assert prover.debug_merkle_fri(vals, logD, 0, False, fold=fold).shape == (1, 4, 8)
    with pytest.raises(xfgstark.XfgStarkError, match="canonical") as e:
        prover.debug_fri_fold(np.full((1, 1, 32), P, dtype=np.uint64), al, 5, 0, False, fold=16)
    assert e.value.status == 9


# ---------------------------------------------------------------- arbitrary traces
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("F", FACTORS)
def test_prove_arbitrary_trace_bytes_match_oracle(prover, F, ext):
    """a proof of a FALSE statement (uniformly random trace cells) per factor and field: the GPU proof is
    the oracle's byte for byte, and the oracle verifier, the host verifier and the GPU batch verifier reject it"""
    import xfgstark
    n, blowup = 256, 8
    tr, air = R.make_trace("random", n, 7700 + 10 * F + ext)
    oa = O.Air()
    for i in range(12):
        oa.pub[i] = air[0][i]
    oa.secret, oa.nullifier, oa.commitment = 0, air[1], air[2]
    flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr for v in col])
    opts = O.options(blowup=blowup, field_extension=ext, fri_folding=F)
    st, want = O.prove(oa, n, opts, trace=flat)
    assert st == 0
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension, o.fri_folding_factor = blowup, ext, F
    prover._options = o
    got = prover.prove_trace(np.array(tr, dtype=np.uint64), air[0], air[1], air[2]).to_bytes()
    assert got == want
    assert O.verify(oa, got, opts) != 0
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    assert v.batch_verify([(got, air)]) == [False]
    assert v.batch_verify([(got, air)], gpu=prover) == [False]
