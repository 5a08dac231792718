"""The host verifier as the serial executor of the verification plan (no GPU): xfg_verify plans a proof
with plan_proof, walks every batch Merkle opening the way vtree_kernel does and runs the per-query checks
the kernels run. Pinned here: the place of the structural FRI errors in the host's check order, the walk
of the openings against the oracle's on node vectors that do not fit, and the smallest trees."""
import functools

import pytest

import fold_cases as FC
import oracle_lib as O
import proof_mutants as PM
from test_verifier import _flip, _sections


@pytest.fixture(scope="module")
def X():
    import xfgstark
    return xfgstark


@functools.lru_cache(maxsize=None)
def reference_proof(n):
    """(burn inputs, oracle AIR, proof) with the reference options and the base field"""
    return FC.oracle_proof((n, 8, 31, 42, 8, 1))


@pytest.mark.parametrize("case", PM.CHECK_ORDER, ids=PM.check_order_id)
def test_host_reports_structural_errors_at_their_place_in_the_walk(X, case):
    """a FRI section of the wrong size, alone and together with a flipped byte in a section that is
    opened before it: xfg_verify answers with the first failure in the order trace tree, constraint tree,
    per layer (section size, tree, fold), remainder length, remainder commitment, remainder evaluation.
    The texts were recorded from the build before the host verifier became an executor of the plan."""
    n, short, cut, flip, want = case
    kw, air, proof = reference_proof(n)
    bad = PM.doubly_broken(proof, short, cut, flip)
    X.StarkProof.from_bytes(bad)
    v = X.XfgBurnMintVerifier()
    assert v.verify_with_details(proof, X.air_consts(**kw))[:2] == (True, None)
    ok, err, _ = v.verify_with_details(bad, X.air_consts(**kw))
    assert (ok, err) == (False, want)
    assert O.verify(air, bad, O.options()) != 0


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("shape", [(1024, 8, 31, 42, 8), (256, 8, 7, 42, 2)], ids=["n1024-f8", "n256-f2"])
def test_node_vector_mutants_host_equals_oracle(X, shape, ext):
    """the host's serial walk of the batch openings (vtree_kernel's walk: vector j feeds position j, a
    `used` count per vector, nvec == npairs) on node vectors that parse but do not fit: host = oracle =
    the mutant's stated verdict, the appended node is never read (accepted), the untouched proof verifies"""
    case = shape + (ext,)
    kw, air, proof = FC.oracle_proof(case)
    v = X.XfgBurnMintVerifier(proof_options=FC.product_options(X, case))
    xair = X.air_consts(**kw)
    opts = FC.oracle_options(case)
    mutants = PM.node_vector_mutants(proof)
    assert [ok for m, ok in mutants].count(True) == 3  # one appended node per opening
    for m, want in [(proof, True)] + mutants:
        assert v.verify_with_details(m, xair)[0] == want
        assert (O.verify(air, m, opts) == 0) == want
    assert v.batch_verify([(m, xair) for m, ok in mutants], threads=1) == [ok for m, ok in mutants]


@pytest.mark.parametrize("ext", [1, 2])
def test_tree_with_one_opened_leaf(X, ext):
    """one query (the fewest the options admit) at n = 8, blowup 8: every opening is a single leaf with
    one node vector, and no FRI layer stands between the DEEP value and the remainder"""
    case = (8, 8, 31, 1, 8, ext)
    kw, air, proof = FC.oracle_proof(case)
    assert X.StarkProof.from_bytes(proof).num_unique_queries == 1
    v = X.XfgBurnMintVerifier(proof_options=FC.product_options(X, case))
    xair = X.air_consts(**kw)
    assert v.verify_with_details(proof, xair)[:2] == (True, None)
    ok, err, _ = v.verify_with_details(_flip(proof, _sections(proof)["trace_rows"][0] + 3), xair)
    assert (ok, err) == (False, PM.TRACE)
