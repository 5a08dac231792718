"""FRI folding factors 2, 4 and 16 on the CPU: the plain fold reference (tests/fold_ref.py), and the product's
proof parser and host verifier (libxfgstark.so host code, no GPU) on the oracle's proofs with those
factors -- accepted, their size inside xfg_proof_size_bound, tampering answered with the VerifierError
families of the fold-8 tests (tests/test_verifier.py), always the oracle verifier's verdict -- and the
parser + verifier under AddressSanitizer / UBSan through the mutation driver tests/sanitize/fuzz_verify.cpp
(a stand-alone program) with folding arguments 2, 4 and 16."""
import os
import random
import struct
import subprocess

import pytest

import fold_cases as FC
import fold_ref as FR
import oracle_lib as O
import plain_ref as R
from test_verifier import _flip, _sections

P = R.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def X():
    import xfgstark
    return xfgstark


def _rand_e(rng):
    return (rng.randrange(P), rng.randrange(P))


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("F", [2, 4, 16])
@pytest.mark.parametrize("D,beta", [(64, 2), (128, 8), (256, 16), (512, 8)])
def test_fold_reference_divides_the_degree_by_the_factor(D, beta, F, ext):
    """f of degree < D / beta evaluated over 7 <w_D>, folded by F with alpha: the D / F values, read over
    7 <w_(D/F)> (every FRI layer's domain in the product and in Winterfell), interpolate to degree
    < D / (F beta). Exactly: f(x) = sum_j x^j f_j(x^F) folds to g = sum_j alpha^j f_j at x^F = 7^F w_(D/F)^i,
    so over 7 <w_(D/F)> the coefficients are g_k 7^((F - 1) k)."""
    rng = random.Random(D * 10 + beta + ext + 1000 * F)
    d = D // beta
    f = [_rand_e(rng) if ext == 2 else (rng.randrange(P), 0) for _ in range(d)]
    alpha = _rand_e(rng) if ext == 2 else (rng.randrange(P), 0)
    planes = [O.evaluate_lde([c[k] for c in f], beta, R.GEN) for k in range(2)]
    vals = list(zip(*planes))
    layer = FR.fold_layer(vals, D, alpha, F)
    assert len(layer) == D // F
    got = list(zip(*[O.interpolate([v[k] for v in layer], R.GEN) for k in range(2)]))
    want = []
    for k in range(D // F):
        g, apow = (0, 0), (1, 0)
        for j in range(F):
            if F * k + j < d:
                g = R.e_add(g, R.e_mul(apow, f[F * k + j]))
            apow = R.e_mul(apow, alpha)
        want.append(R.e_scale(g, pow(R.GEN, (F - 1) * k, P)))
    assert all(c == (0, 0) for c in got[max(d // F, 1):])
    assert got == want
    if ext == 1:
        assert all(v[1] == 0 for v in layer)


def test_fold_reference_at_eight_is_plain_ref():
    rng = random.Random(8)
    D = 64
    vals = [_rand_e(rng) for _ in range(D)]
    alpha = _rand_e(rng)
    want = R.fold_layer(vals, D, alpha)
    assert FR.fold_layer(vals, D, alpha, 8) == [want[i] for i in range(D // 8)]


def test_fri_tree_reference_at_eight_is_merkle_ref(X):
    import numpy as np
    import merkle_ref as M
    rng = np.random.default_rng(3)
    vals = rng.integers(0, P, size=(2, 2, 256), dtype=np.uint64)
    for cm in (False, True):
        assert np.array_equal(FR.fri_trees(vals, 5, 3, cm, 8, blake3=O.blake3), M.fri_trees(vals, 5, 3, cm))
        # 256-byte leaves: the oracle's BLAKE3 and the library's host BLAKE3 agree, leaf by leaf
        big = rng.integers(0, P, size=(1, 2, 512), dtype=np.uint64)
        assert np.array_equal(FR.fri_trees(big, 6, 3, cm, 16), FR.fri_trees(big, 6, 3, cm, 16, blake3=X.blake3))


# ---------------------------------------------------------------- the host verifier on oracle proofs
@pytest.mark.parametrize("case", FC.CASES, ids=FC.case_id)
def test_verifier_accepts_oracle_proofs_of_every_factor(X, case):
    n, beta, remdeg, q, fold, ext = case
    kw, oair, proof = FC.oracle_proof(case)
    air = X.air_consts(**kw)
    o = FC.product_options(X, case)
    ok, err, _ = X.XfgBurnMintVerifier(proof_options=o).verify_with_details(proof, air)
    assert ok, err
    p = X.StarkProof.from_bytes(proof)
    assert p.options.fri_folding_factor == fold and p.trace_length == n
    assert p.num_fri_layers == FC.num_layers(n, beta, remdeg, fold)[0]
    if case[:4] in FC.FACTOR_2_DEEP:
        assert p.num_fri_layers == 13
    bound = X._lib.xfg_proof_size_bound(n, X.C.byref(o._c()))
    assert bound >= len(proof), (bound, len(proof))
    # the same options with any other factor are not acceptable for this proof
    for other in (2, 4, 8, 16):
        if other != fold:
            o2 = FC.product_options(X, case)
            o2.fri_folding_factor = other
            ok, err, _ = X.XfgBurnMintVerifier(proof_options=o2).verify_with_details(proof, air)
            assert not ok and err == "UnacceptableProofOptions", (other, err)


@pytest.mark.parametrize("fold", [0, 1, 3, 5, 32])
def test_verifier_refuses_factors_outside_the_set(X, fold):
    """a proof whose options byte names another factor, offered with exactly those options as the
    acceptable set: UnacceptableProofOptions (check_options), whatever the rest of the proof holds"""
    case = (64, 8, 31, 42, 2, 1)
    kw, oair, proof = FC.oracle_proof(case)
    b = bytearray(proof)
    meta = struct.unpack_from("<H", proof, 3)[0]
    at = 5 + meta + 1 + 8 + 4  # Context: width, aux, logn, u16 meta, u8 modulus length, modulus, then the options
    assert b[at] == 2 and b[at - 1] == 1 and b[at + 1] == 31
    b[at] = fold
    o = FC.product_options(X, case)
    o.fri_folding_factor = fold
    ok, err, _ = X.XfgBurnMintVerifier(proof_options=o).verify_with_details(bytes(b), X.air_consts(**kw))
    assert not ok and err == "UnacceptableProofOptions"


TAMPER_CASES = [(256, 4, 7, 42, 2, 1), (256, 4, 7, 42, 4, 2), (4096, 8, 31, 42, 16, 1), (1024, 16, 31, 24, 16, 2),
                (8192, 8, 0, 42, 2, 2)]


@pytest.mark.parametrize("case", TAMPER_CASES, ids=FC.case_id)
def test_verifier_rejects_tampering_with_reference_errors(X, case):
    """one flipped bit in every layer's values and paths and in the remainder (both coordinates of an
    element with the extension): the FriVerificationFailed family, as for fold 8; in the other sections:
    their own errors. Every verdict is the oracle verifier's"""
    n, beta, remdeg, q, fold, ext = case
    kw, oair, proof = FC.oracle_proof(case)
    air = X.air_consts(**kw)
    o, oo = FC.product_options(X, case), FC.oracle_options(case)
    v = X.XfgBurnMintVerifier(proof_options=o)
    sec = _sections(proof)
    nl = FC.num_layers(n, beta, remdeg, fold)[0]
    assert nl >= 2 and f"fri_vals{nl - 1}" in sec and f"fri_vals{nl}" not in sec
    row = 8 * fold * ext
    expect = {"trace_rows": "TraceQueryDoesNotMatchCommitment", "constraint_rows": "ConstraintQueryDoesNotMatchCommitment",
              "ood": "InconsistentOodConstraintEvaluations", "hz": "InconsistentOodConstraintEvaluations",
              "remainder": "FriVerificationFailed"}
    places = []
    for name, want in expect.items():
        places += [(name, sec[name][0] + 3, want)]
        if ext == 2 and name != "trace_rows":
            places += [(name, sec[name][0] + 9, want)]  # the second coordinate
    for l in range(nl):
        at, ln = sec[f"fri_vals{l}"]
        assert ln % row == 0 and ln > 0
        places += [(f"fri_vals{l}", at + 3, "FriVerificationFailed"),
                   (f"fri_vals{l}", at + ln - 2, "FriVerificationFailed")]  # first and last value of the layer
        at, ln = sec[f"fri_paths{l}"]
        if ln > 2 + 32:  # u8 vector count, u8 length, then the first vector's digests
            places += [(f"fri_paths{l}", at + 2 + 5, "FriVerificationFailed(LayerCommitmentMismatch)")]
    for name, at, want in places:
        bad = _flip(proof, at)
        ok, err, _ = v.verify_with_details(bad, air)
        assert not ok and err.startswith(want), (name, at, err)
        assert O.verify(oair, bad, oo) != 0, (name, at)
    ok, err, _ = v.verify_with_details(_flip(proof, sec["trace_paths"][0] + 2 + 5), air)
    assert not ok and err == "TraceQueryDoesNotMatchCommitment"
    pub, nf, cm = air
    ok, err, _ = v.verify_with_details(proof, (pub, nf ^ 1, cm))
    assert not ok and err == "InconsistentOodConstraintEvaluations"
    assert v.batch_verify([(proof, air), (_flip(proof, sec["remainder"][0]), air)]) == [True, False]


# ---------------------------------------------------------------- parser + verifier under ASan / UBSan
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")


@pytest.fixture(scope="module")
def fuzz_bin():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "xfg-stark_amd"), "sanitize"], check=True)
    return os.path.join(ROOT, "xfg-stark_amd", "build", "asan", "fuzz_verify")


@pytest.mark.parametrize("case,stride", [((64, 8, 31, 42, 2, 1), 1), ((256, 4, 7, 42, 4, 1), 5),
                                         ((64, 8, 31, 42, 16, 2), 2)], ids=lambda v: FC.case_id(v) if isinstance(v, tuple) else None)
def test_mutated_proofs_rejected_under_asan_ubsan(fuzz_bin, tmp_path, case, stride):
    """the stand-alone mutation driver on oracle proofs with folding argument 2, 4 and 16: the untouched
    proof accepted, every mutant rejected, both sanitizers silent"""
    n, beta, remdeg, q, fold, ext = case
    kw, air, proof = FC.oracle_proof(case)
    pf, af = tmp_path / "proof.bin", tmp_path / "air.bin"
    pf.write_bytes(proof)
    af.write_bytes(struct.pack("<14Q", *air.pub, air.nullifier, air.commitment))
    r = subprocess.run([fuzz_bin, str(pf), str(af), str(q), str(beta), "4", str(ext), str(fold), str(remdeg), str(stride)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("checked ") and r.stdout.rstrip().endswith("accepted 0")
