"""GPU: blowup factors 32, 64 and 128. The composed LDE (g = blowup / 16 blowup-16 transforms on twisted
coefficients, csrc/ntt_plan.hpp lde_plan) against the oracle at every point, the constraint hook, whole proofs
against the oracle's bytes with the three verifiers' verdicts (the Merkle kernels' new instantiations are
covered through these: at n = 8 the 255 queries open every row), the batch paths, digests of sizes the oracle
is not run at here, the GPU verifier on tampered proofs, and the refusals."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fold_cases as FC
import oracle_lib as O
import plain_ref as R
import synthetic
import trace_check_ref as T
import verifier_faults as VF
import wide_blowup_cases as W
from test_gpu_parity import _KINDS, _ce_coeffs, _run_constraint_eval
from test_verifier import _flip, _sections

pytestmark = pytest.mark.gpu
P = R.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "wide_blowup_proofs.json")


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _status_of(call):
    import xfgstark
    with pytest.raises(xfgstark.XfgStarkError) as e:
        call()
    return e.value.status, str(e.value)


# ---------------------------------------------------------------- the LDE hook
def _three_polys(n, seed):
    """random values; every coefficient p - 1; one non-zero coefficient at j = n - 1 (the twist's highest power)"""
    rng = np.random.default_rng(seed)
    coef = np.zeros((3, n), dtype=np.uint64)
    coef[0] = rng.integers(0, P, size=n, dtype=np.uint64)
    coef[1] = P - 1
    coef[2, n - 1] = rng.integers(1, P, dtype=np.uint64)
    return coef


@pytest.mark.parametrize("n", [8, 64, 512, 4096])
@pytest.mark.parametrize("blowup", W.WIDE)
def test_lde_matches_oracle_at_every_point(prover, blowup, n):
    """R x C splits 2 x 4, 8 x 8, 16 x 32 and 64 x 64; natural order out, whatever the planes' placement"""
    coef = _three_polys(n, 17 * n + blowup)
    got = np.asarray(prover.debug_lde(coef, n, blowup))
    assert got.shape == (3, n * blowup)
    for p in range(3):
        assert np.array_equal(got[p], O.evaluate_lde_np(coef[p], blowup, 7)), p


def test_lde_2p16_blowup32_matches_oracle(prover):
    n = 1 << 16
    coef = _three_polys(n, 1632)
    got = np.asarray(prover.debug_lde(coef, n, 32))
    for p in range(3):
        assert np.array_equal(got[p], O.evaluate_lde_np(coef[p], 32, 7)), p


def test_lde_2p16_blowup32_all_coset_route(prover):
    """32 polynomials make the 512 all-coset blocks at which the tabled 2^16 sub-transforms take ntt_pass_a_cos2
    + ntt_pass_b_tq, the benchmark's route, here with the composed plane stride. The 32 are the three
    polynomials of the test above in turn: three oracle runs, every plane of every polynomial compared"""
    n = 1 << 16
    three = _three_polys(n, 1632)
    got = np.asarray(prover.debug_lde(three[np.arange(32) % 3], n, 32))
    want = [O.evaluate_lde_np(three[p], 32, 7) for p in range(3)]
    for k in range(32):
        assert np.array_equal(got[k], want[k % 3]), k


def test_lde_2p19_blowup32_pass_tables_only(prover):
    """2^24 points: each blowup-16 sub-transform is past the four-step tables (pass tables alone)"""
    n = 1 << 19
    rng = np.random.default_rng(n + 32)
    coef = rng.integers(0, P, size=(1, n), dtype=np.uint64)
    got = np.asarray(prover.debug_lde(coef, n, 32))[0]
    assert np.array_equal(got, O.evaluate_lde_np(coef[0], 32, 7))


@pytest.mark.parametrize("n,blowup", [(64, 64), (4096, 32)])
def test_lde_skip_fills_flagged_planes_only(prover, n, blowup):
    """flags 1 0 1: the flagged polynomials take no transform and every one of their beta planes holds their
    first coefficient (launch_const_fill writes all of them); the other is bit-equal to the unflagged call"""
    coef = _three_polys(n, 5 * n + blowup)
    coef[2, 0] = P - 2
    plain = np.asarray(prover.debug_lde(coef, n, blowup))
    got = np.asarray(prover.debug_lde_skip(coef, n, blowup, [1, 0, 1]))
    assert np.array_equal(got[1], plain[1])
    assert np.all(got[0] == coef[0, 0]) and np.all(got[2] == P - 2)


# ---------------------------------------------------------------- the constraint hook
@pytest.mark.parametrize("n,blowup", [(8, 32), (64, 128)])
@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_eval_reads_cosets_0_and_half(prover, ext, n, blowup):
    """constraint_eval_kernel reads cosets 0 and beta / 2 of the composed trace LDE: every point of the CE
    domain against plain_ref.constraint_evals, two instances, three coefficient styles"""
    import random
    rng = random.Random(n * 64 + blowup * 4 + ext)
    for call, style in enumerate(["random", "edge", "zeros"]):
        made = [R.make_trace(_KINDS[(call + b) % 3], n, rng.randrange(1 << 30)) for b in range(2)]
        traces, airs = [m[0] for m in made], [m[1] for m in made]
        coeffs = [_ce_coeffs(style, ext, rng) for _ in range(2)]
        got = _run_constraint_eval(prover, traces, airs, coeffs, blowup, ext)
        for b in range(2):
            want = R.constraint_evals(traces[b], airs[b], coeffs[b])
            bad = [i for i in range(2 * n) if got[b][i] != want[i]]
            assert not bad, (style, b, bad[:8])


# ---------------------------------------------------------------- whole proofs
@pytest.mark.parametrize("case", W.PROOF_CASES, ids=W.case_id)
def test_proofs_equal_oracle_bytes_and_verdicts(prover, case):
    """prove_burn_mint on a true statement and prove_trace on a uniformly random trace (a false one): both byte
    for byte the oracle's; the true one accepted, the false one rejected by xfg_verify, xfg_verify_batch_gpu
    and the oracle verifier"""
    import xfgstark
    n, beta, remdeg, q, fold, ext = case
    o, oo = FC.product_options(xfgstark, case), FC.oracle_options(case)
    prover._options = o
    try:
        kw, oair, want = FC.oracle_proof(case)
        got = prover.prove_burn_mint(**kw, trace_length=n).to_bytes()
        assert got == want
        assert len(got) <= prover.proof_size_bound(n)
        air = xfgstark.air_consts(**kw)
        v = xfgstark.XfgBurnMintVerifier(proof_options=o)
        assert v.verify_with_details(got, air)[:2] == (True, None)
        assert v.batch_verify([(got, air)]) == [True]
        assert v.batch_verify([(got, air)], gpu=prover) == [True]
        assert O.verify(oair, got, oo) == 0
        tr, fair, foa, fwant = W.false_proof(case)
        fgot = prover.prove_trace(tr, fair[0], fair[1], fair[2]).to_bytes()
        assert fgot == fwant
        assert not v.verify_with_details(fgot, fair)[0]
        assert v.batch_verify([(fgot, fair)]) == [False]
        assert v.batch_verify([(fgot, fair)], gpu=prover) == [False]
        assert O.verify(foa, fgot, oo) != 0
    finally:
        prover._options = xfgstark.ProofOptions.reference()


# ---------------------------------------------------------------- batch paths at (64, 64)
BATCH_CASE = (64, 64, 31, 21, 8, 1)
BATCH = 70


def _batch_inputs():
    return [synthetic.burn_inputs(7300 + i) for i in range(BATCH)]


@functools.lru_cache(maxsize=None)
def _oracle_batch():
    oo = FC.oracle_options(BATCH_CASE)
    out = []
    for kw in _batch_inputs():
        st, want = O.prove(FC.oracle_air(kw), 64, oo)
        assert st == 0
        out.append(want)
    return out


def test_two_batches_in_flight_equal_oracle(prover):
    """70 inputs as two submissions in flight together (units of 32 * 16 / 64 = 8 proofs, ragged ends)"""
    import xfgstark
    prover._options = FC.product_options(xfgstark, BATCH_CASE)
    try:
        kws, wants = _batch_inputs(), _oracle_batch()
        a = prover.submit_batch(kws[:37], trace_length=64)
        b = prover.submit_batch(kws[37:], trace_length=64)
        got = [p.to_bytes() for p in b.result()]
        got = [p.to_bytes() for p in a.result()] + got
        assert len(got) == BATCH
        for i in range(BATCH):
            assert got[i] == wants[i], i
    finally:
        prover._options = xfgstark.ProofOptions.reference()


def test_trace_batch_validation_isolates_the_invalid_trace(prover):
    import xfgstark
    prover._options = FC.product_options(xfgstark, BATCH_CASE)
    try:
        oo = FC.oracle_options(BATCH_CASE)
        traces, airs, wants = [], [], []
        for i in range(BATCH):
            tr, air = T.valid_trace(64, 900 + i)
            if i == 35:
                tr[5][62] = 77  # constraint 5 at the last checked step
            st, want = O.prove(T.oracle_air(air), 64, oo, trace=W.flat(tr))
            assert st == 0
            traces.append(tr)
            airs.append(air)
            wants.append(want)
        res = prover.prove_traces(np.stack(traces), airs, validate=True)
        for i in range(BATCH):
            if i == 35:
                assert isinstance(res[i], xfgstark.XfgStarkError) and res[i].status == 11 and res[i].kind == "INVALID_TRACE"
            else:
                assert res[i].to_bytes() == wants[i], i
    finally:
        prover._options = xfgstark.ProofOptions.reference()


_KNOB_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import synthetic, xfgstark
pr = xfgstark.XfgBurnMintProver(proof_options=xfgstark.ProofOptions(21, 64, 4, 1, 8, 31))
res = pr.prove_batch([synthetic.burn_inputs(7300 + i) for i in range(70)], trace_length=64)
print(" ".join(hashlib.sha256(r.to_bytes()).hexdigest() for r in res))
pr.close()
"""


def test_unit_and_lane_knobs_keep_the_bytes():
    """XFG_UNIT = 5 (one proof per unit at blowup 64) and two lanes in a child process: the oracle's digests"""
    env = dict(os.environ, XFG_LANES="2", XFG_UNIT="5")
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, os.path.join(ROOT, "xfg-stark_amd"), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [hashlib.sha256(w).hexdigest() for w in _oracle_batch()]


# ---------------------------------------------------------------- sizes the oracle is not run at here
@pytest.mark.parametrize("case", W.GOLDEN_CASES, ids=W.case_id)
def test_large_shapes_match_recorded_oracle_digests(prover, case):
    import xfgstark
    n, beta, remdeg, q, fold, ext = case
    rec = [g for g in json.load(open(GOLD)) if g["case"] == list(case)]
    assert len(rec) == W.GOLDEN_PROOFS
    o = FC.product_options(xfgstark, case)
    prover._options = o
    try:
        kws = [synthetic.burn_inputs(W.GOLDEN_SEED + i) for i in range(W.GOLDEN_PROOFS)]
        got = [p.to_bytes() for p in prover.prove_batch(kws, trace_length=n)]
        v = xfgstark.XfgBurnMintVerifier(proof_options=o)
        items = [(g, xfgstark.air_consts(**kw)) for g, kw in zip(got, kws)]
        for g, r in zip(got, sorted(rec, key=lambda r: r["index"])):
            assert (len(g), hashlib.sha256(g).hexdigest()) == (r["len"], r["sha256"]), r["index"]
        assert v.batch_verify(items) == [True] * len(items)
        assert v.batch_verify(items, gpu=prover) == [True] * len(items)
        for (g, _), kw in zip(items, kws):
            assert O.verify(FC.oracle_air(kw), g, FC.oracle_options(case)) == 0
    finally:
        prover._options = xfgstark.ProofOptions.reference()


# ---------------------------------------------------------------- the GPU verifier on tampered proofs
@pytest.mark.parametrize("case", W.TAMPER_CASES, ids=W.case_id)
def test_gpu_verifier_on_tampered_and_forged_proofs(prover, case):
    """the items of the CPU test (a bit flipped in every section of one proof; the consistently committed
    forged proofs): the GPU verifier's verdict and error are the host verifier's, the verdict the oracle's"""
    import xfgstark
    kw, oair, proof = FC.oracle_proof(case)
    air = xfgstark.air_consts(**kw)
    v = xfgstark.XfgBurnMintVerifier(proof_options=FC.product_options(xfgstark, case))
    oo = FC.oracle_options(case)
    sec = _sections(proof)
    places = [sec["commitments"] + 1, sec["nonce"][0]]
    for name, where in sec.items():
        if name not in ("commitments", "nonce") and where[1] > 0:
            places += [where[0] + min(where[1] - 1, 7), where[0] + where[1] - 1]
    items = [(proof, air)] + [(_flip(proof, at), air) for at in places]
    oracle = [O.verify(oair, pf, oo) == 0 for pf, _ in items]
    for k, kw2, air2, faults, st, pf in VF.interleaved(case):
        assert st == 0
        items.append((pf, xfgstark.air_consts(**kw2)))
        oracle.append(O.verify(air2, pf, oo) == 0)
    got = v.debug_batch_verify(items, prover)
    host = [v.verify_with_details(*it)[:2] for it in items]
    assert [(ok, err) for ok, flags, err in got] == host
    assert [ok for ok, flags, err in got] == oracle
    assert v.batch_verify(items, gpu=prover) == oracle
    assert oracle.count(True) == 1 + VF.STATEMENTS


# ---------------------------------------------------------------- refusals
def test_refusals(prover):
    import xfgstark
    kw = synthetic.burn_inputs(1)
    try:
        prover._options = xfgstark.ProofOptions(42, 256, 4, 1, 8, 31)
        assert _status_of(lambda: prover.prove_burn_mint(**kw, trace_length=64))[0] == 6
        prover._options = xfgstark.ProofOptions(42, 32, 4, 1, 8, 31)
        st, msg = _status_of(lambda: prover.prove_burn_mint(**kw, trace_length=1 << 20))
        assert st == 6 and str(1 << 20) in msg and "32" in msg and str(1 << 24) in msg, msg
        # options that break an earlier rule as well are told about that rule, not about the domain
        prover._options = xfgstark.ProofOptions(42, 32, 4, 1, 3, 31)
        st, msg = _status_of(lambda: prover.prove_burn_mint(**kw, trace_length=1 << 20))
        assert st == 6 and "folding factor" in msg and str(1 << 24) not in msg, msg
        # a last FRI layer below the blowup factor, folding factor 8 included past blowup 16
        n, beta, remdeg = 128, 128, 0
        nl, last = FC.num_layers(n, beta, remdeg, 8)
        assert nl == 3 and last == 32 < beta
        prover._options = xfgstark.ProofOptions(42, beta, 4, 1, 8, remdeg)
        st, msg = _status_of(lambda: prover.prove_burn_mint(**kw, trace_length=n))
        assert st == 6 and "smaller than the blowup factor" in msg, msg
        assert FC.num_layers(64, 128, 0, 8) == (2, 128)  # a last layer equal to the blowup is proven
    finally:
        prover._options = xfgstark.ProofOptions.reference()
    assert _status_of(lambda: prover.debug_lde(np.zeros((1, 1 << 20), dtype=np.uint64), 1 << 20, 32))[0] == 9
    assert _status_of(lambda: prover.debug_lde(np.zeros((1, 64), dtype=np.uint64), 64, 256))[0] == 9
