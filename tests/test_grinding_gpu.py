"""GPU: the proof-of-work search on the device (csrc/grind.hip) -- the kernel alone through debug_grind against
the one-hash-at-a-time reference of tests/grind_ref.py (fixture seeds at chosen chunk positions, random seeds
under forced and planned geometry, a start just below 2^32, bounds, argument errors), then whole proofs at
grinding factors on both sides of GRIND_DEVICE_MIN byte for byte against the CPU oracle, through the three
verifiers, in batches with the search counters, as back-to-back units of one lane, and with a tampered nonce."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

import grind_ref as G
import oracle_lib as O
import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# forced geometries: (chunk_log, blocks); (0, 0) is the planner's own
SMALL = [(6, 1), (6, 5), (8, 3), (9, 64)]
PLAN = (0, 0)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


@pytest.fixture(scope="module")
def fixture_seeds():
    """[(seed, grind, nonce)] of tests/golden/grind_seeds.json, every nonce re-derived first"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "grind_seeds.json")))
    assert fx["chunk"] == 256
    out = [(bytes.fromhex(s["seed"]), s["grind"], s["nonce"]) for s in fx["seeds"]]
    for seed, grind, nonce in out:
        assert G.min_nonce(seed, grind) == nonce
    assert [x[2] for x in out] == [1, 2, 256, 257, 512, 513, 768, 769, 1537]
    return out


@functools.lru_cache(maxsize=None)
def _reference(count, grind):
    """(seeds, their smallest nonces from 1), computed once per shape"""
    seeds = G.random_seeds(f"{count}/{grind}", count)
    return seeds, [G.min_nonce(s, grind) for s in seeds]


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("blocks", [1, 2, 3, 7])
def test_fixture_seeds_at_chunk_positions(prover, fixture_seeds, blocks):
    """256-nonce chunks from nonce 1: the first and the last lane of chunk 0, the first of chunk 1, ... of
    chunk 6, with 1, 2, 3 and 7 blocks (a block's second and third claim); seeds of one factor share a call"""
    for grind in sorted({g for _, g, _ in fixture_seeds}):
        sel = [x for x in fixture_seeds if x[1] == grind]
        got = prover.debug_grind([s for s, _, _ in sel], grind, chunk_log=8, blocks=blocks)
        assert got == [n for _, _, n in sel], (grind, blocks)


def test_fixture_seeds_with_the_planned_geometry(prover, fixture_seeds):
    for seed, grind, nonce in fixture_seeds:
        assert prover.debug_grind([seed], grind) == [nonce]
    for grind in sorted({g for _, g, _ in fixture_seeds}):
        sel = [x for x in fixture_seeds if x[1] == grind]
        assert prover.debug_grind([s for s, _, _ in sel], grind) == [n for _, _, n in sel]


@pytest.mark.parametrize("count,grind", [(c, g) for g in (0, 1, 4, 8, 10) for c in (1, 3, 64, 257)] + [(64, 12)])
def test_random_seeds_match_reference(prover, count, grind):
    """every nonce equals grind_ref's under small forced geometries and the planner's, three times over with
    identical answers (at factors 0..2 nearly every chunk holds hits and a later chunk's can land first)"""
    seeds, want = _reference(count, grind)
    assert len(want) == count and all(w >= 1 for w in want)
    for chunk_log, blocks in SMALL + [PLAN]:
        runs = [prover.debug_grind(seeds, grind, chunk_log=chunk_log, blocks=blocks) for _ in range(3)]
        bad = [i for i in range(count) if runs[0][i] != want[i]]
        assert not bad, (chunk_log, blocks, bad[:5], [(runs[0][i], want[i]) for i in bad[:3]])
        assert runs[1] == runs[0] and runs[2] == runs[0], (chunk_log, blocks)


def test_search_crosses_into_the_high_message_word(prover):
    """first_nonce = 2^32 - 300 at factor 8: some seeds' nonces lie below 2^32 and some above (the bound is
    given: the prover's own, 2^16, lies below this start)"""
    first = (1 << 32) - 300
    last = first + (1 << 16)
    seeds = G.random_seeds("wrap", 16)
    want = [G.min_nonce(s, 8, first, last) for s in seeds]
    assert any(0 < w < 1 << 32 for w in want) and any(w >= 1 << 32 for w in want)
    for chunk_log, blocks in [(6, 3), (8, 2), PLAN]:
        got = prover.debug_grind(seeds, 8, first_nonce=first, max_nonce=last, chunk_log=chunk_log, blocks=blocks)
        assert got == want, (chunk_log, blocks)
    assert prover.debug_grind(seeds, 8, first_nonce=first) == [0] * 16  # max_nonce 0: the bound 2^16 < first


def test_max_nonce_bounds_the_search(prover):
    """max_nonce one below a seed's nonce: 0 for that seed (and for every seed whose nonce lies above it), the
    right nonce for the others; max_nonce equal to it: the nonce. Also a bound inside a chunk and an empty range"""
    seeds, want = _reference(64, 8)
    for pick in (want.index(max(want)), want.index(sorted(want)[32])):
        m = want[pick]
        assert m > 1
        for geo in [(6, 2), (8, 3), PLAN]:
            below = prover.debug_grind(seeds, 8, max_nonce=m - 1, chunk_log=geo[0], blocks=geo[1])
            assert below[pick] == 0
            assert below == [w if w <= m - 1 else 0 for w in want], geo
            at = prover.debug_grind(seeds, 8, max_nonce=m, chunk_log=geo[0], blocks=geo[1])
            assert at[pick] == m
            assert at == [w if w <= m else 0 for w in want], geo
    assert prover.debug_grind(seeds[:3], 8, first_nonce=5, max_nonce=4) == [0, 0, 0]
    # max_nonce 0 is the prover's bound 2^(grind + 8): every nonce lies below it
    assert max(want) <= 1 << 16 and prover.debug_grind(seeds, 8, max_nonce=0) == want


def test_argument_errors(prover):
    import xfgstark
    seed = [bytes(32)]
    for kw in [dict(grind=33), dict(grind=8, first_nonce=0), dict(grind=8, chunk_log=5), dict(grind=8, chunk_log=17),
               dict(grind=8, blocks=4097)]:
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.debug_grind(seed, **kw)
        assert e.value.status == 9, kw
    with pytest.raises(xfgstark.XfgStarkError) as e:
        prover.debug_grind([], 8)
    assert e.value.status == 9
    assert prover.debug_grind(seed, 32, max_nonce=300, chunk_log=6, blocks=4096) == [0]  # the limits themselves are served


# ---------------------------------------------------------------- whole proofs
def _options(xfgstark, beta, ext, fold, grind):
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension, o.fri_folding_factor, o.grinding_factor = beta, ext, fold, grind
    return o


def _oracle_options(beta, ext, fold, grind):
    return O.options(blowup=beta, field_extension=ext, fri_folding=fold, grinding=grind)


def _oracle_air(kw):
    st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
    assert st == 0
    return air


@functools.lru_cache(maxsize=None)
def _oracle_proof(index, n, beta, ext, fold, grind):
    kw = synthetic.burn_inputs(index)
    st, proof = O.prove(_oracle_air(kw), n, _oracle_options(beta, ext, fold, grind))
    assert st == 0
    return proof


def _check_proof(prover, index, n, beta, ext, fold, grind):
    import xfgstark
    kw = synthetic.burn_inputs(index)
    want = _oracle_proof(index, n, beta, ext, fold, grind)
    o = _options(xfgstark, beta, ext, fold, grind)
    prover._options = o
    got = prover.prove_burn_mint(**kw, trace_length=n).to_bytes()
    assert got == want
    air = xfgstark.air_consts(**kw)
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    ok, err, _ = v.verify_with_details(got, air)
    assert ok, err
    assert v.batch_verify([(got, air)], gpu=prover) == [True]
    assert O.verify(_oracle_air(kw), got, _oracle_options(beta, ext, fold, grind)) == 0
    return got


@pytest.mark.parametrize("n,beta,ext,fold,grind", [(64, 8, 1, 8, 12), (64, 8, 2, 8, 16), (256, 4, 1, 4, 16),
                                                   (512, 16, 2, 16, 14), (64, 8, 1, 8, 20)])
def test_proof_bytes_match_oracle_and_verify(prover, n, beta, ext, fold, grind):
    """one proof per shape (the factor-20 one included): the oracle's bytes, accepted by xfg_verify, the GPU
    batch verifier and the oracle verifier"""
    _check_proof(prover, 5200 + grind, n, beta, ext, fold, grind)


def test_both_sides_of_the_device_threshold(prover):
    """grinding factors GRIND_DEVICE_MIN - 1 (host loop) and GRIND_DEVICE_MIN (device search): the oracle's
    bytes either way, and the counters say which path ran"""
    dmin = prover.grind_probe()[0]
    assert 9 <= dmin <= 32
    for grind, where in [(dmin - 1, 2), (dmin, 1)]:
        before = prover.grind_probe()
        _check_proof(prover, 5300, 64, 8, 1, 8, grind)
        after = prover.grind_probe()
        assert after[where] - before[where] == 1 and after[3 - where] == before[3 - where], (grind, before, after)


def test_batches_match_singles_and_oracle_and_count_searches(prover):
    """prove_batch and submit_batch of 5 inputs at factor 16: the 5 single proofs, the oracle's; +5 device and
    +0 host searches around each. The same batch at factor 4: the reverse"""
    import xfgstark
    n, beta, ext, fold = 64, 8, 1, 8
    inputs = [synthetic.burn_inputs(5400 + i) for i in range(5)]
    for grind, where in [(16, 1), (4, 2)]:
        want = [_oracle_proof(5400 + i, n, beta, ext, fold, grind) for i in range(5)]
        prover._options = _options(xfgstark, beta, ext, fold, grind)
        singles = [prover.prove_burn_mint(**kw, trace_length=n).to_bytes() for kw in inputs]
        assert singles == want
        p0 = prover.grind_probe()
        assert [p.to_bytes() for p in prover.prove_batch(inputs, trace_length=n)] == want
        p1 = prover.grind_probe()
        assert [p.to_bytes() for p in prover.submit_batch(inputs, trace_length=n).result()] == want
        p2 = prover.grind_probe()
        for a, b in [(p0, p1), (p1, p2)]:
            assert b[where] - a[where] == 5 and b[3 - where] == a[3 - where], (grind, a, b)


_ONE_LANE_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import synthetic, xfgstark
o = xfgstark.ProofOptions.reference()
o.grinding_factor = 14
pr = xfgstark.XfgBurnMintProver(proof_options=o)
pend = [pr.submit_batch([synthetic.burn_inputs(5500 + 6 * k + i) for i in range(6)], trace_length=64) for k in range(2)]
for p in pend:
    print(" ".join(hashlib.sha256(r.to_bytes()).hexdigest() for r in p.result()))
print("probe", *pr.grind_probe())
"""


def test_one_lane_back_to_back_units_match_oracle():
    """XFG_LANES=1 XFG_UNIT=2: two batches of 6 inputs at factor 14 kept in flight are 6 units back to back on
    one lane, each writing its seeds to and reading its nonces from the same pinned blocks; every proof equals
    the oracle's, so no unit read a seed or a nonce written for the one before"""
    env = dict(os.environ, XFG_LANES="1", XFG_UNIT="2", XFG_SPLIT_MIN="2")
    r = subprocess.run([sys.executable, "-c", _ONE_LANE_CHILD, os.path.join(ROOT, "xfg-stark_amd"), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    got = " ".join(lines[:-1]).split()
    assert len(got) == 12
    for i in range(12):
        want = _oracle_proof(5500 + i, 64, 8, 1, 8, 14)
        assert hashlib.sha256(want).hexdigest() == got[i], i
    probe = lines[-1].split()
    assert probe[0] == "probe" and int(probe[1]) <= 14 and (int(probe[2]), int(probe[3])) == (12, 0)


def test_tampered_nonce_is_rejected_by_every_verifier(prover):
    """a factor-16 proof whose nonce (its last 8 bytes) is replaced by nonce + 1"""
    import xfgstark
    n, beta, ext, fold, grind = 64, 8, 1, 8, 16
    kw = synthetic.burn_inputs(5600)
    proof = _check_proof(prover, 5600, n, beta, ext, fold, grind)
    nonce = int.from_bytes(proof[-8:], "little")
    assert nonce == xfgstark.StarkProof.from_bytes(proof).pow_nonce
    bad = proof[:-8] + (nonce + 1).to_bytes(8, "little")
    air = xfgstark.air_consts(**kw)
    v = xfgstark.XfgBurnMintVerifier(proof_options=_options(xfgstark, beta, ext, fold, grind))
    ok, err, _ = v.verify_with_details(bad, air)
    assert not ok and err
    assert v.batch_verify([(proof, air), (bad, air)], gpu=prover) == [True, False]
    assert O.verify(_oracle_air(kw), bad, _oracle_options(beta, ext, fold, grind)) != 0
