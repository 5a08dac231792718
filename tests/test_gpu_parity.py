"""GPU parity: libxfgstark.so (HIP, gfx950) against the CPU oracle, bit for bit.

Kernel level: coset LDE / interpolation vs oracle NTT. Proof level: StarkProof bytes of the GPU
path == oracle bytes on the same ExecutionTrace / burn inputs (small sizes run the oracle live; the
benchmark shapes -- configs[2]'s 128 proofs of n=2^16 and the configs[4] proof of n=2^20 x 16,
quadratic -- are checked against committed oracle digests, tests/golden/). Large sizes beyond
the fixtures are checked through size-independent properties (the oracle verifier accepts,
determinism, batch == single)."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

import ntt_shapes
import oracle_lib as O
import proof_mutants as PM
import synthetic

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def oracle_air(kw):
    st, air = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                                kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
    assert st == 0
    return air


def with_blowup(prover, b):
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor = b
    prover._options = o
    return o


@pytest.mark.parametrize("n,blowup", ntt_shapes.LDE_3POLY)
def test_lde_kernel_matches_oracle(prover, n, blowup):
    rng = np.random.default_rng(n + blowup)
    coef = rng.integers(0, P, size=(3, n), dtype=np.uint64)
    got = prover.debug_lde(coef, n, blowup)
    for p in range(3):
        want = O.evaluate_lde([int(v) for v in coef[p]], blowup, 7)
        assert [int(v) for v in got[p]] == want


@pytest.mark.parametrize("n,blowup", ntt_shapes.LDE_1POLY)
def test_lde_kernel_tile_paths_match_oracle(prover, n, blowup):
    """the remaining four-step shapes: 2^18 (R = 256 narrow tiles, C = 1024 with 512-thread pass B
    tiles) and 2^22 (R = 1024 wide 1024-thread pass A, C = 4096 narrow pass B), one polynomial,
    compared as arrays; 2^20 x 16 (configs[4]) and 2^22 x 4: 2^24 points, past the four-step
    tables (running-product twiddles, standalone pass tables)"""
    rng = np.random.default_rng(n + 7)
    coef = rng.integers(0, P, size=(1, n), dtype=np.uint64)
    got = np.asarray(prover.debug_lde(coef, n, blowup))[0]
    assert np.array_equal(got, O.evaluate_lde_np(coef[0], blowup, 7))


@pytest.mark.parametrize("npoly,blowup", ntt_shapes.LDE_2P16_SETS)
def test_lde_launch_set_routes_match_oracle(prover, npoly, blowup):
    """the two routes of the tabled 2^16 forward LDE: launch sets of >= 512 all-coset blocks (16 per
    polynomial: 32 or 33 polynomials) take ntt_pass_a_cos2 (beta >= 4) / ntt_pass_a_cos (beta = 2) +
    ntt_pass_b_tq, smaller ones (28: one proof's trace is 7) one block per (tile, poly, coset); both
    bit-exact against the oracle on every polynomial"""
    n = 1 << 16
    rng = np.random.default_rng(npoly * 100 + blowup)
    coef = rng.integers(0, P, size=(npoly, n), dtype=np.uint64)
    got = np.asarray(prover.debug_lde(coef, n, blowup))
    for k in range(npoly):
        assert np.array_equal(got[k], O.evaluate_lde_np(coef[k], blowup, 7)), k


@pytest.mark.parametrize("blowup", ntt_shapes.LDE_R1024_BLOWUPS)
def test_lde_r1024_kernels_two_polys_match_oracle(prover, blowup):
    """ntt_pass_a_r1024 / ntt_pass_b_r1024 (n = 2^20 past the four-step tables): two polynomials, so
    the (poly, coset) block numbering of the coset-consecutive order is exercised across polys"""
    n = 1 << 20
    rng = np.random.default_rng(blowup + 31)
    coef = rng.integers(0, P, size=(2, n), dtype=np.uint64)
    got = np.asarray(prover.debug_lde(coef, n, blowup))
    for k in range(2):
        assert np.array_equal(got[k], O.evaluate_lde_np(coef[k], blowup, 7)), k


@pytest.mark.parametrize("n,npoly,blowup", ntt_shapes.LDE_ALL_COSET_GENERIC_B)
def test_lde_all_coset_generic_pass_b_matches_oracle(prover, n, npoly, blowup):
    """launch sets of >= 512 all-coset blocks at 2^17 and 2^18 (production batch shapes): ntt_pass_a_cos /
    ntt_pass_a_cos2 leave the four-step twiddles to the generic ntt_pass_b<9 | 10, false, 8, 5> (tq_b);
    bit-exact against the oracle on every polynomial"""
    rng = np.random.default_rng(n + npoly * 100 + blowup)
    coef = rng.integers(0, P, size=(npoly, n), dtype=np.uint64)
    got = np.asarray(prover.debug_lde(coef, n, blowup))
    for k in range(npoly):
        assert np.array_equal(got[k], O.evaluate_lde_np(coef[k], blowup, 7)), k


def test_ntt_sizes_without_a_kernel_are_refused(prover):
    """n = 16, blowup 2, remainder degree 7 folds 32 points once: the FRI remainder would be interpolated at
    size 4, which has no kernel (nor have sizes from 2^23): the prover says so instead of emitting a proof
    with an unwritten remainder, and the debug entries refuse such sizes as invalid arguments"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.fri_remainder_max_degree, o.num_queries = 2, 7, 8
    prover._options = o
    try:
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.prove_burn_mint(**synthetic.burn_inputs(916), trace_length=16)
        assert e.value.status == 6 and "NTT of size 4" in str(e.value)
        o.fri_remainder_max_degree = 1  # n = 32: 64 -> 8 -> 1, a remainder of size 1
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.prove_burn_mint(**synthetic.burn_inputs(916), trace_length=32)
        assert e.value.status == 6 and "NTT of size 1 " in str(e.value)
    finally:
        prover._options = xfgstark.ProofOptions.reference()
    big = np.zeros((1, 1 << 23), dtype=np.uint64)
    for call in (lambda: prover.debug_lde(big, 1 << 23, 2), lambda: prover.debug_interpolate(big, 1 << 23, False)):
        with pytest.raises(xfgstark.XfgStarkError) as e:
            call()
        assert e.value.status == 9


@pytest.mark.parametrize("n,off7", ntt_shapes.INTERPOLATE_1POLY)
def test_interpolate_kernel_tile_paths_match_oracle(prover, n, off7):
    rng = np.random.default_rng(n + 11)
    ev = rng.integers(0, P, size=(1, n), dtype=np.uint64)
    got = np.asarray(prover.debug_interpolate(ev, n, off7))[0]
    assert np.array_equal(got, O.interpolate_np(ev[0], 7 if off7 else 1))


P_GL = (1 << 64) - (1 << 32) + 1
_EDGE = [0, 1, 2, 3, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, P_GL - 2, P_GL - 1,
         P_GL, P_GL + 1, (1 << 64) - 2, (1 << 64) - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFE]


def _field_inputs(canonical, seed):
    rng = random.Random(seed)
    vals = [v for v in _EDGE if not canonical or v < P_GL]
    a = [x for x in vals for _ in vals] + [rng.randrange(P_GL if canonical else 1 << 64) for _ in range(20000)]
    b = [y for _ in vals for y in vals] + [rng.randrange(P_GL if canonical else 1 << 64) for _ in range(20000)]
    return a, b


def _pair_inputs(canonical, seed):
    """operands of the paired ops as interleaved arrays: the first words (a[2i], b[2i]) run through
    the edge list crossed with itself, the second words (a[2i+1], b[2i+1]) through an independently
    shuffled copy of the same cross, so the two halves of a pair are unrelated; plus 20000 random
    pairs, and the pairs with zero words ((0, 0), (x, 0), (0, x))"""
    rng = random.Random(seed)
    vals = [v for v in _EDGE if not canonical or v < P_GL]
    top = P_GL if canonical else 1 << 64
    first = [(x, y) for x in vals for y in vals]
    second = list(first)
    rng.shuffle(second)
    quads = [(x0, x1, y0, y1) for (x0, y0), (x1, y1) in zip(first, second)]
    quads += [(0, 0, 0, 0), (0, 0, 5, 7), (5, 0, 3, 0), (0, 5, 0, 3), (P_GL - 1, 0, 0, P_GL - 1), (0, 1, 0, 1)]
    quads += [tuple(rng.randrange(top) for _ in range(4)) for _ in range(20000)]
    a = [w for q in quads for w in q[:2]]
    b = [w for q in quads for w in q[2:]]
    return quads, a, b


def _check_pair_op(prover, op):
    import plain_ref as R
    quads, a, b = _pair_inputs(op != "mul2_pair", sum(op.encode()))
    got = prover.debug_field(op, np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)).tolist()
    assert len(got) == 2 * len(quads)
    for k, (x0, x1, y0, y1) in enumerate(quads):
        r = (got[2 * k], got[2 * k + 1])
        if op == "mul2_pair":  # two unrelated products through one gl_mul2, any u64 operands
            want = (x0 * y0 % P_GL, x1 * y1 % P_GL)
        elif op == "e2_mul":
            want = R.e_mul((x0, x1), (y0, y1))
        elif op == "e2_mulb":
            want = (x0 * y0 % P_GL, x1 * y0 % P_GL)
        else:  # e2_inv: x * out = 1 by the schoolbook product; 0 -> 0
            assert r[0] < P_GL and r[1] < P_GL, (op, x0, x1, r)
            want = (0, 0) if (x0, x1) == (0, 0) else (1, 0)
            assert R.e_mul((x0, x1), r) == want, (op, x0, x1, r)
            if (x0, x1) == (0, 0):
                assert r == (0, 0)
            continue
        assert r == want, (op, (x0, x1), (y0, y1), r, want)


@pytest.mark.parametrize("op", ["mul", "add", "sub", "canon", "pow2", "fold", "sub_weak", "add_w", "mul2", "mul2_pair",
                                "e2_mul", "e2_mulb", "e2_inv"])
def test_field_primitives_match_bigint(prover, op):
    """the gfx950 inline-asm Goldilocks primitives (gl.hpp) against Python integers, edge values
    (0, 2^32 - 1, p - 1, p, 2^64 - 1, ...) crossed with each other plus random operands; the paired
    ops (mul2_pair: one gl_mul2 on two unrelated products; e2_mul / e2_mulb / e2_inv of the quadratic
    extension, built on it) against the schoolbook product of plain_ref, both output words"""
    if op in ("mul2_pair", "e2_mul", "e2_mulb", "e2_inv"):
        return _check_pair_op(prover, op)
    canonical_in = op in ("add", "sub")
    a, b = _field_inputs(canonical_in, sum(op.encode()))
    if op == "pow2":
        b = [y % 96 for y in b]
    if op == "fold":
        b = [y & 0xFFFFFFFF for y in b]
    if op in ("sub_weak", "add_w"):  # butterfly contract: subtrahend / addend < p
        b = [y % P_GL for y in b]
    got = prover.debug_field(op, np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)).tolist()
    for x, y, r in zip(a, b, got):
        if op in ("mul", "mul2"):  # mul2: the interleaved pair (x y, y x), both checked on the device
            want = x * y % P_GL
        elif op == "add":
            want = (x + y) % P_GL
        elif op == "sub":
            want = (x - y) % P_GL
        elif op == "canon":
            want = x % P_GL
        elif op == "pow2":
            want = x * pow(2, y, P_GL) % P_GL
            if y == 0:  # identity: returned as is
                assert r == x
                continue
        elif op == "fold":
            want = (x + y * 0xFFFFFFFF) % P_GL
        elif op == "add_w":  # weak: the 64-bit sum with one carry folded in as + (2^32 - 1)
            want = x + y if x + y < (1 << 64) else x + y - (1 << 64) + 0xFFFFFFFF
            assert want < (1 << 64) and want % P_GL == (x + y) % P_GL
            assert r == want, (op, x, y, r, want)
            continue
        else:
            want = x - y if x >= y else x - y + P_GL
            assert r == want, (op, x, y, r, want)
            continue
        assert r == want, (op, x, y, r, want)


@pytest.mark.parametrize("n,off7", ntt_shapes.INTERPOLATE_2POLY)
def test_interpolate_kernel_matches_oracle(prover, n, off7):
    rng = np.random.default_rng(n)
    ev = rng.integers(0, P, size=(2, n), dtype=np.uint64)
    got = prover.debug_interpolate(ev, n, off7)
    for p in range(2):
        want = O.interpolate([int(v) for v in ev[p]], 7 if off7 else 1)
        assert [int(v) for v in got[p]] == want


EDGE = [0, 1, 2, P - 1, P - 2, 0xFFFFFFFF, 0x100000000, 0xFFFFFFFF00000000, 1 << 63, (1 << 63) - 1, P - 0xFFFFFFFF]


@pytest.mark.parametrize("n,blowup", [(4096, 8), (1 << 16, 8)])
def test_ntt_edge_values_match_oracle(prover, n, blowup):
    """boundary field values (all p - 1, all 0 but one, alternating extremes, random picks from
    EDGE): the weakly reduced butterflies and the carry-based reductions must agree with the
    oracle's canonical arithmetic"""
    rng = np.random.default_rng(7)
    polys = np.stack([np.full(n, P - 1, dtype=np.uint64),
                      np.array([EDGE[i % len(EDGE)] for i in range(n)], dtype=np.uint64),
                      np.array(rng.choice(EDGE, size=n), dtype=np.uint64),
                      np.where(np.arange(n) % 2 == 0, np.uint64(P - 1), np.uint64(0xFFFFFFFF00000000))])
    got = prover.debug_lde(polys, n, blowup)
    for p in range(len(polys)):
        assert [int(v) for v in got[p]] == O.evaluate_lde([int(v) for v in polys[p]], blowup, 7), p
    for off7 in (False, True):
        got = prover.debug_interpolate(polys, n, off7)
        for p in range(len(polys)):
            assert [int(v) for v in got[p]] == O.interpolate([int(v) for v in polys[p]], 7 if off7 else 1), (p, off7)


def _ood_deep_reference(co, h, z, zg, a, gam):
    """T_c(z), T_c(zg), H(z) and the DEEP quotient coefficients (synthetic division), plain ints"""
    n = len(h)

    def ev(poly, x):
        acc = 0
        for v in reversed(poly):
            acc = (acc * x + v) % P
        return acc
    ood = []
    for c in range(7):
        ood += [ev(co[c], z), ev(co[c], zg)]
    ood.append(ev(h, z))
    c1 = (sum(a[c] * ood[2 * c] for c in range(7)) + gam * ood[14]) % P
    c2 = sum(a[c] * ood[2 * c + 1] for c in range(7)) % P
    s = [sum(a[c] * co[c][j] for c in range(7)) % P for j in range(n)]
    p1 = [(s[j] + gam * h[j]) % P for j in range(n)]
    p1[0] = (p1[0] - c1) % P
    p2 = list(s)
    p2[0] = (p2[0] - c2) % P
    q1, q2, d = 0, 0, [0] * n
    for k in range(n - 2, -1, -1):
        q1 = (p1[k + 1] + z * q1) % P
        q2 = (p2[k + 1] + zg * q2) % P
        d[k] = (q1 + q2) % P
    return ood, d


@pytest.mark.parametrize("n,count", [(8, 2), (64, 3), (4096, 2), (1 << 14, 1)])
def test_ood_deep_kernels_match_reference(prover, n, count):
    rng = random.Random(n * 31 + count)
    co = [[[rng.randrange(P) for _ in range(n)] for _ in range(7)] for _ in range(count)]
    h = [[rng.randrange(P) for _ in range(n)] for _ in range(count)]
    zp = [[rng.randrange(1, P), rng.randrange(1, P)] for _ in range(count)]
    cf = [[rng.randrange(P) for _ in range(8)] for _ in range(count)]
    ood, deep = prover.debug_ood_deep(np.array(co, dtype=np.uint64), np.array(h, dtype=np.uint64),
                                      np.array(zp, dtype=np.uint64), np.array(cf, dtype=np.uint64))
    for b in range(count):
        want_ood, want_deep = _ood_deep_reference(co[b], h[b], zp[b][0], zp[b][1], cf[b][:7], cf[b][7])
        assert [int(v) for v in ood[b]] == want_ood
        assert [int(v) for v in deep[b]] == want_deep


@pytest.mark.parametrize("src,n,blowup", [("package", 64, 8), ("package", 64, 4), (0, 8, 8), (1, 16, 4), (7, 32, 2),
                                          (2, 128, 8), (3, 1024, 4), (4, 1024, 8), (5, 2048, 16), (6, 4096, 8)])
def test_prove_trace_bytes_match_oracle(prover, src, n, blowup):
    kw = synthetic.REFERENCE_PACKAGE if src == "package" else synthetic.burn_inputs(src)
    air = oracle_air(kw)
    opts = O.options(blowup=blowup)
    st, want = O.prove(air, n, opts)
    assert st == 0
    with_blowup(prover, blowup)
    trace = np.frombuffer(bytes(O.build_trace(air, n)), dtype=np.uint64).reshape(7, n)
    got = prover.prove_trace(trace, list(air.pub), air.nullifier, air.commitment).to_bytes()
    assert got == want
    assert O.verify(air, got, opts) == 0


@pytest.mark.parametrize("case", json.load(open(os.path.join(GOLD, "proofs.json"))), ids=lambda c: c["name"])
def test_prove_burn_mint_matches_golden(prover, case):
    kw = synthetic.REFERENCE_PACKAGE if case["source"] == "package" else synthetic.burn_inputs(case["source"])
    o = with_blowup(prover, case["blowup"])
    names = {"field_extension": "field_extension", "num_queries": "num_queries"}
    for k, v in case.get("options", {}).items():
        setattr(o, names[k], v)
    proof = prover.prove_burn_mint(**kw, trace_length=case["n"]).to_bytes()
    assert len(proof) == case["len"]
    assert hashlib.sha256(proof).hexdigest() == case["sha256"]
    if "proof_hex" in case:
        assert proof.hex() == case["proof_hex"]


def test_batch_equals_oracle_per_proof(prover):
    with_blowup(prover, 8)
    n = 1024
    inputs = [synthetic.burn_inputs(100 + i) for i in range(6)]
    proofs = prover.prove_batch(inputs, trace_length=n)
    for kw, pr in zip(inputs, proofs):
        st, want = O.prove(oracle_air(kw), n, O.options())
        assert pr.to_bytes() == want


def test_submitted_batches_in_flight_match_oracle(prover):
    """xfg_prove_batch_submit: three batches (different trace lengths, one spanning several lane
    units) in flight together, collected out of order; every proof equals the oracle's."""
    import xfgstark
    with_blowup(prover, 8)
    plan = [(1024, [synthetic.burn_inputs(300 + i) for i in range(40)]),
            (256, [synthetic.burn_inputs(400 + i) for i in range(5)]),
            (2048, [synthetic.burn_inputs(500 + i) for i in range(3)])]
    pend = [prover.submit_batch(kws, trace_length=n) for n, kws in plan]
    with pytest.raises(xfgstark.XfgStarkError):  # lane 0 belongs to the workers meanwhile
        prover.debug_lde(np.zeros((1, 8), dtype=np.uint64), 8, 2)
    with pytest.raises(xfgstark.XfgStarkError, match="batches pending"):
        prover.debug_constraint_eval(np.zeros((1, 7, 8), dtype=np.uint64), [([0] * 12, 0, 0)],
                                     np.zeros((1, 15, 1), dtype=np.uint64), 2)
    with pytest.raises(xfgstark.XfgStarkError, match="batches pending"):
        prover.debug_fri_fold(np.zeros((1, 1, 16), dtype=np.uint64), np.zeros((1, 1), dtype=np.uint64), 4, 0, False)
    for (n, kws), pb in reversed(list(zip(plan, pend))):
        res = pb.result()
        assert len(res) == len(kws)
        for kw, pr in zip(kws, res):
            st, want = O.prove(oracle_air(kw), n, O.options())
            assert st == 0 and pr.to_bytes() == want


def _config_golden(name):
    """tests/golden/config_proofs.json: digests of the oracle's proofs at the benchmark shapes
    (tests/golden/make_golden.py --configs; parity unpinned against real Winterfell, see
    oracle/oracle.h), so the GPU box never runs the oracle prover at these sizes"""
    return json.load(open(os.path.join(GOLD, "config_proofs.json")))[name]


def test_config2_full_batch_in_flight(prover):
    """BASELINE configs[2] at its real size: two 64-proof batches of (n = 2^16, blowup 8, options
    42/8/4/None/8/31) submitted together (depth 2, so both 32-proof units of each batch and the
    lane splitting of the tail run as in bench.py). ALL 128 proofs equal the oracle's bytes (length +
    SHA-256 of each, committed fixtures), and every one is accepted by the GPU batch verifier, the
    host verifier and the oracle verifier (reference: every proof is what prove_burn_mint returns,
    src/burn_mint_prover.rs:62-129; harness src/benchmarks/mod.rs:301-342)."""
    import xfgstark
    gold = _config_golden("config2_batch")
    n = gold["n"]
    assert n == 1 << 16 and gold["blowup"] == 8 and [g["source"] for g in gold["proofs"]] == list(range(128))
    prover._options = xfgstark.ProofOptions.reference()
    batches = [[synthetic.burn_inputs(i) for i in range(64)], [synthetic.burn_inputs(64 + i) for i in range(64)]]
    pend = [prover.submit_batch(kws, trace_length=n) for kws in batches]
    res = [pb.result() for pb in pend]
    proofs = [p.to_bytes() for r in res for p in r]
    bad = [i for i, (p, g) in enumerate(zip(proofs, gold["proofs"]))
           if len(p) != g["len"] or hashlib.sha256(p).hexdigest() != g["sha256"]]
    assert not bad, f"proofs differing from the oracle's: {bad}"
    v = xfgstark.XfgBurnMintVerifier()
    for kws, r in zip(batches, res):
        items = [(p.to_bytes(), xfgstark.air_consts(**kw)) for p, kw in zip(r, kws)]
        assert all(v.batch_verify(items, gpu=prover))
        assert all(v.batch_verify(items))
        for (p, _), kw in zip(items, kws):
            assert O.verify(oracle_air(kw), p, O.options()) == 0
    assert len(set(proofs)) == 128


def test_batch_isolates_invalid_inputs(prover):
    import xfgstark
    with_blowup(prover, 8)
    good = synthetic.burn_inputs(7)
    bad_burn = dict(good, burn_amount=1000, mint_amount=1000)
    bad_tx = dict(good, tx_prefix_hash=bytes(32))
    bad_rcpt = dict(good, recipient_address=b"\x01" * 19)
    res = prover.prove_batch([bad_burn, good, bad_tx, bad_rcpt, good], trace_length=256)
    assert isinstance(res[0], xfgstark.XfgStarkError) and res[0].status == 1
    assert isinstance(res[2], xfgstark.XfgStarkError) and res[2].status == 3
    assert isinstance(res[3], xfgstark.XfgStarkError) and res[3].status == 4
    st, want = O.prove(oracle_air(good), 256, O.options())
    assert res[1].to_bytes() == want == res[4].to_bytes()


def test_prove_burn_mint_errors_carry_reference_messages(prover):
    import xfgstark
    kw = synthetic.burn_inputs(1)
    with pytest.raises(xfgstark.XfgStarkError) as e:
        prover.prove_burn_mint(**dict(kw, mint_amount=16_000_000))
    assert "does not match burn amount" in str(e.value) and e.value.status == 2
    with pytest.raises(xfgstark.XfgStarkError) as e:
        prover.prove_burn_mint(**dict(kw, burn_amount=5))
    assert str(e.value).startswith("Burn amount must be exactly 0.8 XFG")


def test_invalid_trace_same_outcome_as_oracle(prover):
    import xfgstark
    kw = synthetic.burn_inputs(12)
    air = oracle_air(kw)
    n = 512
    tr = O.build_trace(air, n)
    tr[4 * n + 100] = 2  # illegal state jump
    opts = O.options()
    st, want = O.prove(air, n, opts, trace=tr)
    with_blowup(prover, 8)
    trace = np.frombuffer(bytes(tr), dtype=np.uint64).reshape(7, n)
    if st == 0:
        got = prover.prove_trace(trace, list(air.pub), air.nullifier, air.commitment).to_bytes()
        assert got == want
        assert O.verify(air, got, opts) != 0
    else:
        with pytest.raises(xfgstark.XfgStarkError):
            prover.prove_trace(trace, list(air.pub), air.nullifier, air.commitment)


_KINDS = ["random", "edge", "wide_consts"]


def _air_of(air):
    """O.Air filled field by field from (pub[12], nullifier, commitment)"""
    oa = O.Air()
    for i in range(12):
        oa.pub[i] = air[0][i]
    oa.secret = 0
    oa.nullifier = air[1]
    oa.commitment = air[2]
    return oa


def _arbitrary_case(ext, n, blowup, kind):
    """seeded arbitrary trace (plain_ref.make_trace) with its statement and the oracle's options"""
    import plain_ref as R
    tr, air = R.make_trace(kind, n, 7000 + 100 * ext + 3 * n + blowup + _KINDS.index(kind))
    flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr for v in col])
    return tr, air, _air_of(air), flat, O.options(blowup=blowup, field_extension=ext)


@pytest.mark.parametrize("kind", _KINDS)
@pytest.mark.parametrize("n,blowup", [(8, 8), (64, 2), (256, 8), (1024, 16)])
@pytest.mark.parametrize("ext", [1, 2])
def test_prove_arbitrary_trace_bytes_match_oracle(prover, ext, n, blowup, kind):
    """proofs of FALSE statements: traces that are no burn traces (uniformly random cells; edge
    values with d and d - 1 at 0, 1, p - 1; 64-bit AIR constants up to p - 1 with single constraints
    vanishing), so every transition expression, boundary numerator and composition coefficient
    contributes to the bytes -- on a valid trace six columns are constants and most of them are
    identically zero. The GPU proof equals the oracle's byte for byte, and the oracle verifier, the
    host verifier and the GPU batch verifier all reject it"""
    import xfgstark
    tr, air, oa, flat, opts = _arbitrary_case(ext, n, blowup, kind)
    st, want = O.prove(oa, n, opts, trace=flat)
    assert st == 0
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension = blowup, ext
    prover._options = o
    got = prover.prove_trace(np.array(tr, dtype=np.uint64), air[0], air[1], air[2]).to_bytes()
    assert got == want
    assert O.verify(oa, got, opts) != 0
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    assert v.batch_verify([(got, air)]) == [False]
    assert v.batch_verify([(got, air)], gpu=prover) == [False]


def _ce_coeffs(style, ext, rng):
    """15 composition coefficients (E tuples): random, edge-valued, or -- with an extension -- with one
    coordinate zero, alternating"""
    import plain_ref as R
    out = []
    for k in range(15):
        if style == "random":
            c = (rng.randrange(P), rng.randrange(P))
        elif style == "edge":
            c = (rng.choice(EDGE), rng.choice(EDGE))
        else:  # zero coordinates (and a zero coefficient)
            c = [(rng.randrange(P), 0), (0, rng.randrange(P)), (0, 0), (R.P - 1, 0), (0, 1)][(k + rng.randrange(5)) % 5]
        out.append(c if ext == 2 else (c[0], 0))
    return out


def _run_constraint_eval(prover, traces, airs, coeffs, blowup, ext):
    """-> per instance, the kernel's 2n E tuples"""
    co = np.array([[list(c[:ext]) for c in cs] for cs in coeffs], dtype=np.uint64)
    ce = prover.debug_constraint_eval(np.array(traces, dtype=np.uint64), airs, co, blowup)
    assert ce.shape == (len(traces), ext, 2 * len(traces[0][0]))
    return [[(int(ce[b, 0, i]), int(ce[b, 1, i]) if ext == 2 else 0) for i in range(ce.shape[2])]
            for b in range(len(traces))]


@pytest.mark.parametrize("n,blowup,count", [(8, 2, 1), (8, 16, 2), (128, 8, 1), (256, 4, 2), (512, 2, 3)])
@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_eval_kernel_matches_reference(prover, ext, n, blowup, count):
    """constraint_eval_kernel behind the prover's own interpolation, LDE and batch-inverted divisor
    table, against plain_ref.constraint_evals at every point of the CE domain. Shapes: a block smaller
    than a wavefront with beta / 2 = 1 (8, 2); nce = 256, exactly one block (128); one block per
    parity (256); four blocks and three instances (512: the blockIdx.y strides of air, coeffs, lde,
    ce). Three calls per shape rotate the trace kinds over the instances with random, edge-valued and
    zero-coordinate coefficients"""
    import plain_ref as R
    rng = random.Random(n * 64 + blowup * 4 + ext)
    for call, style in enumerate(["random", "edge", "zeros"]):
        made = [R.make_trace(_KINDS[(call + b) % 3], n, rng.randrange(1 << 30)) for b in range(count)]
        traces, airs = [m[0] for m in made], [m[1] for m in made]
        coeffs = [_ce_coeffs(style, ext, rng) for _ in range(count)]
        got = _run_constraint_eval(prover, traces, airs, coeffs, blowup, ext)
        for b in range(count):
            want = R.constraint_evals(traces[b], airs[b], coeffs[b])
            bad = [i for i in range(2 * n) if got[b][i] != want[i]]
            assert not bad, (style, b, bad[:8], [(got[b][i], want[i]) for i in bad[:2]])


@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_eval_unit_coefficients_name_the_index(prover, ext):
    """one coefficient at a time set to 1 (and to phi with an extension), the others 0, at n = 8: a
    swapped or misread coefficient slot shows up under its own index"""
    import plain_ref as R
    n, blowup = 8, 4
    tr, _ = R.make_trace("random", n, 41)
    air = R.WIDE_AIR
    units = [(k, u) for u in ([(1, 0), (0, 1)] if ext == 2 else [(1, 0)]) for k in range(15)]
    coeffs = [[u if j == k else (0, 0) for j in range(15)] for k, u in units]
    got = _run_constraint_eval(prover, [tr] * len(units), [air] * len(units), coeffs, blowup, ext)
    wrong = [(k, u) for b, (k, u) in enumerate(units) if got[b] != R.constraint_evals(tr, air, coeffs[b])]
    assert not wrong, f"coefficient slots (index, unit) evaluated wrongly: {wrong}"
    zero = R.constraint_evals(tr, air, [(0, 0)] * 15)
    assert all(got[b] != zero for b in range(len(units)))  # every slot contributes on this trace


def _fold_set(name, D, ext, rng):
    """D E-values in natural order for one fold instance"""
    R8 = D // 8
    hi = (1 << 64) - (1 << 32)

    def plane(flip):
        if name == "random":
            return [rng.randrange(P) for _ in range(D)]
        if name == "all_pm1":
            return [P - 1] * D
        if name == "one_per_row":  # row i holds indices i + k D/8
            v = [0] * D
            for i in range(R8):
                v[i + rng.randrange(8) * R8] = rng.choice([1, P - 1, hi, rng.randrange(1, P)])
            return v
        if name == "alternating":  # alternates inside a row (k) and from row to row
            return [P - 1 if (K + K // R8 + flip) % 2 == 0 else hi for K in range(D)]
        return [rng.choice(EDGE) for _ in range(D)]
    planes = [plane(0), plane(1) if ext == 2 else [0] * D]
    return list(zip(*planes))


def _run_fold(prover, sets, alphas, logn, logbeta, coset_major, ext):
    import plain_ref as R
    n, beta = 1 << logn, 1 << logbeta
    stored = [R.to_coset_major(s, n, beta) if coset_major else s for s in sets]
    vals = np.array([[[v[c] for v in s] for c in range(ext)] for s in stored], dtype=np.uint64)
    al = np.array([list(a[:ext]) for a in alphas], dtype=np.uint64)
    out = prover.debug_fri_fold(vals, al, logn, logbeta, coset_major)
    assert out.shape == (len(sets), ext, (n * beta) // 8)
    return out


@pytest.mark.parametrize("logn,logbeta,coset_major", [(4, 0, False), (6, 0, False), (5, 1, True), (11, 0, False),
                                                      (9, 3, True), (8, 4, True)])
@pytest.mark.parametrize("ext", [1, 2])
def test_fri_fold_kernel_matches_reference(prover, ext, logn, logbeta, coset_major):
    """fri_fold_kernel (size-8 inverse DFT, canonicalisation, Horner in E, the 2^-3 scaling) against
    the Lagrange interpolation of plain_ref.fold_row, every row. Shapes: D = 16 (a 2-thread block),
    64 natural and coset-major, 2048 (256 rows: one full block), 4096 coset-major at beta 8 and 16
    (two blocks). Inputs: random, all p - 1, one non-zero value per row, alternating p - 1 /
    2^64 - 2^32, picks from EDGE; each with every alpha: random, 1, p - 1 and with an extension
    (a, 0), (0, b), (p - 1, p - 1); two instances per launch"""
    import plain_ref as R
    D = 1 << (logn + logbeta)
    rng = random.Random(D * 8 + logbeta * 2 + ext)
    if ext == 2:
        alphas = [(rng.randrange(P), rng.randrange(P)), (1, 0), (P - 1, 0), (rng.randrange(P), 0),
                  (0, rng.randrange(1, P)), (P - 1, P - 1)]
    else:
        alphas = [(rng.randrange(P), 0), (1, 0), (P - 1, 0), (rng.choice(EDGE[4:]), 0)]
    for name in ["random", "all_pm1", "one_per_row", "alternating", "edge"]:
        for k in range(0, len(alphas), 2):
            sets = [_fold_set(name, D, ext, rng) for _ in range(2)]
            out = _run_fold(prover, sets, alphas[k:k + 2], logn, logbeta, coset_major, ext)
            for b in range(2):
                want = R.fold_layer(sets[b], D, alphas[k + b])
                got = [(int(out[b, 0, i]), int(out[b, 1, i]) if ext == 2 else 0) for i in range(D // 8)]
                bad = [i for i in range(D // 8) if got[i] != want[i]]
                assert not bad, (name, alphas[k + b], bad[:8], [(got[i], want[i]) for i in bad[:2]])


def test_fri_fold_kernel_first_layer_of_config2_sampled(prover):
    """D = 2^19 coset-major at beta 8 (the first FRI layer of the n = 2^16 benchmark shape), no
    extension: the kernel runs in full; the first and last row of each of its 256 blocks and 2048
    seeded random rows are compared (a full Python reference at this size would take minutes)"""
    import plain_ref as R
    logn, logbeta = 16, 3
    D, rows = 1 << 19, 1 << 16
    rs = np.random.default_rng(19)
    nat = rs.integers(0, P, size=D, dtype=np.uint64)
    edge_at = rs.integers(0, D, size=D // 8)
    nat[edge_at] = rs.choice(np.array(EDGE, dtype=np.uint64), size=D // 8)
    K = np.arange(D)
    stored = np.zeros(D, dtype=np.uint64)
    stored[(K % 8) * (1 << logn) + K // 8] = nat  # natural index K at (K mod beta) n + K // beta
    alpha = (random.Random(19).randrange(P), 0)
    out = prover.debug_fri_fold(stored.reshape(1, 1, D), np.array([[alpha[0]]], dtype=np.uint64), logn, logbeta, True)
    pick = sorted({b * 256 + e for b in range(rows // 256) for e in (0, 255)}
                  | set(random.Random(20).sample(range(rows), 2048)))
    bad = []
    for i in pick:
        want = R.fold_row([(int(nat[i + k * rows]), 0) for k in range(8)], i, D, alpha)
        if (int(out[0, 0, i]), 0) != want:
            bad.append(i)
    assert not bad, bad[:16]


def test_noncanonical_air_constants_and_debug_inputs_are_rejected(prover):
    """xfg_prove_trace and the kernel-level hooks refuse values >= p with XFG_INVALID_ARGUMENT and a
    message (the constraint kernel's subtractions are exact for canonical operands only); p - 1 is
    accepted (wide_consts above)"""
    import plain_ref as R
    import xfgstark
    with_blowup(prover, 8)
    n = 8
    tr, air = R.make_trace("random", n, 77)
    trace = np.array(tr, dtype=np.uint64)
    for bad in [([P if i == 5 else v for i, v in enumerate(air[0])], air[1], air[2]),
                (air[0], P, air[2]), (air[0], air[1], (1 << 64) - 1)]:
        with pytest.raises(xfgstark.XfgStarkError, match="AIR constant is not a canonical") as e:
            prover.prove_trace(trace, bad[0], bad[1], bad[2])
        assert e.value.status == 9
        with pytest.raises(xfgstark.XfgStarkError, match="AIR constant is not a canonical") as e:
            prover.debug_constraint_eval(trace[None], [bad], np.ones((1, 15, 1), dtype=np.uint64), 2)
        assert e.value.status == 9
    co = np.ones((1, 15, 2), dtype=np.uint64)
    co[0, 14, 1] = P
    with pytest.raises(xfgstark.XfgStarkError, match="not a canonical") as e:
        prover.debug_constraint_eval(trace[None], [air], co, 2)
    assert e.value.status == 9
    vals, al = np.ones((1, 1, 16), dtype=np.uint64), np.ones((1, 1), dtype=np.uint64)
    for v, a in [(np.where(np.arange(16) == 9, np.uint64(P), vals), al), (vals, al * np.uint64(P))]:
        with pytest.raises(xfgstark.XfgStarkError, match="not a canonical") as e:
            prover.debug_fri_fold(v, a, 4, 0, False)
        assert e.value.status == 9
    # the accepted neighbours: the same calls with canonical values run
    assert prover.debug_fri_fold(vals, al, 4, 0, False).shape == (1, 1, 2)
    assert prover.debug_constraint_eval(trace[None], [air], np.ones((1, 15, 2), dtype=np.uint64), 2).shape == (1, 2, 16)


@pytest.mark.parametrize("logn,blowup", [(17, 8), (18, 8), (20, 16)])
def test_large_traces_verify(prover, logn, blowup):
    # beyond fixture sizes: the oracle verifier (fast, O(queries * log N)) must accept the GPU proof,
    # and proving twice is deterministic
    kw = synthetic.burn_inputs(logn)
    with_blowup(prover, blowup)
    n = 1 << logn
    p1 = prover.prove_burn_mint(**kw, trace_length=n).to_bytes()
    p2 = prover.prove_burn_mint(**kw, trace_length=n).to_bytes()
    assert p1 == p2
    assert O.verify(oracle_air(kw), p1, O.options(blowup=blowup)) == 0


@pytest.mark.parametrize("n,kw", [(2048, dict(fri_remainder_max_degree=255)), (1024, dict(fri_remainder_max_degree=7)),
                                  (512, dict(num_queries=24, grinding_factor=0)), (256, dict(blowup_factor=16))])
def test_other_options_match_oracle_and_verify(prover, n, kw):
    """non-default ProofOptions (long multi-chunk FRI remainder commitment, small remainder, fewer
    queries / no grinding, blowup 16): GPU bytes == oracle bytes, and the product verifier accepts"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    for k, v in kw.items():
        setattr(o, k, v)
    prover._options = o
    kws = synthetic.burn_inputs(900 + n)
    proof = prover.prove_burn_mint(**kws, trace_length=n).to_bytes()
    oo = O.options(num_queries=o.num_queries, blowup=o.blowup_factor, grinding=o.grinding_factor,
                   fri_rem_max_deg=o.fri_remainder_max_degree)
    st, want = O.prove(oracle_air(kws), n, oo)
    assert st == 0 and proof == want
    assert xfgstark.XfgBurnMintVerifier(proof_options=o).verify_burn_mint(proof, **kws)


def test_generate_from_data_package_matches_golden(prover, tmp_path):
    """CLI `generate` path: data package JSON -> MI355X proof -> proof package JSON; the proof bytes
    equal the committed oracle fixture for the reference package (n = 64, blowup 8)"""
    import test_package as TP
    from xfgstark import package as K
    with_blowup(prover, 8)
    src, dst = tmp_path / "pkg.json", tmp_path / "proof.json"
    src.write_text(json.dumps(TP._package()))
    K.generate_proof(prover, str(src), str(dst), trace_length=64, created_at="2025-08-30T06:00:00+00:00")
    data, pub, meta = K.load_proof_package(str(dst))
    case = [c for c in json.load(open(os.path.join(GOLD, "proofs.json"))) if c["name"] == "pkg_n64_b8"][0]
    assert data.hex() == case["proof_hex"]
    # batch generate: invalid packages are reported, valid ones proven in one batch
    pk = [K.StarkProofDataPackage(TP._package()),
          K.StarkProofDataPackage(TP._package(**{"burn_transaction.burn_amount_xfg": "1.0"})),
          K.StarkProofDataPackage(TP._package(**{"burn_transaction.transaction_hash": "00"})),
          K.StarkProofDataPackage(TP._package())]
    res = K.generate_proofs(prover, pk, trace_length=64)
    assert res[1][0] is None and not res[1][1].is_valid
    assert res[2][0] is None and isinstance(res[2][1], K.PackageError)
    assert bytes(res[0][0]["proof_data"]) == bytes(res[3][0]["proof_data"]) == data


@pytest.mark.parametrize("n,kw", [(64, dict(blowup_factor=8)), (256, dict(blowup_factor=4)),
                                  (1024, dict(blowup_factor=16, num_queries=24)),
                                  (2048, dict(blowup_factor=8, fri_remainder_max_degree=255)),
                                  (128, dict(blowup_factor=2, grinding_factor=0))])
def test_quadratic_extension_matches_oracle(prover, n, kw):
    """FieldExtension::Quadratic: GPU bytes == oracle bytes (batch of 3 statements), and both the
    product verifier and the oracle verifier accept"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.field_extension = 2
    for k, v in kw.items():
        setattr(o, k, v)
    prover._options = o
    kws = [synthetic.burn_inputs(1300 + n + i) for i in range(3)]
    res = prover.prove_batch(kws, trace_length=n)
    oo = O.options(num_queries=o.num_queries, blowup=o.blowup_factor, grinding=o.grinding_factor, field_extension=2,
                   fri_rem_max_deg=o.fri_remainder_max_degree)
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    for kw_, pr in zip(kws, res):
        st, want = O.prove(oracle_air(kw_), n, oo)
        assert st == 0 and pr.to_bytes() == want
        assert v.verify_burn_mint(pr, **kw_)


def test_config5_quadratic_2p20_blowup16(prover):
    """BASELINE configs[4] as bench.py runs it: n = 2^20, blowup 16, quadratic extension, 24 queries,
    grinding 4 (~100-bit conjectured security). The proof's bytes equal the oracle's (length + SHA-256,
    committed fixture), both verifiers accept it, and proving twice is deterministic"""
    import xfgstark
    gold = _config_golden("config5")
    assert gold["n"] == 1 << 20 and gold["blowup"] == 16 and gold["options"] == {"field_extension": 2, "num_queries": 24}
    o = xfgstark.ProofOptions.reference()
    o.field_extension, o.blowup_factor, o.num_queries = 2, 16, 24
    prover._options = o
    kw = synthetic.burn_inputs(gold["source"])
    p1 = prover.prove_burn_mint(**kw, trace_length=1 << 20).to_bytes()
    assert len(p1) == gold["len"] and hashlib.sha256(p1).hexdigest() == gold["sha256"]
    assert xfgstark.XfgBurnMintVerifier(proof_options=o).verify_burn_mint(p1, **kw)
    oo = O.options(num_queries=24, blowup=16, field_extension=2)
    assert O.verify(oracle_air(kw), p1, oo) == 0
    assert prover.prove_burn_mint(**kw, trace_length=1 << 20).to_bytes() == p1


def test_config5_pipelined_batches(prover):
    """bench.py config5()'s own workload: 4-proof configs[4] batches (synthetic.burn_inputs(50000..50003),
    n = 2^20, blowup 16, quadratic, 24 queries), three calls in flight through submit_batch so that lanes
    prove them side by side; all 12 proofs equal the committed oracle digests"""
    import xfgstark
    gold = _config_golden("config5_batch")
    assert gold["n"] == 1 << 20 and gold["blowup"] == 16 and gold["options"] == {"field_extension": 2, "num_queries": 24}
    o = xfgstark.ProofOptions.reference()
    o.field_extension, o.blowup_factor, o.num_queries = 2, 16, 24
    prover._options = o
    kws = [synthetic.burn_inputs(g["source"]) for g in gold["proofs"]]
    pend = [prover.submit_batch(kws, trace_length=gold["n"]) for _ in range(3)]
    res = [pb.result() for pb in pend]
    bad = [(c, i) for c, r in enumerate(res) for i, (p, g) in enumerate(zip(r, gold["proofs"]))
           if hashlib.sha256(p.to_bytes()).hexdigest() != g["sha256"]]
    assert bad == [] and all(len(r) == 4 for r in res)


@pytest.mark.parametrize("shape", ["config5", "config2"])
def test_repeated_single_proofs_identical(prover, shape):
    """The same proof requested 16 times in a row, one synchronous call each: the calls land on
    different lanes, some of them fresh, so any race or unmodelled hazard in the kernels (a result that
    depends on timing) shows up as a proof whose bytes differ. Every one must equal the committed oracle
    digest (configs[4] at n = 2^20, and configs[2]'s first proof at 2^16). A round-6 butterfly variant
    (two borrow chains in one asm block) returned a different trace, composition or FRI root in about 1
    of 4 such configs[4] proofs while every single-call test passed (profiles/r06/determinism.txt)"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    if shape == "config5":
        gold = _config_golden("config5")
        o.field_extension, o.blowup_factor, o.num_queries = 2, 16, 24
        src, n, want = gold["source"], gold["n"], gold["sha256"]
    else:
        gold = _config_golden("config2_batch")
        src, n, want = 0, gold["n"], gold["proofs"][0]["sha256"]
    prover._options = o
    kw = synthetic.burn_inputs(src)
    got = [hashlib.sha256(prover.prove_burn_mint(**kw, trace_length=n).to_bytes()).hexdigest() for _ in range(16)]
    assert [i for i, h in enumerate(got) if h != want] == []


@pytest.mark.parametrize("ext,n,blowup", [(1, 1024, 8), (2, 512, 16), (1, 1 << 16, 8)])
def test_gpu_batch_verify_matches_host_verifier(prover, ext, n, blowup):
    """xfg_verify_batch_gpu: same verdicts as the host verifier on GPU-made proofs, valid and
    tampered (every section), wrong statements and wrong options"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.field_extension, o.blowup_factor = ext, blowup
    prover._options = o
    kws = [synthetic.burn_inputs(2100 + i) for i in range(6)]
    proofs = [p.to_bytes() for p in prover.prove_batch(kws, trace_length=n)]
    airs = [xfgstark.air_consts(**kw) for kw in kws]
    items = []
    for p, a in zip(proofs, airs):
        items.append((p, a))
        for frac in (0.05, 0.2, 0.35, 0.5, 0.7, 0.9, 0.995):  # flips across the proof sections
            b = bytearray(p)
            b[int(len(b) * frac)] ^= 0x10
            items.append((bytes(b), a))
        items.append((p, (a[0], a[1] ^ 1, a[2])))
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    host = v.batch_verify(items)
    dev = v.batch_verify(items, gpu=prover)
    assert dev == host
    assert sum(host) == len(proofs)  # exactly the untampered proofs with their own statement
    # the oracle's own verifier on the same items: accepted exactly where the product accepts
    oo = O.options(blowup=blowup, field_extension=ext)
    for (p, a), ok in zip(items, host):
        oa = O.Air()
        oa.pub = (O.C.c_uint64 * 12)(*a[0])
        oa.nullifier, oa.commitment = a[1], a[2]
        assert (O.verify(oa, p, oo) == 0) == ok
    other = xfgstark.ProofOptions.reference()
    other.num_queries = 41
    assert not any(xfgstark.XfgBurnMintVerifier(proof_options=other).batch_verify(items[:3], gpu=prover))


@pytest.mark.parametrize("ext", [1, 2])
def test_gpu_batch_verify_node_vector_mutants(prover, ext):
    """vtree_kernel's device walk of the batch openings (node-vector consumption, npairs == nvec,
    compaction) against the host verifier's BatchMerkleProof::get_root and the oracle verifier on
    openings whose node vectors parse but do not fit: the GPU, host and oracle verdicts are equal on
    every item, the misfits are rejected, an appended (unread) node is accepted as winter-crypto
    0.8's get_root accepts it, and the untouched proofs stay accepted in the same batch.
    Pinned to the project's oracle restatement (oracle/orc_stark.c batch_root), not to an upstream
    fixture: winter-crypto is not vendored in the reference, so the appended-node verdict is parity
    unpinned against it"""
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.field_extension = ext
    prover._options = o
    kws = [synthetic.burn_inputs(2500 + i) for i in range(3)]
    proofs = [p.to_bytes() for p in prover.prove_batch(kws, trace_length=1024)]
    airs = [xfgstark.air_consts(**kw) for kw in kws]
    items, want = [], []
    for p, a in zip(proofs, airs):
        items.append((p, a))
        want.append(True)
        for m, ok in PM.node_vector_mutants(p):
            items.append((m, a))
            want.append(ok)
    v = xfgstark.XfgBurnMintVerifier(proof_options=o)
    host = v.batch_verify(items)
    dev = v.batch_verify(items, gpu=prover)
    assert dev == host
    assert host == want
    oo = O.options(field_extension=ext)
    for (p, a), ok in zip(items, host):
        oa = O.Air()
        oa.pub = (O.C.c_uint64 * 12)(*a[0])
        oa.nullifier, oa.commitment = a[1], a[2]
        assert (O.verify(oa, p, oo) == 0) == ok


def test_gpu_batch_verifier_reports_structural_errors_first(prover):
    """the nine doubly broken proofs of proof_mutants.CHECK_ORDER (a FRI section of the wrong size, alone
    or with a flipped byte in a section opened before it) in one xfg_debug_verify_batch_gpu call, an honest
    proof before each: the GPU verifier does not send a proof with a broken FRI structure to the device, so
    it answers with the structural error whatever else is wrong, flag word 0 (recorded from the build before
    the host verifier became an executor of the plan), while xfg_verify reports the same proofs at the
    structural error's place in its walk (test_verifier_plan_cpu.py); the honest proofs are accepted"""
    import xfgstark
    import fold_cases as FC
    v = xfgstark.XfgBurnMintVerifier()
    items, want_gpu, want_host = [], [], []
    for n, short, cut, flip, host_err in PM.CHECK_ORDER:
        kw, air, proof = FC.oracle_proof((n, 8, 31, 42, 8, 1))
        xair = xfgstark.air_consts(**kw)
        items += [(proof, xair), (PM.doubly_broken(proof, short, cut, flip), xair)]
        want_gpu += [(True, 0, None), (False, 0, PM.REMAINDER_FOLDING if short == "remainder" else PM.LAYER_SIZE)]
        want_host += [(True, None), (False, host_err)]
    assert v.debug_batch_verify(items, prover) == want_gpu
    assert [v.verify_with_details(*it)[:2] for it in items] == want_host
    assert v.batch_verify(items, gpu=prover) == [ok for ok, err in want_host]


def test_rejects_options_the_reference_rejects(prover):
    import xfgstark
    kw = synthetic.burn_inputs(3)
    with_blowup(prover, 2)
    with pytest.raises(xfgstark.XfgStarkError) as e:  # 42 queries >= LDE domain of 32
        prover.prove_burn_mint(**kw, trace_length=16)
    assert e.value.status == 6
    with_blowup(prover, 3)
    with pytest.raises(xfgstark.XfgStarkError):
        prover.prove_burn_mint(**kw, trace_length=64)
    with_blowup(prover, 8)
    with pytest.raises(xfgstark.XfgStarkError):
        prover.prove_burn_mint(**kw, trace_length=100)


def test_submit_rejects_empty_and_unsized_batches(prover):
    """an empty batch and a trace length with no proof-size bound reach the C library, which reports
    XFG_INVALID_ARGUMENT / PROVER_ERROR as XfgStarkError (not a bare ValueError from the buffer pool)"""
    import xfgstark
    prover._options = xfgstark.ProofOptions.reference()
    prover.__dict__.get("_free", []).clear()
    with pytest.raises(xfgstark.XfgStarkError):
        prover.submit_batch([], trace_length=1024).result()
    with pytest.raises(xfgstark.XfgStarkError):
        prover.submit_batch([synthetic.burn_inputs(1)], trace_length=100).result()


_KNOB_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import synthetic, xfgstark
pr = xfgstark.XfgBurnMintProver()
for n in (1024, 1 << 16):
    res = pr.prove_batch([synthetic.burn_inputs(700 + i) for i in range(12)], trace_length=n)
    print(n, " ".join(hashlib.sha256(r.to_bytes()).hexdigest() for r in res))
"""


def test_env_knobs_keep_proof_bytes(prover, tmp_path):
    """every environment knob the library still reads (XFG_LANES, XFG_UNIT, XFG_SPLIT_MIN,
    XFG_HOST_THREADS, XFG_TRACE) changes scheduling only: a child process with non-default values
    (2 lanes, 5-proof units split down to 2, 1 host thread, host traces on) emits the same 12 proofs
    at n = 2^10 and 2^16 as this process at the defaults, and the first proof equals the oracle's"""
    import subprocess
    import sys
    import xfgstark
    prover._options = xfgstark.ProofOptions.reference()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, XFG_LANES="2", XFG_UNIT="5", XFG_SPLIT_MIN="2", XFG_HOST_THREADS="1", XFG_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, os.path.join(root, "xfg-stark_amd"), root],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.strip(), "XFG_TRACE=1 printed no host trace"
    got = {int(line.split()[0]): line.split()[1:] for line in r.stdout.strip().splitlines()}
    for n in (1024, 1 << 16):
        kws = [synthetic.burn_inputs(700 + i) for i in range(12)]
        want = [p.to_bytes() for p in prover.prove_batch(kws, trace_length=n)]
        assert got[n] == [hashlib.sha256(b).hexdigest() for b in want], n
    st, oracle = O.prove(oracle_air(synthetic.burn_inputs(700)), 1024, O.options())
    assert st == 0 and hashlib.sha256(oracle).hexdigest() == got[1024][0]


_ONE_LANE_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import synthetic, xfgstark
pr = xfgstark.XfgBurnMintProver()
pend = [pr.submit_batch([synthetic.burn_inputs(1300 + 6 * k + i) for i in range(6)], trace_length=1024)
        for k in range(2)]
for p in pend:
    print(" ".join(hashlib.sha256(r.to_bytes()).hexdigest() for r in p.result()))
"""


def test_one_lane_back_to_back_units_match_oracle():
    """the per-unit host blocks kernels read and write in place (AIR constants, coins, replay block,
    opening indices / values / digests: fine-grained pinned memory) are rewritten by the CPU for every
    unit: ONE lane with 2-proof units proves 12 distinct inputs as 6 units back to back (two batches in
    flight), and every proof equals the oracle's -- a stale constant, coin or index from the previous
    unit would change the bytes"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, XFG_LANES="1", XFG_UNIT="2", XFG_SPLIT_MIN="2")
    r = subprocess.run([sys.executable, "-c", _ONE_LANE_CHILD, os.path.join(root, "xfg-stark_amd"), root],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = " ".join(r.stdout.split()).split()
    assert len(got) == 12
    for i in range(12):
        st, want = O.prove(oracle_air(synthetic.burn_inputs(1300 + i)), 1024, O.options())
        assert st == 0 and hashlib.sha256(want).hexdigest() == got[i], i


_INTERLEAVED_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import synthetic, xfgstark
traces, airs = np.load(sys.argv[3]), [tuple(a) for a in json.load(open(sys.argv[4]))]
pr = xfgstark.XfgBurnMintProver()
first = pr.submit_batch([synthetic.burn_inputs(1400 + i) for i in range(5)], trace_length=64)
mid = pr.submit_traces(traces, airs, validate=True)
last = pr.submit_batch([synthetic.burn_inputs(1410 + i) for i in range(4)], trace_length=64)
res = {"last": last.result(), "first": first.result(), "mid": mid.result()}
sha = lambda r: hashlib.sha256(r.to_bytes()).hexdigest()
out = {k: [sha(r) if hasattr(r, "to_bytes") else [r.status, mid._lens[i], list(r.fault.astuple()), str(r)]
           for i, r in enumerate(v)] for k, v in res.items()}
out["one"] = sha(pr.prove_trace(traces[2], *airs[2]))
print(json.dumps(out))
"""


def test_interleaved_batch_kinds_waited_out_of_order(tmp_path):
    """two lanes, 2-proof units halved to 1: a generated batch of 5, a validated host-trace batch of 3 whose
    middle trace breaks the AIR, and a generated batch of 4 are in flight together and waited for as 3rd,
    1st, 2nd; then one xfg_prove_trace on the same context. Every valid proof equals the oracle's, the
    invalid trace has XFG_INVALID_TRACE, length 0 and the reference check's fault, its neighbours are intact"""
    import subprocess
    import sys
    import trace_check_ref as T
    from test_trace_batch_gpu import _flat
    n, root = 64, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    traces, airs = zip(*[T.valid_trace(n, 1420 + i) for i in range(3)])
    traces[1][5][n - 2] = 77  # constraint 5 at the last checked step
    fault = T.first_fault(traces[1], airs[1])
    assert fault == (2, 5, 0, n - 2, 0, 0)
    np.save(tmp_path / "traces.npy", np.stack(traces))
    json.dump(airs, open(tmp_path / "airs.json", "w"))
    env = dict(os.environ, XFG_LANES="2", XFG_UNIT="2", XFG_SPLIT_MIN="1")
    r = subprocess.run([sys.executable, "-c", _INTERLEAVED_CHILD, os.path.join(root, "xfg-stark_amd"), root,
                        str(tmp_path / "traces.npy"), str(tmp_path / "airs.json")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)

    def oracle_sha(air, trace=None):
        st, want = O.prove(air, n, O.options(), **({} if trace is None else {"trace": _flat(trace)}))
        assert st == 0
        return hashlib.sha256(want).hexdigest()
    assert got["first"] == [oracle_sha(oracle_air(synthetic.burn_inputs(1400 + i))) for i in range(5)]
    assert got["last"] == [oracle_sha(oracle_air(synthetic.burn_inputs(1410 + i))) for i in range(4)]
    assert got["mid"][0] == oracle_sha(T.oracle_air(airs[0]), traces[0])
    assert got["mid"][2] == oracle_sha(T.oracle_air(airs[2]), traces[2]) == got["one"]
    assert got["mid"][1] == [11, 0, list(fault), "main transition constraint 5 did not evaluate to ZERO at step 62"]


def test_batch_record_and_consumption_rules(prover):
    """submit_batch_record writes proofs and lengths straight into a caller's fixed-size record (the
    exchange format of bench.Exchange); a batch is consumed once: result() after packed_into() or
    record_ready() raises instead of returning an empty list"""
    import ctypes as C
    import xfgstark
    prover._options = xfgstark.ProofOptions.reference()
    n, k = 1024, 5
    kws = [synthetic.burn_inputs(900 + i) for i in range(k)]
    want = [p.to_bytes() for p in prover.prove_batch(kws, trace_length=n)]
    size = xfgstark.record_size(k, n, prover._options)
    cap = prover.proof_size_bound(n)
    assert size == 8 * k + k * cap
    rec = (C.c_uint8 * size)()
    p = prover.submit_batch_record(kws, n, C.addressof(rec), size)
    assert p.record_ready() == size
    raw = bytes(rec)
    lens = np.frombuffer(raw[:8 * k], dtype=np.int64)
    assert [raw[8 * k + i * cap:8 * k + i * cap + int(lens[i])] for i in range(k)] == want
    with pytest.raises(xfgstark.XfgStarkError):
        p.result()
    with pytest.raises(xfgstark.XfgStarkError):  # too small a record
        prover.submit_batch_record(kws, n, C.addressof(rec), size - 1)
    q = prover.submit_batch(kws, trace_length=n)
    dst = np.zeros(8 * k + sum(map(len, want)), dtype=np.uint8)
    assert q.packed_into(dst) == dst.size
    with pytest.raises(xfgstark.XfgStarkError):
        q.result()
    with pytest.raises(xfgstark.XfgStarkError):
        q.record_ready()
    r = prover.submit_batch(kws, trace_length=n)
    assert [x.to_bytes() for x in r.result()] == want and r.result() is r.result()
    with pytest.raises(xfgstark.XfgStarkError):
        r.packed_into(dst)
    s = prover.submit_batch(kws, trace_length=n)
    free = len(prover._free)
    assert s.wait() == 0
    del s  # waited but never consumed: its buffer returns to the pool
    assert len(prover._free) == free + 1
