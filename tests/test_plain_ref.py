"""CPU self-checks of tests/plain_ref.py: the references the GPU kernel tests compare against must
themselves satisfy the identities of the protocol (no GPU, no library code)."""
import random

import pytest

import oracle_lib as O
import plain_ref as R
import synthetic

P = R.P


def _rand_e(rng):
    return (rng.randrange(P), rng.randrange(P))


def _oracle_air(air):
    a = O.Air()
    a.pub = (O.C.c_uint64 * 12)(*air[0])
    a.nullifier, a.commitment = air[1], air[2]
    return a


def test_root_and_field_match_oracle():
    for k in range(1, 33):
        assert R.root(k) == O.lib().orc_field_root(k)
        assert pow(R.root(k), 1 << k, P) == 1 and pow(R.root(k), 1 << (k - 1), P) == P - 1
    rng = random.Random(1)
    for _ in range(200):
        a, b = rng.randrange(P), rng.randrange(P)
        assert O.lib().orc_field_mul(a, b) == a * b % P


def test_extension_product_is_a_ring_with_phi2_eq_phi_minus_2():
    """no oracle-side E product is reachable through the committed KATs, so the schoolbook rule is
    checked through its defining relation and the ring laws on random triples"""
    phi = (0, 1)
    assert R.e_mul(phi, phi) == R.e_sub(phi, (2, 0))
    rng = random.Random(2)
    for _ in range(300):
        x, y, z = _rand_e(rng), _rand_e(rng), _rand_e(rng)
        assert R.e_mul(x, y) == R.e_mul(y, x)
        assert R.e_mul(R.e_mul(x, y), z) == R.e_mul(x, R.e_mul(y, z))
        assert R.e_mul(x, R.e_add(y, z)) == R.e_add(R.e_mul(x, y), R.e_mul(x, z))
        assert R.e_mul(x, (1, 0)) == x and R.e_mul(x, (0, 0)) == (0, 0)
        assert R.e_mul(x, (y[0], 0)) == R.e_scale(x, y[0])
    # the conjugate (a0 + a1) - a1 phi: x * conj(x) is the norm a0^2 + a0 a1 + 2 a1^2, in the base field
    for _ in range(100):
        a0, a1 = _rand_e(rng)
        assert R.e_mul((a0, a1), ((a0 + a1) % P, (P - a1) % P)) == ((a0 * a0 + a0 * a1 + 2 * a1 * a1) % P, 0)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("D,beta", [(64, 2), (128, 8), (256, 16), (512, 8)])
def test_fold_reference_divides_the_degree_by_eight(D, beta, ext):
    """f of degree < D / beta evaluated over 7 <w_D>, folded with alpha: the D/8 values, read over the
    next layer's domain as the product uses it -- fri_fold_kernel folds layer l + 1 at x = 7 w^i and
    the remainder is interpolated with offset 7, i.e. every layer lives on 7 <w_(D/8)> -- interpolate
    to degree < D / (8 beta). Exactly: f(x) = sum_j x^j f_j(x^8) folds to g = sum_j alpha^j f_j at
    x^8 = 7^8 w_(D/8)^i, so over 7 <w_(D/8)> the coefficients are g_k 7^(7k)."""
    rng = random.Random(D * 10 + beta + ext)
    d = D // beta
    f = [_rand_e(rng) if ext == 2 else (rng.randrange(P), 0) for _ in range(d)]
    alpha = _rand_e(rng) if ext == 2 else (rng.randrange(P), 0)
    planes = [O.evaluate_lde([c[k] for c in f], beta, R.GEN) for k in range(2)]
    vals = list(zip(*planes))
    folded = R.fold_layer(vals, D, alpha)
    layer = [folded[i] for i in range(D // 8)]
    next_offset = R.GEN  # the offset of every FRI layer's domain in the product (and in Winterfell)
    got = list(zip(*[O.interpolate([v[k] for v in layer], next_offset) for k in range(2)]))
    want = []
    for k in range(D // 8):
        g, apow = (0, 0), (1, 0)
        for j in range(8):
            if 8 * k + j < d:
                g = R.e_add(g, R.e_mul(apow, f[8 * k + j]))
            apow = R.e_mul(apow, alpha)
        want.append(R.e_scale(g, pow(R.GEN, 7 * k, P)))
    assert all(c == (0, 0) for c in got[d // 8:])
    assert got == want
    if ext == 1:
        assert all(v[1] == 0 for v in layer)


def test_coset_major_layout_roundtrip():
    n, beta = 16, 4
    nat = list(range(n * beta))
    cm = R.to_coset_major(nat, n, beta)
    assert sorted(cm) == nat
    for K in nat:
        assert cm[(K % beta) * n + K // beta] == K


def test_transition_reference_matches_oracle():
    rng = random.Random(3)
    for t in range(200):
        air = R.WIDE_AIR if t % 2 else R.small_air(t)
        pick = (lambda: rng.choice(R.EDGE_CELLS)) if t % 3 == 0 else (lambda: rng.randrange(P))
        cur, nxt = [pick() for _ in range(7)], [pick() for _ in range(7)]
        assert R.transition(air, cur, nxt) == O.eval_transition(_oracle_air(air), cur, nxt)


@pytest.mark.parametrize("src,n", [(0, 8), (5, 64), ("package", 256)])
def test_constraint_reference_on_a_valid_trace_has_degree_below_n(src, n):
    """valid burn trace, random E coefficients: every constraint vanishes where its divisor does, so
    the 2n evaluations interpolate (over 7 <w_2n>) to a polynomial whose upper n coefficients are
    zero -- transition degree 2 (n - 1) + 1 - n = n - 1, boundary n - 2"""
    kw = synthetic.REFERENCE_PACKAGE if src == "package" else synthetic.burn_inputs(src)
    st, oa = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                               kw["secret"])
    assert st == 0
    air = (list(oa.pub), oa.nullifier, oa.commitment)
    flat = list(O.build_trace(oa, n))
    trace = [flat[c * n:(c + 1) * n] for c in range(7)]
    rng = random.Random(n)
    coeffs = [_rand_e(rng) for _ in range(15)]
    ce = R.constraint_evals(trace, air, coeffs)
    for k in range(2):
        co = O.interpolate([v[k] for v in ce], R.GEN)
        assert any(co[:n]) and not any(co[n:])


def test_constraint_reference_on_an_invalid_trace_has_full_degree():
    """the same check must fail for a false statement, else it says nothing"""
    tr, air = R.make_trace("random", 16, 4)
    rng = random.Random(5)
    ce = R.constraint_evals(tr, air, [(rng.randrange(P), 0) for _ in range(15)])
    assert any(O.interpolate([v[0] for v in ce], R.GEN)[16:])
    assert all(v[1] == 0 for v in ce)


@pytest.mark.parametrize("kind", ["random", "edge", "wide_consts"])
def test_trace_generators_are_canonical_and_seeded(kind):
    a, air = R.make_trace(kind, 64, 9)
    b, _ = R.make_trace(kind, 64, 9)
    assert a == b and all(0 <= v < P for col in a for v in col)
    assert all(v < P for v in air[0]) and air[1] < P and air[2] < P
