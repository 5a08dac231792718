"""Plain references for the kernel-level parity tests: Python integers modulo p = 2^64 - 2^32 + 1.

TEST INFRASTRUCTURE ONLY. Nothing here shares code with the library: the quadratic extension is the
schoolbook product for phi^2 = phi - 2 (not the Karatsuba form of gl.hpp's e2_mul), inverses are
pow(x, -1, p), the FRI fold is a Lagrange interpolation through the eight points of a row, and the
constraint evaluation restates oracle/orc_stark.c's loop (air_transition, air_assertions, the three
divisors) point by point. Only the NTTs behind the constraint reference come from the oracle
(orc_interpolate / orc_evaluate_lde, pinned by test_oracle_kats.py). tests/test_plain_ref.py checks
these references against identities they must satisfy, on the CPU.

Elements of E are 2-tuples (a0, a1) = a0 + a1 phi; base-field values are the tuples (a, 0).
"""
import random

P = (1 << 64) - (1 << 32) + 1
GEN = 7  # multiplicative generator, Winterfell's domain offset
STD_BURN = 8000000
LARGE_BURN = 8000000 * 1000

# boundary values of the field and of the AIR (burn amounts) used by the edge-valued inputs
EDGE_CELLS = [0, 1, P - 1, P - 2, STD_BURN, LARGE_BURN, (1 << 32) - 1, 1 << 32, (1 << 64) - (1 << 32)]


def root(k):
    """primitive 2^k-th root of unity (winter-math get_root_of_unity: 7^((p - 1) / 2^k))"""
    return pow(GEN, (P - 1) >> k, P)


# ---- quadratic extension, schoolbook
def e_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def e_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def e_mul(x, y):
    """(a0 + a1 phi)(b0 + b1 phi) = (a0 b0 - 2 a1 b1) + (a0 b1 + a1 b0 + a1 b1) phi"""
    a0, a1 = x
    b0, b1 = y
    return ((a0 * b0 - 2 * a1 * b1) % P, (a0 * b1 + a1 * b0 + a1 * b1) % P)


def e_scale(x, s):
    return (x[0] * s % P, x[1] * s % P)


# ---- FRI fold (folding factor 8, every layer over the coset 7 <w_D>)
def fold_row(v, i, D, alpha):
    """the value the fold gives row i of a D-point layer: v[k] (E) is the layer's value at
    x_k = 7 w_D^(i + k D/8), k < 8; the polynomial of degree < 8 through (x_k, v[k]) is evaluated at
    alpha (E) by Lagrange's formula"""
    w = root(D.bit_length() - 1)
    xs = [GEN * pow(w, i + k * (D // 8), P) % P for k in range(8)]
    acc = (0, 0)
    for k in range(8):
        num, den = (1, 0), 1
        for j in range(8):
            if j != k:
                num = e_mul(num, e_sub(alpha, (xs[j], 0)))
                den = den * (xs[k] - xs[j]) % P
        acc = e_add(acc, e_mul(e_scale(num, pow(den, -1, P)), v[k]))
    return acc


def fold_layer(vals, D, alpha, rows=None):
    """vals: D E-values in natural order (index K <-> 7 w_D^K); -> {row: folded value} for `rows`
    (all D/8 by default)"""
    R = D // 8
    return {i: fold_row([vals[i + k * R] for k in range(8)], i, D, alpha) for i in (range(R) if rows is None else rows)}


def to_coset_major(vals, n, beta):
    """natural order -> the first layer's storage: natural index K at (K mod beta) n + K // beta"""
    out = [None] * (n * beta)
    for K, v in enumerate(vals):
        out[(K % beta) * n + K // beta] = v
    return out


# ---- AIR: XfgBurnMintAir transition constraints and assertions (oracle/orc_stark.c air_transition,
# air_assertions); air = (pub[12], nullifier, commitment)
def transition(air, cur, nxt):
    pub, nullifier, commitment = air
    d = (nxt[4] - cur[4]) % P
    return [(cur[0] - STD_BURN) * (cur[0] - LARGE_BURN) % P,
            (cur[1] - cur[0]) % P,
            (cur[2] - (pub[2] & 0xFFFFFFFF)) % P,
            (cur[3] - (pub[3] & 0xFFFFFFFF)) % P,
            d * (d - 1) % P,
            (cur[5] - nullifier) % P,
            (cur[6] - commitment) % P]


def assertions(air, n):
    """[(column, step, value)]: step 0 on every column, step n - 1 on column 4"""
    pub, nullifier, commitment = air
    v0 = [pub[0], pub[1], pub[2], pub[3], 0, nullifier, commitment]
    return [(c, 0, v0[c]) for c in range(7)] + [(4, n - 1, 3)]


def constraint_evals(trace, air, coeffs):
    """composition evaluations over the CE domain: trace = 7 columns of n values, coeffs = 15 E
    elements (7 transition, 7 step-0 boundary, 1 final-step) -> 2n E values, index i <-> x = 7 w_2n^i:
      t (x - g^(n-1)) / (x^n - 1) + b0 / (x - 1) + b1 / (x - g^(n-1))
    with t, b0, b1 the coefficient-weighted sums of the transition expressions and of the assertion
    numerators at steps 0 and n - 1. Column values at x and at x g come from the oracle's LDE at
    blowup 2 (the next row of CE index i is index i + 2)."""
    import oracle_lib as O
    n = len(trace[0])
    nce = 2 * n
    logn = n.bit_length() - 1
    cols = [O.evaluate_lde(O.interpolate([int(v) for v in col], 1), 2, GEN) for col in trace]
    g_last = pow(root(logn), n - 1, P)
    w = root(logn + 1)
    asr = assertions(air, n)
    out = []
    for i in range(nce):
        x = GEN * pow(w, i, P) % P
        cur = [cols[c][i] for c in range(7)]
        nxt = [cols[c][(i + 2) % nce] for c in range(7)]
        r = transition(air, cur, nxt)
        t, b0, b1 = (0, 0), (0, 0), (0, 0)
        for c in range(7):
            t = e_add(t, e_scale(coeffs[c], r[c]))
        for a, (col, step, val) in enumerate(asr):
            term = e_scale(coeffs[7 + a], (cur[col] - val) % P)
            if step == 0:
                b0 = e_add(b0, term)
            else:
                b1 = e_add(b1, term)
        acc = e_scale(t, (x - g_last) * pow(pow(x, n, P) - 1, -1, P) % P)
        acc = e_add(acc, e_scale(b0, pow(x - 1, -1, P)))
        acc = e_add(acc, e_scale(b1, pow(x - g_last, -1, P)))
        out.append(acc)
    return out


# ---- seeded inputs of the arbitrary-trace tests (the same generators on the CPU and the GPU side)
WIDE_PUB = [STD_BURN, (1 << 63) + 11, P - 1, (1 << 63) + 5, 0xFFFFFFFF00000000, 0x123456789ABCDEF0, 1 << 32,
            (1 << 32) - 1, P - 2, 0x8000000080000001, 0xFEDCBA9876543210, 0xFFFFFFFE00000002]
WIDE_AIR = (WIDE_PUB, P - 1, (1 << 64) - (1 << 32))
assert len(WIDE_PUB) == 12 and all(v < P for v in WIDE_PUB)


def small_air(seed):
    """AIR constants below 2^32, as every burn input gives them"""
    rng = random.Random(seed)
    return ([rng.randrange(1 << 32) for _ in range(12)], rng.randrange(1 << 32), rng.randrange(1 << 32))


def make_trace(kind, n, seed):
    """(trace: 7 lists of n canonical values, air) for kind in random / edge / wide_consts"""
    rng = random.Random(seed)
    if kind == "random":
        return [[rng.randrange(P) for _ in range(n)] for _ in range(7)], small_air(seed + 1)
    if kind == "edge":
        tr = [[rng.choice(EDGE_CELLS) for _ in range(n)] for _ in range(7)]
        for c in (0, 2, 5):  # constant columns, one edge value each
            tr[c] = [rng.choice(EDGE_CELLS)] * n
        tr[4] = [rng.choice([0, 1, 2, 3, P - 1]) for _ in range(n)]  # d and d - 1 hit 0, 1 and p - 1
        return tr, small_air(seed + 1)
    if kind == "wide_consts":
        tr = [[rng.randrange(P) for _ in range(n)] for _ in range(7)]
        tr[5] = [0] * n
        tr[6] = [P - 1] * n
        tr[2] = [WIDE_PUB[2] & 0xFFFFFFFF] * n
        return tr, WIDE_AIR
    raise ValueError(kind)
