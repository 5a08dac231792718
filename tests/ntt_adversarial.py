"""Adversarial inputs for the four-step NTT (xfg-stark_amd/csrc/ntt.hip): TEST INFRASTRUCTURE ONLY.

The NTT keeps butterfly values weakly reduced (any u64 congruent mod p) and canonicalises at a few
places that differ from kernel to kernel. A u64 is non-canonical only in [p, 2^64), 2^32 - 1 values
wide, so random data almost never puts a value there. The DFT is linear and invertible: here the values
wanted at an internal boundary of the transform (the target) are chosen first and pulled back exactly
to the transform's input. Small targets (<= 2^32 - 2) are what an add_w produces as p + s; sparse
targets make the levels before them cancel to 0, held as 0 or as p.

Notation (ntt.hip): p = 2^64 - 2^32 + 1, n = R C, input index j = C j1 + j2, output index
k = k1 + R k2, N = beta n, w_k the oracle's root of order 2^k. Forward, coset t:
    x[j1]      = c[C j1 + j2] o^j1,  o = 7^C w_(beta R)^t        first-step inputs of pass A
    X_j2[k1]   = sum_j1 x[j1] w_R^(j1 k1)                        pass A's column DFTs
    y[k1][j2]  = X_j2[k1] 7^j2 w_N^(j2 (t + beta k1))            first-step inputs of pass B
    out[t][k]  = sum_j2 y[k1][j2] w_C^(j2 k2)
Inverse: x = e, X_j2[k1] = sum_j1 e[C j1 + j2] w_R^-(j1 k1), y = X w_n^-(j2 k1) / n (the table carries
1 / n), out[k] = sum_j2 y[k1][j2] w_C^-(j2 k2) (times 7^-k with off7).
The first Stockham step of a size-S pass with first radix R1 (G = S / R1 groups) turns the inputs
in[j + r G] of group j into Z_j[q] = sum_r in[j + r G] w_R1^(+-r q), kept at position j R1 + q.

Boundaries (each target is pulled back to the transform's input):
    out      the transform's outputs: plane t of the LDE [n], or the coefficients [n]
    pass     X[k1][j2]        [R][C]   (ntt_pass_a_r1024: X s_t(j2), what its last butterflies hold)
    step_a   Z_j[q] of pass A [R][C], row j R1 + q
    step_b   Z_j[q] of pass B [R][C], column j R1 + q of row k1
    in_a     x[j1][j2]        [R][C]   (what the first butterflies of pass A load)
    in_b     y[k1][j2]        [R][C]
ntt_pass_a_cos2 and ntt_pass_a_r1024 move the group part o^j0 of the pre-factor (j1 = j0 + r G) onto the
second step's twiddles, so their first step sees c o^(r G) (r1024: times s_t(j2) = 7^j2 w_N^(j2 t)):
`variant` selects that model for in_a and step_a.

All arithmetic is vectorised: numpy on 32-bit limbs (mulmod) and the oracle's C transforms."""
import ctypes as C

import numpy as np

import oracle_lib as O

P = (1 << 64) - (1 << 32) + 1
_EPS = np.uint64(0xFFFFFFFF)
_P = np.uint64(P)
_U64P = C.POINTER(C.c_uint64)
BOUNDARIES = ("out", "pass", "step_a", "step_b", "in_a", "in_b")


# ---------------------------------------------------------------- Goldilocks on numpy uint64
def _u64(a):
    return np.atleast_1d(np.asarray(a, dtype=np.uint64))


def _chunked(f, a, b):
    """f(a, b) elementwise over the broadcast of a and b, in slices of about 2^15 elements along the
    longest axis: the dozens of temporaries of one slice then stay in the cache"""
    a, b = np.broadcast_arrays(_u64(a), _u64(b))
    if a.size <= 1 << 16:
        return f(a, b)
    out = np.empty(a.shape, dtype=np.uint64)
    ax = int(np.argmax(a.shape))
    am, bm, om = np.moveaxis(a, ax, 0), np.moveaxis(b, ax, 0), np.moveaxis(out, ax, 0)
    step = max(1, (1 << 15) // (a.size // a.shape[ax]))
    for i in range(0, a.shape[ax], step):
        om[i:i + step] = f(am[i:i + step], bm[i:i + step])
    return out


def _mulmod(a, b):
    a0, a1, b0, b1 = a & _EPS, a >> np.uint64(32), b & _EPS, b >> np.uint64(32)
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (ll >> np.uint64(32)) + (lh & _EPS) + (hl & _EPS)  # < 3 2^32
    lo = (ll & _EPS) | ((mid & _EPS) << np.uint64(32))
    hi = hh + (lh >> np.uint64(32)) + (hl >> np.uint64(32)) + (mid >> np.uint64(32))
    # lo + hi_lo 2^64 + hi_hi 2^96 = lo - hi_hi + hi_lo (2^32 - 1)  (2^64 = 2^32 - 1, 2^96 = -1)
    h1, h0 = hi >> np.uint64(32), hi & _EPS
    t = lo - h1
    t = np.where(lo < h1, t - _EPS, t)  # borrow: + p = + 2^64 - (2^32 - 1); t >= 2^64 - 2^32 before it
    m = h0 * _EPS
    r = t + m
    r = np.where(r < m, r + _EPS, r)  # carry: 2^64 = 2^32 - 1; r <= 2^64 - 2^33 before it
    return np.where(r >= _P, r - _P, r)


def mulmod(a, b):
    """a b mod p, elementwise, for any u64 operands; canonical result"""
    return _chunked(_mulmod, a, b)


def _addmod(a, b):
    s = a + b
    s = np.where(s < a, s + _EPS, s)
    return np.where(s >= _P, s - _P, s)


def _submod(a, b):
    return np.where(a < b, a - b - _EPS, a - b)


def addmod(a, b):
    """canonical operands"""
    return _chunked(_addmod, a, b)


def submod(a, b):
    """canonical operands"""
    return _chunked(_submod, a, b)


def root(k):
    """the oracle's root of unity of order 2^k"""
    return int(O.lib().orc_field_root(k))


def inv(x):
    return pow(int(x), P - 2, P)


def pow_table(base, count):
    """[base^0 .. base^(count - 1)], by doubling"""
    t = np.ones(1, dtype=np.uint64)
    while t.size < count:
        t = np.concatenate([t, mulmod(t, np.uint64(pow(int(base), t.size, P)))])
    return t[:count]


def pow_of(base, e, bits):
    """base^e for an array of exponents below 2^bits: two table look-ups and one multiply"""
    e = _u64(e)
    lo_bits = (bits + 1) // 2
    lo = pow_table(base, 1 << lo_bits)
    hi = pow_table(pow(int(base), 1 << lo_bits, P), 1 << max(bits - lo_bits, 0))
    return mulmod(lo[e & np.uint64((1 << lo_bits) - 1)], hi[e >> np.uint64(lo_bits)])


def dft_axis0(x, w):
    """X[q] = sum_r x[r] w^(r q) along axis 0 (length a power of two, w of that order), radix 2"""
    m = x.shape[0]
    if m == 1:
        return x
    w2 = w * w % P
    ev, od = dft_axis0(x[0::2], w2), dft_axis0(x[1::2], w2)
    tw = pow_table(w, m // 2).reshape((-1,) + (1,) * (x.ndim - 1))
    od = mulmod(od, tw)
    return np.concatenate([addmod(ev, od).reshape(ev.shape), submod(ev, od).reshape(ev.shape)])


def _rows_interpolate(rows, offset):
    """orc_interpolate of every row of a [count][S] array, in place"""
    assert rows.flags.c_contiguous and rows.dtype == np.uint64
    L, S, base = O.lib(), rows.shape[1], rows.ctypes.data
    for i in range(rows.shape[0]):
        L.orc_interpolate(C.cast(base + i * S * 8, _U64P), S, offset)
    return rows


def _rows_evaluate(rows):
    """orc_evaluate_lde(row, S, 1, 1) of every row of a [count][S] array"""
    assert rows.flags.c_contiguous and rows.dtype == np.uint64
    out = np.empty_like(rows)
    L, S, a, b = O.lib(), rows.shape[1], rows.ctypes.data, out.ctypes.data
    for i in range(rows.shape[0]):
        L.orc_evaluate_lde(C.cast(a + i * S * 8, _U64P), S, 1, 1, C.cast(b + i * S * 8, _U64P))
    return out


# ---------------------------------------------------------------- geometry of one transform
class Geometry:
    """One transform and where its boundaries lie. Forward: coset t of 2^logbeta, or plane tsub of
    sub-transform u of a composed LDE of g blowup-16 transforms (coefficients twisted by w_N^(u j), N =
    16 g n). first_a / first_b: log2 of the first radix of pass A / B (step boundaries only)."""

    def __init__(self, direction, logn, logr, logc, logbeta=0, t=0, off7=False, first_a=None, first_b=None,
                 variant="plain", u=0, g=1):
        assert direction in ("fwd", "inv") and logr + logc == logn and variant in ("plain", "cos2", "r1024")
        self.fwd, self.logn, self.logr, self.logc = direction == "fwd", logn, logr, logc
        self.logbeta, self.t, self.off7 = (logbeta if self.fwd else 0), (t if self.fwd else 0), off7
        self.first_a, self.first_b, self.variant, self.u, self.g = first_a, first_b, variant, u, g
        self.n, self.R, self.Cc = 1 << logn, 1 << logr, 1 << logc
        self.logN = logn + self.logbeta  # of this (sub-)transform
        if self.fwd:
            self.o = pow(7, self.Cc, P) * pow(root(self.logbeta + logr), self.t, P) % P

    def fourstep_inv(self):
        """X / y [R][C]: forward 1 / (7^j2 w_N^(j2 (t + beta k1))), inverse n w_n^(j2 k1). Row k1 is row 0
        times w_n^(-+j2 k1): the rows double, row m + k1 = row k1 times (w_n^(-+m))^j2"""
        wn = inv(root(self.logn)) if self.fwd else root(self.logn)
        rows = (self.seed_inv() if self.fwd else np.full(self.Cc, self.n % P, dtype=np.uint64)).reshape(1, -1)
        while rows.shape[0] < self.R:
            step = pow_table(pow(wn, rows.shape[0], P), self.Cc).reshape(1, -1)
            rows = np.concatenate([rows, mulmod(rows, step)])
        return rows

    def seed_inv(self):
        """1 / s_t(j2), s_t(j2) = 7^j2 w_N^(j2 t) [C]"""
        return pow_table(inv(7 * pow(root(self.logN), self.t, P) % P), self.Cc)

    def prefactor_inv(self):
        """c / x as the first step of pass A sees x (forward): [R][1] or [R][C]"""
        j1 = np.arange(self.R)
        if self.variant == "plain":
            return pow_table(inv(self.o), self.R).reshape(-1, 1)
        G = self.R >> self.first_a
        f = pow_table(inv(self.o), self.R)[j1 - j1 % G].reshape(-1, 1)
        return mulmod(f, self.seed_inv().reshape(1, -1)) if self.variant == "r1024" else f


def _unstep(z, logr1, inverse_dft, axis):
    """the inputs in[j + r G] of every first-step group from its outputs Z_j[q] at j R1 + q along `axis`"""
    z = np.moveaxis(z, axis, 0)
    S, R1 = z.shape[0], 1 << logr1
    G = S // R1
    zq = np.moveaxis(z.reshape((G, R1) + z.shape[1:]), 1, 0)  # [q][j]...
    w = root(logr1) if logr1 else 1
    # Z = sum_r in_r w^(+-r q)  ->  in_r = 1/R1 sum_q Z_q w^(-+r q)
    x = dft_axis0(np.ascontiguousarray(zq), w if inverse_dft else inv(w))
    x = mulmod(x, np.uint64(inv(R1))).reshape((R1, G) + z.shape[1:])  # [r][j] -> row r G + j
    return np.moveaxis(x.reshape(z.shape), 0, axis)


def pull_back(geo, boundary, target):
    """the transform's input [n] (coefficients forward, evaluations inverse) for which the values at
    `boundary` equal `target` ([n] for out, [R][C] otherwise; canonical values)"""
    target = np.ascontiguousarray(target, dtype=np.uint64)
    n, R, Cc = geo.n, geo.R, geo.Cc
    if boundary == "out":
        assert target.shape == (n,)
        if geo.fwd:  # the natural coset of the whole LDE: u + g t of N = g 2^logN
            logg = geo.g.bit_length() - 1
            return O.interpolate_np(target, 7 * pow(root(geo.logN + logg), geo.u + geo.g * geo.t, P) % P)
        return O.evaluate_lde_np(target, 1, 7 if geo.off7 else 1)
    else:
        assert target.shape == (R, Cc) and boundary in BOUNDARIES
        v = target
        if boundary == "step_b":
            v = _unstep(v, geo.first_b, not geo.fwd, 1).reshape(R, Cc)
            boundary = "in_b"
        if boundary == "in_b":
            v = mulmod(v, geo.fourstep_inv())
            boundary = "pass"
        elif boundary == "pass" and geo.variant == "r1024":
            v = mulmod(v, geo.seed_inv().reshape(1, -1))
        if boundary == "pass":
            cols = np.ascontiguousarray(v.T)  # [j2][k1]
            if geo.fwd:
                c = np.ascontiguousarray(_rows_interpolate(cols, geo.o).T).reshape(n)
            else:
                return np.ascontiguousarray(_rows_evaluate(mulmod(cols, np.uint64(inv(R))).reshape(Cc, R)).T).reshape(n)
        else:
            if boundary == "step_a":
                v = _unstep(v, geo.first_a, not geo.fwd, 0).reshape(R, Cc)
            if not geo.fwd:
                return np.ascontiguousarray(v).reshape(n)
            c = mulmod(v, geo.prefactor_inv()).reshape(n)
    if geo.u:  # sub-transform u of a composed LDE reads c_j w_N^(u j), N = 16 g n
        logN = geo.logN + (geo.g.bit_length() - 1)
        c = mulmod(c, pow_table(pow(inv(root(logN)), geo.u, P), n))
    return c


# ---------------------------------------------------------------- target value sets
_SMALL_FIXED = np.array([0, 1, 2, 1 << 31, (1 << 32) - 2], dtype=np.uint64)


def small(shape, rng):
    """every entry <= 2^32 - 2: {0, 1, 2, 2^31, 2^32 - 2} and random values below 2^32 - 1"""
    r = rng.integers(0, (1 << 32) - 1, size=shape, dtype=np.uint64)
    return np.where(rng.random(shape) < 0.4, rng.choice(_SMALL_FIXED, size=shape), r)


def neg(shape, rng):
    """p - s for s of small(), s != 0"""
    return _P - np.maximum(small(shape, rng), np.uint64(1))


def sparse(shape, rng, case=None, R=None, Cc=None):
    """zero except at 1 to 3 positions (of the flattened array) holding 1, p - 1 or a random value.
    case 0: the single position 0; case 1: the single last position; case 2: C - 1 and n / 2 (all low
    digits set, and the top digit); case 3: 1, R and n - 1 (a low digit, a middle one, all of them)"""
    n = int(np.prod(shape))
    out = np.zeros(n, dtype=np.uint64)
    vals = [1, P - 1, int(rng.integers(0, P, dtype=np.uint64))]
    case = int(rng.integers(0, 4)) if case is None else case
    R, Cc = R or 2, Cc or 4
    pos = {0: [0], 1: [n - 1], 2: [(Cc - 1) % n, n // 2], 3: [1, R % n, n - 1]}[case]
    assert len(set(pos)) == len(pos)
    for i, q in enumerate(pos):
        out[int(q)] = vals[int(rng.integers(0, 3)) if len(pos) == 1 else i % 3]
    return out.reshape(shape)


def mixed(shape, rng):
    """small() alternating with random canonical values"""
    a, b = small(shape, rng), rng.integers(0, P, size=shape, dtype=np.uint64)
    return np.where(np.arange(int(np.prod(shape))).reshape(shape) % 2 == 0, a, b)


def _brev(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def cancel(shape, rng, logr1, axis):
    """first-step INPUTS (boundaries in_a, in_b) that put a value p + s in front of a w = 1 subtrahend
    of level 1 or 2 of the radix-2^logr1 butterfly network, next to a minuend below s. dft_reg orders its
    registers bit-reversed (a[i] = in[brev(i)]): a[4m .. 4m + 3] = (0, 0, p - 1, 1 + s) makes level 0 leave
    (0, 0, p + s, ..), and level 1 subtracts a[4m + 2] from a[4m]: a subtrahend taken without
    canonicalisation borrows twice. a[8m .. 8m + 7] = (0, 0, 0, 0, p - 1, 0, 1 + s, 0) does the same one
    level up. Groups lie along `axis` of the [R][C] array: element r of group j at j + r G. A radix-2 first
    step has level 0 only, so nothing to cancel: it gets neg() values."""
    R, Cc = shape
    S = shape[axis]
    R1 = 1 << logr1
    G, other = S // R1, shape[1 - axis]
    a = np.zeros((R1, G, other), dtype=np.uint64)  # [a-index][group][line]
    if R1 >= 4:
        for m in range(0, R1, 8 if R1 >= 8 else 4):
            kind = rng.integers(0, 3, size=(G, other)) if R1 >= 8 else np.zeros((G, other), dtype=np.int64)
            s = rng.integers(1, (1 << 32) - 2, size=(G, other), dtype=np.uint64)
            pm1, s1 = np.full((G, other), P - 1, dtype=np.uint64), s + np.uint64(1)
            # kind 0: the level-1 pattern in a[m .. m + 3] (and again in a[m + 4 .. m + 7]);
            # kind 1: the level-2 pattern; kind 2: small values
            a[m + 2] = np.where(kind == 0, pm1, 0)
            a[m + 3] = np.where(kind == 0, s1, 0)
            if R1 >= 8:
                a[m + 4] = np.where(kind == 1, pm1, 0)
                a[m + 6] = np.where(kind == 0, pm1, np.where(kind == 1, s1, 0))
                a[m + 7] = np.where(kind == 0, s1, 0)
                sm = small((G, other), rng)
                for i in range(8):
                    a[m + i] = np.where(kind == 2, np.roll(sm, i, axis=0), a[m + i])
    else:
        a[:] = neg(a.shape, rng)
    x = np.empty_like(a)  # [r][group][line]
    for i in range(R1):
        x[_brev(i, logr1)] = a[i]
    x = x.reshape(S, other)  # element r of group j at r G + j
    return x if axis == 0 else np.ascontiguousarray(x.T)


TARGET_SETS = ("SMALL", "NEG", "SPARSE", "MIXED")


def make_target(name, geo, boundary, rng, case=None):
    shape = (geo.n,) if boundary == "out" else (geo.R, geo.Cc)
    if name == "SMALL":
        return small(shape, rng)
    if name == "NEG":
        return neg(shape, rng)
    if name == "MIXED":
        return mixed(shape, rng)
    if name == "SPARSE":
        return sparse(shape, rng, case, geo.R, geo.Cc)
    assert name == "CANCEL" and boundary in ("in_a", "in_b")
    return cancel(shape, rng, geo.first_a if boundary == "in_a" else geo.first_b, 0 if boundary == "in_a" else 1)
