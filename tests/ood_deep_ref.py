"""Plain references for the OOD frame and the DEEP quotient (ood_kernel, ood_final_kernel,
deep_coin_block, deep_carry_kernel, deep_final_kernel), in the base field and in the quadratic extension.

TEST INFRASTRUCTURE ONLY. Python integers and plain_ref's schoolbook e_mul; nothing is shared with the
library. Elements of E are 2-tuples, base-field values the tuples (a, 0), and the base-field case is the
same code on such tuples. The inverse is x^(p^2 - 2) by square-and-multiply in E (gl.hpp takes the
conjugate and one base-field inversion).

A case is: co = 7 trace polynomials of n base-field coefficients, h = the composition polynomial of n E
coefficients, the points z and zg, the coefficients a[7] and gamma in E. Then
  frame = [T_0(z), T_0(zg), ..., T_6(z), T_6(zg), H(z)],
  c1 = sum a_c T_c(z) + gamma H(z),  c2 = sum a_c T_c(zg),
  P1 = sum a_c T_c + gamma H,  P2 = sum a_c T_c,
  d = (P1 - c1) / (x - z) + (P2 - c2) / (x - zg)   (n coefficients, the last one zero).
The dense reference is Horner's rule and two synthetic divisions over lists. The sparse one takes the
polynomials as {index: coefficient} with few entries, so that n = 2^21 stays affordable: the frame is a
short sum of powers, and only the division recurrences run over all n with one product each. Both assert
that the two division remainders vanish. tests/test_ood_deep_ref.py checks them on the CPU.
"""
from plain_ref import P, e_add, e_mul, e_scale, e_sub, root

ZERO, ONE = (0, 0), (1, 0)
BLOCK = 2048  # coefficients per block of the OOD / DEEP kernels (256 threads x 8), n / 8 threads below that


def e_pow(x, e):
    r = ONE
    while e:
        if e & 1:
            r = e_mul(r, x)
        x = e_mul(x, x)
        e >>= 1
    return r


def e_inv(x):
    """x^(p^2 - 2): the multiplicative group of E has p^2 - 1 elements"""
    assert x != ZERO
    return e_pow(x, P * P - 2)


def rand_e(rng, ext):
    return (rng.randrange(P), rng.randrange(P) if ext == 2 else 0)


def horner(poly, x):
    """poly: E coefficients, lowest first"""
    acc = ZERO
    for v in reversed(poly):
        acc = e_add(e_mul(acc, x), v)
    return acc


def horner_base(poly, x):
    """poly: base-field coefficients (ints)"""
    acc = ZERO
    for v in reversed(poly):
        acc = e_mul(acc, x)
        acc = ((acc[0] + v) % P, acc[1])
    return acc


def deep_constants(frame, a, gam):
    c1, c2 = e_mul(gam, frame[14]), ZERO
    for c in range(7):
        c1 = e_add(c1, e_mul(a[c], frame[2 * c]))
        c2 = e_add(c2, e_mul(a[c], frame[2 * c + 1]))
    return c1, c2


# ---- dense
def frame_dense(co, h, z, zg):
    frame = []
    for c in range(7):
        frame += [horner_base(co[c], z), horner_base(co[c], zg)]
    frame.append(horner(h, z))
    return frame


def combine_dense(co, h, a, gam):
    """(P1, P2) before their constant terms are shifted"""
    n = len(h)
    p2 = [(sum(a[c][0] * co[c][j] for c in range(7)) % P, sum(a[c][1] * co[c][j] for c in range(7)) % P)
          for j in range(n)]
    p1 = [e_add(p2[j], e_mul(gam, h[j])) for j in range(n)]
    return p1, p2


def deep_dense(co, h, z, zg, a, gam, frame=None):
    """-> (frame, d): d = n E coefficients of the DEEP composition polynomial"""
    n = len(h)
    if frame is None:
        frame = frame_dense(co, h, z, zg)
    c1, c2 = deep_constants(frame, a, gam)
    p1, p2 = combine_dense(co, h, a, gam)
    p1[0] = e_sub(p1[0], c1)
    p2[0] = e_sub(p2[0], c2)
    q1, q2, d = ZERO, ZERO, [ZERO] * n
    for k in range(n - 2, -1, -1):
        q1 = e_add(p1[k + 1], e_mul(z, q1))
        q2 = e_add(p2[k + 1], e_mul(zg, q2))
        d[k] = e_add(q1, q2)
    assert e_add(p1[0], e_mul(z, q1)) == ZERO, "remainder of the division by (x - z)"
    assert e_add(p2[0], e_mul(zg, q2)) == ZERO, "remainder of the division by (x - zg)"
    return frame, d


def planes(vals, ext):
    """E values -> ext coordinate lists; a base-field case must have stayed in the base field"""
    if ext == 1:
        assert all(v[1] == 0 for v in vals)
    return [[v[k] for v in vals] for k in range(ext)]


# ---- sparse
def sparse_indices(n, rng, extra=64):
    """where the long polynomials are non-zero: both ends, the first and last index of every block, both
    sides of every thread's 8-coefficient chunk in one block, and `extra` random places"""
    ch = min(BLOCK, n)
    s = {0, 1, n - 2, n - 1}
    for b in range(0, n, ch):
        s |= {b, b + ch - 1}
    base = rng.randrange(n // ch) * ch
    for m in range(ch // 8):
        s |= {base + 8 * m, max(base + 8 * m - 1, 0)}
    s |= {rng.randrange(n) for _ in range(extra)}
    return sorted(s)


def sparse_eval(terms, x):
    """sum v x^j over terms = {j: v} (v in E): Horner over the gaps between the indices, with the
    power of each distinct gap computed once"""
    pw = {}
    acc, at = ZERO, None
    for j in sorted(terms, reverse=True):
        if at is not None:
            gap = at - j
            if gap not in pw:
                pw[gap] = e_pow(x, gap)
            acc = e_mul(acc, pw[gap])
        acc = e_add(acc, terms[j])
        at = j
    return e_mul(acc, e_pow(x, at)) if at else acc


def frame_sparse(co, h, z, zg):
    """co: 7 dicts {j: int}; h: dict {j: E}"""
    frame = []
    for c in range(7):
        t = {j: (v, 0) for j, v in co[c].items()}
        frame += [sparse_eval(t, z), sparse_eval(t, zg)]
    frame.append(sparse_eval(h, z))
    return frame


def deep_sparse(n, co, h, z, zg, a, gam, ext, frame=None):
    """-> (frame, planes of d [ext][n]). The recurrences q_k = z q_{k+1} + P_{k+1} over all n, one
    (schoolbook) product each; ext = 1 runs them on integers and needs every input in the base field"""
    if frame is None:
        frame = frame_sparse(co, h, z, zg)
    c1, c2 = deep_constants(frame, a, gam)
    p1, p2 = {}, {}
    for c in range(7):
        for j, v in co[c].items():
            p2[j] = e_add(p2.get(j, ZERO), e_scale(a[c], v))
    p1 = dict(p2)
    for j, v in h.items():
        p1[j] = e_add(p1.get(j, ZERO), e_mul(gam, v))
    p1[0] = e_sub(p1.get(0, ZERO), c1)
    p2[0] = e_sub(p2.get(0, ZERO), c2)
    # coordinate lists of P1 and P2, zero where nothing was given
    l1 = [[0] * n for _ in range(ext)]
    l2 = [[0] * n for _ in range(ext)]
    for src, dst in ((p1, l1), (p2, l2)):
        for j, v in src.items():
            assert ext == 2 or v[1] == 0
            for k in range(ext):
                dst[k][j] = v[k]
    if ext == 1:
        assert z[1] == 0 and zg[1] == 0
        z0, w0 = z[0], zg[0]
        d = [0] * n
        q1 = q2 = 0
        a1, a2 = l1[0], l2[0]
        for k in range(n - 2, -1, -1):
            q1 = (a1[k + 1] + z0 * q1) % P
            q2 = (a2[k + 1] + w0 * q2) % P
            d[k] = (q1 + q2) % P
        assert (a1[0] + z0 * q1) % P == 0, "remainder of the division by (x - z)"
        assert (a2[0] + w0 * q2) % P == 0, "remainder of the division by (x - zg)"
        return frame, [d]
    (z0, z1), (w0, w1) = z, zg
    da, db = [0] * n, [0] * n
    q1a = q1b = q2a = q2b = 0
    a1, b1, a2, b2 = l1[0], l1[1], l2[0], l2[1]
    for k in range(n - 2, -1, -1):
        # (q0 + q1 phi)(z0 + z1 phi) = (q0 z0 - 2 q1 z1) + (q0 z1 + q1 z0 + q1 z1) phi
        t = (a1[k + 1] + q1a * z0 - 2 * q1b * z1) % P
        q1b = (b1[k + 1] + q1a * z1 + q1b * z0 + q1b * z1) % P
        q1a = t
        t = (a2[k + 1] + q2a * w0 - 2 * q2b * w1) % P
        q2b = (b2[k + 1] + q2a * w1 + q2b * w0 + q2b * w1) % P
        q2a = t
        da[k] = (q1a + q2a) % P
        db[k] = (q1b + q2b) % P
    assert e_add((a1[0], b1[0]), e_mul(z, (q1a, q1b))) == ZERO, "remainder of the division by (x - z)"
    assert e_add((a2[0], b2[0]), e_mul(zg, (q2a, q2b))) == ZERO, "remainder of the division by (x - zg)"
    return frame, [da, db]


def sparse_to_dense(n, co, h):
    return ([[co[c].get(j, 0) for j in range(n)] for c in range(7)], [h.get(j, ZERO) for j in range(n)])


def sparse_polys(n, ext, rng):
    """7 trace polynomials and H, each non-zero on its own sparse_indices"""
    co = [{j: rng.randrange(1, P) for j in sparse_indices(n, rng)} for _ in range(7)]
    h = {j: (rng.randrange(1, P), rng.randrange(1, P) if ext == 2 else 0) for j in sparse_indices(n, rng)}
    return co, h


# ---- the DEEP transcript step (deep_coin_block; host_common.hpp Coin::reseed and draw_e)
def coin_step_model(seed, frame, z, zg, ginv, ext):
    """the coin (32-byte seed; reseeding resets the counter) is reseeded with BLAKE3 of the 14 trace
    values of the frame and then of H(z), each as the LE bytes of its ext words per element; a reseed is
    seed <- BLAKE3(seed || digest). Then a_0..a_6 and gamma are drawn, and the DEEP parameters follow by
    the reference arithmetic: 1 / z (0 for z = 0), 1 / (z g) = (1 / z) ginv, c1, c2"""
    import oracle_lib as O
    from test_gpu_transcript import model_draws  # the coin's draw rule, shared with the draw tests

    def le(vals):
        return b"".join(v[k].to_bytes(8, "little") for v in vals for k in range(ext))
    seed = O.blake3(bytes(seed) + O.blake3(le(frame[:14])))
    seed = O.blake3(seed + O.blake3(le(frame[14:])))
    draws, counter, ok = model_draws(seed, 0, 8, ext, set())
    a, gam = draws[:7], draws[7]
    zinv = e_inv(z) if z != ZERO else ZERO
    c1, c2 = deep_constants(frame, a, gam)
    return {"a": a, "gamma": gam, "z": z, "zg": zg, "zinv": zinv, "zginv": e_scale(zinv, ginv), "c1": c1, "c2": c2,
            "seed": seed, "counter": counter, "fail": int(not ok or z == ZERO)}


def dp_words(m):
    """a model's DEEP parameters in the layout the debug entry returns: 14 elements of 2 words"""
    return [list(v) for v in m["a"]] + [list(m[k]) for k in ("gamma", "z", "zg", "zinv", "zginv", "c1", "c2")]


def domain_generator(n):
    return root(n.bit_length() - 1)
