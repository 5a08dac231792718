"""CPU self-checks of tests/ood_deep_ref.py: the references the OOD / DEEP kernel tests compare against
must satisfy the identities that define the DEEP quotient (no GPU, no library code)."""
import random

import pytest

import ood_deep_ref as D
import plain_ref as R

P = R.P


@pytest.mark.parametrize("x", [(1, 0), (P - 1, 0), (7, 0), (0, 1), (0, P - 1), (0, 12345), (P - 1, P - 1),
                               (0x123456789ABCDEF0, 0), (0xFEDCBA9876543210 % P, 0x8000000080000001)])
def test_e_inv_is_the_inverse(x):
    """among them x in the base field, where the answer is pow(x, -1, p), and x = (0, b)"""
    y = D.e_inv(x)
    assert R.e_mul(x, y) == D.ONE
    if x[1] == 0:
        assert y == (pow(x[0], -1, P), 0)


def test_e_inv_on_random_elements():
    rng = random.Random(11)
    for _ in range(20):
        x = D.rand_e(rng, 2)
        assert R.e_mul(D.e_inv(x), x) == D.ONE
    with pytest.raises(AssertionError):
        D.e_inv(D.ZERO)


def _sparse_case(n, ext, seed):
    rng = random.Random(seed)
    co, h = D.sparse_polys(n, ext, rng)
    z = D.rand_e(rng, ext)
    zg = R.e_scale(z, D.domain_generator(n))
    a = [D.rand_e(rng, ext) for _ in range(7)]
    return co, h, z, zg, a, D.rand_e(rng, ext)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", [64, 4096])
def test_sparse_reference_equals_dense(n, ext):
    co, h, z, zg, a, gam = _sparse_case(n, ext, n + ext)
    frame_s, d_s = D.deep_sparse(n, co, h, z, zg, a, gam, ext)
    dco, dh = D.sparse_to_dense(n, co, h)
    frame_d, d_d = D.deep_dense(dco, dh, z, zg, a, gam)
    assert frame_s == frame_d
    assert d_s == D.planes(d_d, ext)
    assert any(d_s[0]) and d_s[0][n - 1] == 0


def test_sparse_indices_hold_the_block_and_chunk_edges():
    n = 1 << 14
    s = set(D.sparse_indices(n, random.Random(1), extra=0))
    assert {0, 1, n - 2, n - 1} <= s
    assert all(b in s and b + 2047 in s for b in range(0, n, 2048))
    blocks = [b for b in range(0, n, 2048) if all(b + 8 * m in s and b + 8 * m + 7 in s for m in range(256))]
    assert len(blocks) == 1


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", [8, 64, 256])
def test_dense_reference_is_the_deep_quotient(n, ext):
    """d(r) = (P1(r) - c1) / (r - z) + (P2(r) - c2) / (r - zg) at random r in E, with P1 and P2 the
    combinations before their constant terms are shifted; and c1 = P1(z), c2 = P2(zg)"""
    rng = random.Random(100 * n + ext)
    co = [[rng.randrange(P) for _ in range(n)] for _ in range(7)]
    h = [D.rand_e(rng, ext) for _ in range(n)]
    z, zg = D.rand_e(rng, ext), D.rand_e(rng, ext)
    a, gam = [D.rand_e(rng, ext) for _ in range(7)], D.rand_e(rng, ext)
    frame, d = D.deep_dense(co, h, z, zg, a, gam)
    c1, c2 = D.deep_constants(frame, a, gam)
    p1, p2 = D.combine_dense(co, h, a, gam)
    assert D.horner(p1, z) == c1 and D.horner(p2, zg) == c2
    assert d[n - 1] == D.ZERO and d[n - 2] != D.ZERO
    for _ in range(4):
        r = D.rand_e(rng, 2)
        t1 = R.e_mul(R.e_sub(D.horner(p1, r), c1), D.e_inv(R.e_sub(r, z)))
        t2 = R.e_mul(R.e_sub(D.horner(p2, r), c2), D.e_inv(R.e_sub(r, zg)))
        assert D.horner(d, r) == R.e_add(t1, t2)


def test_dense_reference_equals_the_base_field_one():
    """the base-field reference of tests/test_gpu_parity.py, restated on integers"""
    n = 32
    rng = random.Random(5)
    co = [[rng.randrange(P) for _ in range(n)] for _ in range(7)]
    h = [rng.randrange(P) for _ in range(n)]
    z, zg, gam = rng.randrange(1, P), rng.randrange(1, P), rng.randrange(P)
    a = [rng.randrange(P) for _ in range(7)]
    frame, d = D.deep_dense(co, [(v, 0) for v in h], (z, 0), (zg, 0), [(v, 0) for v in a], (gam, 0))

    def ev(poly, x):
        return sum(v * pow(x, j, P) for j, v in enumerate(poly)) % P
    assert D.planes(frame, 1)[0] == [ev(co[c], x) for c in range(7) for x in (z, zg)] + [ev(h, z)]
    s = [sum(a[c] * co[c][j] for c in range(7)) % P for j in range(n)]
    p1 = [(s[j] + gam * h[j]) % P for j in range(n)]
    # quotient coefficient k of (p - p(x0)) / (x - x0) is sum_{j > k} p_j x0^(j - k - 1)
    want = [(sum(p1[j] * pow(z, j - k - 1, P) for j in range(k + 1, n)) +
             sum(s[j] * pow(zg, j - k - 1, P) for j in range(k + 1, n))) % P for k in range(n)]
    assert D.planes(d, 1)[0] == want
