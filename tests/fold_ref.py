"""Plain references for FRI folding factors other than 8: Python integers modulo p, in the spirit of
plain_ref.py (whose fold_row / fold_layer are fixed to 8 and stay the reference of the fold-8 tests).

TEST INFRASTRUCTURE ONLY. The fold is a Lagrange interpolation through the F points of a row -- no
DFT, no shared code with the library; the points and denominators of a row are kept between calls.
The FRI layer commitment takes its leaves from merkle_ref's vectorised BLAKE3 up to 128 bytes and from
the oracle's BLAKE3 beyond (the leaves of factor 16 over the quadratic extension are 256 bytes, past
merkle_ref.hash_words' two blocks), with merkle_ref's merge for the levels above.
"""
import functools

import numpy as np

import merkle_ref as M
import plain_ref as R

P = R.P
GEN = R.GEN
FACTORS = (2, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def _row_points(i, D, F):
    """the F points of row i, x_k = 7 w_D^(i + k D/F), and 1 / prod_{j != k} (x_k - x_j) for each"""
    w = R.root(D.bit_length() - 1)
    xs = [GEN * pow(w, i + k * (D // F), P) % P for k in range(F)]
    inv = []
    for k in range(F):
        den = 1
        for j in range(F):
            if j != k:
                den = den * (xs[k] - xs[j]) % P
        inv.append(pow(den, -1, P))
    return xs, inv


def fold_row(v, i, D, alpha, F):
    """the value the fold by F gives row i of a D-point layer: v[k] (E) is the layer's value at
    x_k = 7 w_D^(i + k D/F), k < F; the polynomial of degree < F through (x_k, v[k]) is evaluated at
    alpha (E) by Lagrange's formula, sum_k v[k] prod_{j != k} (alpha - x_j) / (x_k - x_j) (the numerators
    as products of a prefix and a suffix of the factors alpha - x_j)"""
    xs, inv = _row_points(i, D, F)
    fac = [R.e_sub(alpha, (x, 0)) for x in xs]
    pre, suf = [(1, 0)] * (F + 1), [(1, 0)] * (F + 1)
    for k in range(F):
        pre[k + 1] = R.e_mul(pre[k], fac[k])
        suf[F - 1 - k] = R.e_mul(suf[F - k], fac[F - 1 - k])
    acc = (0, 0)
    for k in range(F):
        num = R.e_mul(pre[k], suf[k + 1])
        acc = R.e_add(acc, R.e_mul(R.e_scale(num, inv[k]), v[k]))
    return acc


def fold_layer(vals, D, alpha, F, rows=None):
    """vals: D E-values in natural order (index K <-> 7 w_D^K); -> [folded value of row i] for i in
    `rows` (all D/F by default)"""
    Rw = D // F
    return [fold_row([vals[i + k * Rw] for k in range(F)], i, D, alpha, F) for i in (range(Rw) if rows is None else rows)]


def fri_leaf_bytes(vals, logn, logbeta, coset_major, F):
    """the leaf messages of B FRI layer commitments, vals [B, ext, D] u64 (D = 2^(logn + logbeta)):
    [B][rows] byte strings of 8 F ext bytes, row i = the E values at natural indices i + k rows, k < F
    (k-major, then coordinate); coset-major storage keeps natural index K at (K mod beta) n + K // beta"""
    vals = np.asarray(vals, dtype=np.uint64)
    B, ext, D = vals.shape
    rows = D // F
    K = np.arange(rows)[:, None] + rows * np.arange(F)[None, :]
    at = (K & ((1 << logbeta) - 1)) * (1 << logn) + (K >> logbeta) if coset_major else K
    v = np.stack([vals[:, c][:, at] for c in range(ext)], axis=3)  # [B, rows, F, ext]
    flat = np.ascontiguousarray(v.reshape(B, rows, F * ext)).astype("<u8")
    return [[flat[b, i].tobytes() for i in range(rows)] for b in range(B)]


def fri_trees(vals, logn, logbeta, coset_major, F, blake3=None):
    """heaps [B, 2 rows, 8] u32 of B FRI layer commitments for folding factor F (slot 1 = root, leaf i at
    rows + i, slot 0 zero). Leaves of up to 128 bytes go through merkle_ref's vectorised hash (pinned by
    tests/test_merkle_ref.py); the 256-byte leaves (F = 16 over the extension) are hashed one by one by
    `blake3` (default: the oracle's). Passing `blake3` hashes every leaf with it, whatever its length"""
    msgs = fri_leaf_bytes(vals, logn, logbeta, coset_major, F)
    B, rows, nbytes = len(msgs), len(msgs[0]), len(msgs[0][0])
    if blake3 is None and nbytes <= 128:
        words = np.frombuffer(b"".join(m for row in msgs for m in row), dtype="<u4").reshape(B * rows, nbytes // 4)
        return M.trees(M.hash_words(words, nbytes).reshape(B, rows, 8))
    if blake3 is None:
        import oracle_lib as O
        blake3 = O.blake3
    leaves = np.array([[np.frombuffer(blake3(m), dtype="<u4") for m in row] for row in msgs], dtype=np.uint32)
    return M.trees(leaves)
