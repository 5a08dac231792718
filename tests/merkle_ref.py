"""Vectorised numpy BLAKE3 for the Merkle commitments: single-chunk messages of at most 128 bytes
(one or two blocks), which is all winter-crypto's Blake3_256 needs for hash_elements of up to 16
field elements and for merge. Digests are arrays [..., 8] of little-endian u32 words, the form the
device keeps them in. Pinned against xfgstark.blake3 by tests/test_merkle_ref.py.

On top of it, the whole trees the prover commits to, built from the leaves up (heap layout of
MerkleTree::new: slot 1 = root, slot i = merge(slot 2i, slot 2i+1), leaf k at slot L + k)."""
import numpy as np

IV = np.array([0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19],
              dtype=np.uint32)
PERM = [2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8]
CHUNK_START, CHUNK_END, ROOT = 1, 2, 8


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(s, a, b, c, d, x, y):
    s[a] = s[a] + s[b] + x
    s[d] = _rotr(s[d] ^ s[a], 16)
    s[c] = s[c] + s[d]
    s[b] = _rotr(s[b] ^ s[c], 12)
    s[a] = s[a] + s[b] + y
    s[d] = _rotr(s[d] ^ s[a], 8)
    s[c] = s[c] + s[d]
    s[b] = _rotr(s[b] ^ s[c], 7)


def compress(cv, m, block_len, flags):
    """cv: 8 arrays [N] u32 (or the IV words), m: 16 arrays [N] u32; counter 0. Returns 8 arrays [N]"""
    n = m[0].shape[0]
    full = lambda v: np.full(n, v, dtype=np.uint32)
    s = [np.array(w, dtype=np.uint32) if np.ndim(w) else full(w) for w in cv]
    s += [full(IV[0]), full(IV[1]), full(IV[2]), full(IV[3]), full(0), full(0), full(block_len), full(flags)]
    m = list(m)
    for r in range(7):
        _g(s, 0, 4, 8, 12, m[0], m[1])
        _g(s, 1, 5, 9, 13, m[2], m[3])
        _g(s, 2, 6, 10, 14, m[4], m[5])
        _g(s, 3, 7, 11, 15, m[6], m[7])
        _g(s, 0, 5, 10, 15, m[8], m[9])
        _g(s, 1, 6, 11, 12, m[10], m[11])
        _g(s, 2, 7, 8, 13, m[12], m[13])
        _g(s, 3, 4, 9, 14, m[14], m[15])
        m = [m[PERM[i]] for i in range(16)]
    return [s[i] ^ s[i + 8] for i in range(8)]


def hash_words(words, nbytes):
    """BLAKE3 of N messages of nbytes <= 128 bytes each, given as [N, ceil(nbytes / 4)] LE u32 words
    (a last partial word zero padded). Returns [N, 8] u32"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    assert w.ndim == 2 and 0 < nbytes <= 128 and w.shape[1] == (nbytes + 3) // 4
    nblk = 2 if nbytes > 64 else 1
    pad = np.zeros((w.shape[0], 16 * nblk), dtype=np.uint32)
    pad[:, :w.shape[1]] = w
    cv = list(IV)
    with np.errstate(over="ignore"):
        for b in range(nblk):
            last = b == nblk - 1
            flags = (CHUNK_START if b == 0 else 0) | ((CHUNK_END | ROOT) if last else 0)
            blen = nbytes - 64 * b if last else 64
            cv = compress(cv, [pad[:, 16 * b + i] for i in range(16)], blen, flags)
    return np.stack(cv, axis=1)


def hash_bytes(msgs):
    """BLAKE3 of equally long byte strings (<= 128 bytes): list of 32-byte digests"""
    n = len(msgs[0])
    assert all(len(x) == n for x in msgs)
    padded = b"".join(x + bytes(-n % 4) for x in msgs)
    words = np.frombuffer(padded, dtype="<u4").reshape(len(msgs), -1)
    return [d.astype("<u4").tobytes() for d in hash_words(words, n)]


def hash_elements(e):
    """Blake3_256::hash_elements of N rows of K <= 16 base-field elements, e [N, K] u64: the elements'
    8 K little-endian bytes"""
    e = np.ascontiguousarray(e, dtype="<u8")
    return hash_words(e.view("<u4").reshape(e.shape[0], 2 * e.shape[1]), 8 * e.shape[1])


def merge(a, b):
    """Blake3_256::merge: BLAKE3(a || b) for digests [N, 8]"""
    return hash_words(np.concatenate([a, b], axis=1), 64)


def trees(leaves):
    """the heaps [B, 2 L, 8] over B sets of L = 2^k leaf digests, leaves [B, L, 8]; slot 0 is zero.
    (All B trees level by level in one array: the cost is numpy calls, not hashes.)"""
    B, L, _ = leaves.shape
    assert L & (L - 1) == 0
    heap = np.zeros((B, 2 * L, 8), dtype=np.uint32)
    heap[:, L:] = leaves
    w = L
    while w > 1:
        kids = heap[:, w:2 * w].reshape(B * w // 2, 16)
        heap[:, w // 2:w] = merge(kids[:, :8], kids[:, 8:]).reshape(B, w // 2, 8)
        w //= 2
    return heap


def lde_trees(lde):
    """heaps [B, 2 n beta, 8] of B LDE commitments, lde [B, nc, beta, n] coset-major: leaf m beta + t =
    hash_elements(the nc columns at coset t, row m), i.e. the row at natural LDE index t + beta m"""
    B, nc, beta, n = lde.shape
    rows = np.ascontiguousarray(np.transpose(lde, (0, 3, 2, 1))).reshape(B * n * beta, nc)
    return trees(hash_elements(rows).reshape(B, n * beta, 8))


def lde_local_heap(heap, n, beta, m):
    """the 2 beta slots of row m's subtree in one proof's heap (slot 1 = node n + m of the full heap,
    leaf t at beta + t)"""
    out = np.zeros((2 * beta, 8), dtype=np.uint32)
    w = 1
    while w <= beta:
        out[w:2 * w] = heap[(n + m) * w:(n + m + 1) * w]
        w *= 2
    return out


def fri_trees(vals, logn, logbeta, coset_major):
    """heaps [B, 2 rows, 8] of B FRI layer commitments, vals [B, ext, D] (D = 2^(logn + logbeta), rows =
    D / 8): leaf i = hash_elements(the E values at natural indices i + k rows, k < 8, coordinates
    interleaved); coset-major storage keeps natural index K at (K mod beta) n + K // beta"""
    B, ext, D = vals.shape
    rows = D // 8
    K = np.arange(rows)[:, None] + rows * np.arange(8)[None, :]
    at = (K & ((1 << logbeta) - 1)) * (1 << logn) + (K >> logbeta) if coset_major else K
    v = np.stack([vals[:, c][:, at] for c in range(ext)], axis=3)  # [B, rows, 8, ext]
    return trees(hash_elements(v.reshape(B * rows, 8 * ext)).reshape(B, rows, 8))
