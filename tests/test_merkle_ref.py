"""The numpy BLAKE3 of tests/merkle_ref.py (the reference of the whole-heap Merkle tests) against the
library's host BLAKE3 (xfgstark.blake3, itself pinned by the published vectors in test_oracle_kats.py)."""
import random

import numpy as np
import pytest

import merkle_ref as M


@pytest.mark.parametrize("nbytes", [8, 16, 56, 64, 128])
def test_numpy_blake3_matches_library(nbytes):
    import xfgstark
    rng = random.Random(nbytes)
    msgs = [bytes(nbytes), bytes([0xFF]) * nbytes] + [rng.randbytes(nbytes) for _ in range(30)]
    assert M.hash_bytes(msgs) == [xfgstark.blake3(m) for m in msgs]


def test_hash_elements_merge_and_tree():
    import xfgstark
    rng = random.Random(7)
    e = np.array([[rng.randrange(1 << 64) for _ in range(7)] for _ in range(8)], dtype=np.uint64)
    leaves = M.hash_elements(e)
    for row, d in zip(e, leaves):
        assert d.astype("<u4").tobytes() == xfgstark.blake3(row.astype("<u8").tobytes())
    heap = M.trees(leaves[None])[0]
    by = lambda d: d.astype("<u4").tobytes()
    for i in range(1, 8):
        assert by(heap[i]) == xfgstark.blake3(by(heap[2 * i]) + by(heap[2 * i + 1]))
    assert np.array_equal(heap[8:], leaves)
