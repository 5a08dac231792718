"""GPU: every Merkle node the commitment kernels store, against a numpy BLAKE3 tree built from the
leaves up (tests/merkle_ref.py).

A proof carries the root and a few dozen authentication paths, and the root comes from registers and
LDS, not from the stored heap: a parent written to the wrong slot or a level's store that is lost
shows in a whole-proof test only if a query lands on it. xfg_debug_merkle_lde / xfg_debug_merkle_fri run
the commitment as the prover does and return the whole heap (pre-set to 0xFF bytes), and the local
heaps of the opening kernel. The shapes are the smallest that reach each leaf kernel and each of the
tree kernels above it (csrc/merkle.hip: the routing thresholds)."""
import numpy as np
import pytest

import merkle_ref as M

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def field_values(shape, seed):
    """canonical elements, different for every proof (leading axis), with 0 and p - 1 among them"""
    v = np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)
    flat = v.reshape(shape[0], -1)
    flat[:, 0] = 0
    flat[:, 1] = P - 1
    flat[:, -1] = P - 1
    flat[:, -2] = 0
    return v


# (count, nc, n, blowup) and the route each reaches
LDE_SHAPES = [
    (2, 7, 8, 2), (3, 2, 64, 16),  # row kernel, block shorter than a wave / than 256 threads
    (2, 1, 512, 4),  # row kernel, whole blocks, n < 1024
    (1, 7, 1024, 8), (1, 1, 1024, 2), (1, 2, 1024, 16),  # two lanes per row; top from 256 nodes
    (1, 1, 2048, 2),  # tree top at its widest level (512 nodes, 1024 threads)
    (1, 1, 4096, 2),  # four-lane middle levels
    (128, 1, 4096, 2),  # row kernel at n >= 1024, one-lane middle levels
]


@pytest.mark.parametrize("count,nc,n,blowup", LDE_SHAPES)
def test_lde_commitment_every_node(prover, count, nc, n, blowup):
    lde = field_values((count, nc, blowup, n), seed=n * 100 + blowup * 7 + nc)
    if count * n <= 1024:
        opened = [(b, m) for b in range(count) for m in range(n)]
    else:
        rows = sorted({0, 1, 2, 63, 64, 255, 256, n // 2 - 1, n // 2, n - 2, n - 1})
        opened = [(b, m) for b in sorted({0, count // 2, count - 1}) for m in rows]
    logn = n.bit_length() - 1
    nodes, local = prover.debug_merkle_lde(lde, [(b << logn) | m for b, m in opened])
    heaps = M.lde_trees(lde)
    for b in range(count):
        got, want = nodes[b, 1:n], heaps[b][1:n]
        bad = np.flatnonzero((got != want).any(axis=1)) + 1
        assert bad.size == 0, f"proof {b}: {bad.size} of {n - 1} stored nodes differ, first at heap slot {bad[0]}"
    for e, (b, m) in enumerate(opened):
        want = M.lde_local_heap(heaps[b], n, blowup, m)
        bad = np.flatnonzero((local[e, 1:] != want[1:]).any(axis=1)) + 1
        assert bad.size == 0, f"proof {b} row {m}: local heap slots {bad.tolist()} differ"


# (count, ext, logn, logbeta, coset_major): rows = 2^(logn + logbeta) / 8
FRI_SHAPES = [(3, ext, logn, logbeta, cm)
              for ext in (1, 2)
              for logn, logbeta, cm in ((3, 1, True), (5, 3, True), (4, 0, False), (9, 0, False), (11, 0, False))]
FRI_SHAPES += [(1, 2, 15, 0, False), (128, 1, 15, 0, False)]  # rows = 4096: four-lane / one-lane middle levels


@pytest.mark.parametrize("count,ext,logn,logbeta,coset_major", FRI_SHAPES)
def test_fri_commitment_every_node(prover, count, ext, logn, logbeta, coset_major):
    D = 1 << (logn + logbeta)
    vals = field_values((count, ext, D), seed=D * 10 + ext * 2 + int(coset_major))
    nodes = prover.debug_merkle_fri(vals, logn, logbeta, coset_major)
    rows = D // 8
    assert nodes.shape == (count, 2 * rows, 8)
    want = M.fri_trees(vals, logn, logbeta, coset_major)
    for b in range(count):
        bad = np.flatnonzero((nodes[b, 1:] != want[b, 1:]).any(axis=1)) + 1
        assert bad.size == 0, f"proof {b}: {bad.size} of {2 * rows - 1} nodes differ, first at heap slot {bad[0]}"


def test_merkle_entries_refuse_unsupported_arguments(prover):
    import xfgstark
    ok = np.zeros((1, 1, 2, 8), dtype=np.uint64)
    for shape in [(1, 3, 2, 8), (1, 1, 32, 8), (1, 1, 1, 8), (1, 1, 3, 8), (1, 1, 2, 4), (1, 1, 2, 24)]:
        with pytest.raises(xfgstark.XfgStarkError) as ei:
            prover.debug_merkle_lde(np.zeros(shape, dtype=np.uint64))
        assert ei.value.status == 9
    with pytest.raises(xfgstark.XfgStarkError) as ei:
        prover.debug_merkle_lde(ok, [8])  # row 8 of an 8-row proof
    assert ei.value.status == 9
    with pytest.raises(xfgstark.XfgStarkError) as ei:
        prover.debug_merkle_fri(np.zeros((1, 3, 16), dtype=np.uint64), 4, 0, False)
    assert ei.value.status == 9
    with pytest.raises(xfgstark.XfgStarkError) as ei:
        prover.debug_merkle_fri(np.zeros((1, 1, 8), dtype=np.uint64), 3, 0, False)
    assert ei.value.status == 9
