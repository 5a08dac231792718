"""GPU: the consumers of a trace LDE whose constant columns have no plane (csrc/columns.hpp ColConst).

The prover no longer writes the LDE plane of a column it found constant: the leaf kernels, the opening
kernel and the constraint evaluation take such a column's value from a descriptor. Kernel level:
  * leaf and opening kernels with flags (xfg_debug_merkle_lde_const: the flagged planes are set to 0xFF
    bytes on the device, so a kernel that still reads one hashes a word that is no field element)
    against the dense path of the same kernels on an LDE whose flagged columns hold the value
    (xfg_debug_merkle_lde, itself pinned by tests/test_merkle.py against tests/merkle_ref.py; past
    blowup 16, which that entry refuses, the same dense kernels through the new entry without flags),
  * the constraint evaluation behind the prover's own trace LDE, the whole LDE buffer set to 0xFF bytes
    first (xfg_debug_poison_lde), against plain_ref.constraint_evals."""
import random

import numpy as np
import pytest

import plain_ref as R

pytestmark = pytest.mark.gpu
P = R.P


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _patterns():
    """none, all, each single column, all but each single column (the burn proof's own is all but 4)"""
    pats = [[0] * 7, [1] * 7]
    pats += [[1 if c == k else 0 for c in range(7)] for k in range(7)]
    pats += [[0 if c == k else 1 for c in range(7)] for k in range(7)]
    return np.array(pats, dtype=np.uint8)


# (n, blowup, count) and the route each reaches (csrc/merkle.hip)
MERKLE_SHAPES = [
    (8, 8, 3),      # leaves_row_kernel, partial block
    (256, 2, 3),    # leaves_row_kernel, whole blocks
    (256, 16, 2),   # leaves_row_kernel, 16-leaf unrolled subtree
    (1024, 8, 1),   # leaves_row2_kernel
    (64, 32, 2),    # rolled levels of lde_subtree_wide
    (64, 128, 1),   # open_rows_kernel with two leaves per lane
]


@pytest.mark.parametrize("n,blowup,count", MERKLE_SHAPES)
def test_leaf_and_opening_kernels_with_flags_equal_dense(prover, n, blowup, count):
    """every pattern, rotated over the proofs of a call so that each proof has flags of its own; nodes
    and the opened local heaps (first, last and two inner rows of every proof) equal the dense run's"""
    pats = _patterns()
    rng = np.random.default_rng(n * 1000 + blowup)
    logn = n.bit_length() - 1
    entries = [(b << logn) | m for b in range(count) for m in (0, n // 3, n // 2 + 1, n - 1)]
    base = rng.integers(0, P, size=(count, 7, blowup, n), dtype=np.uint64)
    edge = [0, P - 1, 1, (1 << 32) - 1]
    for i in range(len(pats)):
        flags = np.stack([pats[(i + b) % len(pats)] for b in range(count)])
        vals = rng.integers(0, P, size=(count, 7), dtype=np.uint64)
        vals[0, i % 7] = edge[i % len(edge)]
        lde = base.copy()
        for b, c in zip(*np.nonzero(flags)):
            lde[b, c] = vals[b, c]
        if blowup <= 16:
            want_nodes, want_local = prover.debug_merkle_lde(lde, entries)
        else:
            want_nodes, want_local = prover.debug_merkle_lde_const(lde, None, None, entries)
        want_nodes, want_local = want_nodes.copy(), want_local.copy()
        # the values of unflagged columns are never to be used: make them wrong
        given = np.where(flags != 0, vals, vals ^ np.uint64(1))
        got_nodes, got_local = prover.debug_merkle_lde_const(lde, flags, given, entries)
        assert (want_nodes[:, 1:n] != 0xFFFFFFFF).any()
        assert np.array_equal(got_nodes, want_nodes), flags.tolist()
        assert np.array_equal(got_local, want_local), flags.tolist()


def test_const_entry_refuses_what_it_has_no_kernel_for(prover):
    import xfgstark
    ok = np.zeros((1, 7, 2, 8), dtype=np.uint64)
    f, v = np.ones((1, 7), dtype=np.uint8), np.zeros((1, 7), dtype=np.uint64)
    prover.debug_merkle_lde_const(ok, f, v)
    for shape in [(1, 7, 256, 8), (1, 7, 3, 8), (1, 7, 2, 4)]:
        with pytest.raises(xfgstark.XfgStarkError) as ei:
            prover.debug_merkle_lde_const(np.zeros(shape, dtype=np.uint64), f, v)
        assert ei.value.status == 9
    with pytest.raises(xfgstark.XfgStarkError) as ei:  # constant columns are those of the 7-column trace
        prover.debug_merkle_lde_const(np.zeros((1, 2, 2, 8), dtype=np.uint64), np.ones((1, 2), dtype=np.uint8),
                                      np.zeros((1, 2), dtype=np.uint64))
    assert ei.value.status == 9


# ---------------------------------------------------------------- constraint evaluation
# per instance of a call, the columns that are constant: the burn proof's own pattern, all (column 4
# flagged: the next row's column 4 is the value too), column 4 alone, none, and two mixed ones
CE_PATTERNS = [[(0, 1, 2, 3, 5, 6), (0, 1, 2, 3, 4, 5, 6), (4,)], [(), (0, 4, 6), (1, 2, 3, 5)]]


def _ce_trace(n, const_cols, rng):
    return [[rng.randrange(P)] * n if c in const_cols else [rng.randrange(P) for _ in range(n)] for c in range(7)]


@pytest.mark.parametrize("n,blowup", [(8, 2), (8, 8), (64, 2), (64, 8)])
@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_eval_with_constant_columns_matches_reference(prover, ext, n, blowup):
    rng = random.Random(n * 100 + blowup * 4 + ext)
    prover.debug_poison_lde(True)
    try:
        for pats in CE_PATTERNS:
            traces = [_ce_trace(n, cols, rng) for cols in pats]
            airs = [R.small_air(rng.randrange(1 << 30)) for _ in pats]
            coeffs = [[(rng.randrange(P), rng.randrange(P) if ext == 2 else 0) for _ in range(15)] for _ in pats]
            co = np.array([[list(c[:ext]) for c in cs] for cs in coeffs], dtype=np.uint64)
            flags = prover.debug_const_columns(np.array(traces, dtype=np.uint64))
            assert [tuple(np.flatnonzero(f)) for f in flags] == [tuple(p) for p in pats]
            ce = prover.debug_constraint_eval(np.array(traces, dtype=np.uint64), airs, co, blowup)
            for b in range(len(pats)):
                want = R.constraint_evals(traces[b], airs[b], coeffs[b])
                got = [(int(ce[b, 0, i]), int(ce[b, 1, i]) if ext == 2 else 0) for i in range(2 * n)]
                bad = [i for i in range(2 * n) if got[i] != want[i]]
                assert not bad, (pats[b], bad[:8])
    finally:
        prover.debug_poison_lde(False)
