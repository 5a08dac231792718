"""GPU: what a proof's constant trace columns fix is computed once per proof, not per point.

  * The trace leaf kernels run the round-1 G functions of a leaf's hash whose inputs are constant columns once
    per row subtree and resume every leaf from them (csrc/blake3.hpp b3_row7_prefix). One call of
    xfg_debug_merkle_lde_const carries 128 proofs, one per constant-column mask, and must equal the dense run on
    the filled LDE, nodes and opened subtrees alike (the opening kernel keeps the whole hash: its digests are the
    leaf kernels'). Shapes: both leaf kernels, a partial block, the 16-row blocks, the rolled wide subtree (blowup
    64 keeps the whole hash). Twice more with the columns that are not constant shared with proof 0.
  * The constraint evaluation starts its sums from a per-proof uniform part (csrc/air.hpp ce_uniform_of). 128
    traces, one per mask, constant columns of random canonical values (so the hoisted terms are not zero), against
    plain_ref.constraint_evals, in both fields; the detection picks the flags."""
import random

import numpy as np
import pytest

import plain_ref as R

pytestmark = pytest.mark.gpu
P = R.P
NMASK = 128
EDGE = [0, P - 1, 1, (1 << 32) - 1, (1 << 32), P - (1 << 32)]


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _mask_bits():
    """[128][7]: bit c of mask b"""
    return np.array([[(b >> c) & 1 for c in range(7)] for b in range(NMASK)], dtype=np.uint8)


# (n, blowup): leaves_row_kernel with a partial block; whole 64-row blocks at the bench's blowup;
# leaves_row2_kernel (128 proofs x 4 blocks of rows: under its block limit); the rolled wide subtree with the
# prefix (blowup 32, 128) and the one blowup that keeps the whole hash (64: that case proves the routing alone)
MERKLE_SHAPES = [(8, 2), (64, 8), (1024, 8), (16, 32), (8, 64), (8, 128)]


def _merkle_case(prover, n, blowup, shared, masks=None):
    """shared: None, "col4" (column 4 where it is not constant) or "all" (every column that is not constant) is
    flagged COL_SHARED against proof 0, whose mask is empty: all of its columns are live.
    masks: the masks of the call's proofs, one each (default: all 128, proof b has mask b)"""
    const = _mask_bits() if masks is None else _mask_bits()[list(masks)]
    NMASK = len(const)
    rng = np.random.default_rng(n * 1000 + blowup + (0 if shared is None else len(shared)))
    logn = n.bit_length() - 1
    entries = [(b << logn) | m for b in range(NMASK) for m in (0, n // 2 + 1, n - 1)]
    lde = rng.integers(0, P, size=(NMASK, 7, blowup, n), dtype=np.uint64)
    vals = rng.integers(0, P, size=(NMASK, 7), dtype=np.uint64)
    for b in range(1, NMASK, 5):
        vals[b, b % 7] = EDGE[b % len(EDGE)]
    flags = const.copy()
    if shared is not None:
        cols = [4] if shared == "col4" else list(range(7))
        for b in range(1, NMASK):
            for c in cols:
                if not const[b, c]:
                    flags[b, c] = 2
                    lde[b, c] = lde[0, c]
    for b, c in zip(*np.nonzero(const)):
        lde[b, c] = vals[b, c]
    if blowup <= 16:
        want_nodes, want_local = prover.debug_merkle_lde(lde, entries)
    else:  # past blowup 16 the dense kernels (CC = false, no prefix) are reached through the same entry, no flags
        want_nodes, want_local = prover.debug_merkle_lde_const(lde, None, None, entries)
    want_nodes, want_local = want_nodes.copy(), want_local.copy()
    given = np.where(const != 0, vals, vals ^ np.uint64(1))  # the value of a column that is not constant: wrong
    got_nodes, got_local = prover.debug_merkle_lde_const(lde, flags, given, entries)
    assert (want_nodes[:, 1:n] != 0xFFFFFFFF).any()
    for b in range(NMASK):
        assert np.array_equal(got_nodes[b], want_nodes[b]), f"nodes, proof {b}, mask {const[b].tolist()}"
    assert np.array_equal(got_local, want_local)


@pytest.mark.parametrize("n,blowup", MERKLE_SHAPES)
def test_leaf_kernels_resume_from_the_prefix_for_every_mask(prover, n, blowup):
    _merkle_case(prover, n, blowup, None)


# leaves_row2_kernel through the rolled wide subtree with the prefix: a sample of masks (the LDE of 128 proofs
# at n = 1024 is 235 MB at blowup 32) -- empty, full, column 4 alone live (the burn proof's), one column G
# uniform, the four column G's alone, all but one column G
@pytest.mark.parametrize("blowup,masks", [(32, (0x00, 0x7F, 0x6F, 0x01, 0x0F, 0x77, 0x3F, 0x5F)), (128, (0x00, 0x7F, 0x6F))])
def test_two_lane_leaf_kernel_of_the_wide_blowups_resumes_from_the_prefix(prover, blowup, masks):
    _merkle_case(prover, 1024, blowup, None, masks)


@pytest.mark.parametrize("shared", ["col4", "all"])
def test_leaf_kernels_with_shared_columns_for_every_mask(prover, shared):
    _merkle_case(prover, 64, 8, shared)


# ---------------------------------------------------------------- constraint evaluation
def _ce_case(prover, ext, n, blowup, same_col4):
    rng = random.Random(n * 100 + blowup * 4 + ext + (1000 if same_col4 else 0))
    const = _mask_bits()
    traces = [[[rng.randrange(P)] * n if const[b, c] else [rng.randrange(P) for _ in range(n)] for c in range(7)]
              for b in range(NMASK)]
    if same_col4:  # column 4, where it is not constant, is proof 0's: the detection finds it shared
        for b in range(1, NMASK):
            if not const[b, 4]:
                traces[b][4] = list(traces[0][4])
    airs = [R.small_air(rng.randrange(1 << 30)) for _ in range(NMASK)]
    coeffs = [[(rng.randrange(P), rng.randrange(P) if ext == 2 else 0) for _ in range(15)] for _ in range(NMASK)]
    co = np.array([[list(c[:ext]) for c in cs] for cs in coeffs], dtype=np.uint64)
    tr = np.array(traces, dtype=np.uint64)
    flags = np.asarray(prover.debug_col_classes(tr))  # the unit's detection as the prover runs it
    want_flags = const.copy()
    if same_col4:
        want_flags[1:, 4] = np.where(const[1:, 4] != 0, 1, 2)
    assert np.array_equal(flags, want_flags)
    prover.debug_poison_lde(True)
    try:
        ce = prover.debug_constraint_eval(tr, airs, co, blowup)
    finally:
        prover.debug_poison_lde(False)
    for b in range(NMASK):
        want = R.constraint_evals(traces[b], airs[b], coeffs[b])
        got = [(int(ce[b, 0, i]), int(ce[b, 1, i]) if ext == 2 else 0) for i in range(2 * n)]
        bad = [i for i in range(2 * n) if got[i] != want[i]]
        assert not bad, (f"mask {b:#x}", bad[:8])


@pytest.mark.parametrize("n,blowup", [(8, 2), (64, 8)])
@pytest.mark.parametrize("ext", [1, 2])
def test_constraint_eval_from_the_uniform_part_for_every_mask(prover, ext, n, blowup):
    _ce_case(prover, ext, n, blowup, False)


def test_constraint_eval_with_column_4_shared_by_all_proofs(prover):
    _ce_case(prover, 1, 8, 2, True)
