"""GPU: trace columns that a unit's proofs share with its first proof.

A column of proof b > 0 that equals the same column of proof 0 element for element is not transformed: its
coefficient and LDE planes are never written and every reader goes to proof 0's (csrc/columns.hpp ColConst,
COL_SHARED). Constant columns keep their own class, and OOD and DEEP take both through the descriptor.

Three layers:
  * the unit's detection against numpy (xfg_debug_col_classes),
  * whole proofs of units of three caller-supplied traces, and of three generated burn proofs, byte for
    byte against the CPU oracle, with the trace's LDE and coefficient buffers set to 0xFF bytes before
    every unit (xfg_debug_poison_lde): a reader that still goes to an unwritten plane fails,
  * the OOD and DEEP kernels with a descriptor against the dense ones on the planes written out in full
    (xfg_debug_ood_deep_const against xfg_debug_ood_deep_e)."""
import random

import numpy as np
import pytest

import fold_cases as FC
import oracle_lib as O
import plain_ref as R
import synthetic
from test_const_columns import _air_of, _trace

pytestmark = pytest.mark.gpu
P = R.P
DETECT_SPAN = 1024  # rows per detection block (CONST_DETECT_SPAN, csrc/columns.hpp)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    pr.debug_poison_lde(True)
    yield pr
    pr._options = xfgstark.ProofOptions.reference()
    pr.debug_poison_lde(False)
    pr.close()


# ---------------------------------------------------------------- classification against numpy
def _classes_np(tr):
    """0 live, 1 constant, 2 equal to trace 0's column (never trace 0 itself); constant wins"""
    const = (tr == tr[:, :, :1]).all(axis=2)
    same = (tr == tr[:1]).all(axis=2)
    same[0] = False
    return np.where(const, 1, np.where(same, 2, 0)).astype(np.uint8)


def _rand(rng, n):
    return rng.integers(0, P, size=n, dtype=np.uint64)


def _mixed_unit(n, seed):
    """three traces; column by column: shared by all, shared by proof 1 alone, by none, proofs 1 and 2 equal
    to each other but not to proof 0, one constant in all three, proof 0's constant and proof 1's not,
    proof 0's live with proof 1's constant and proof 2's shared"""
    rng = np.random.default_rng(seed)
    tr = np.empty((3, 7, n), dtype=np.uint64)
    tr[:, 0] = _rand(rng, n)
    tr[0, 1] = tr[1, 1] = _rand(rng, n)
    tr[2, 1] = _rand(rng, n)
    for b in range(3):
        tr[b, 2] = _rand(rng, n)
    tr[0, 3] = _rand(rng, n)
    tr[1, 3] = tr[2, 3] = _rand(rng, n)
    tr[:, 4] = int(rng.integers(0, P, dtype=np.uint64))
    tr[0, 5] = tr[2, 5] = int(rng.integers(0, P, dtype=np.uint64))
    tr[1, 5] = _rand(rng, n)
    tr[0, 6] = tr[2, 6] = _rand(rng, n)
    tr[1, 6] = int(rng.integers(0, P, dtype=np.uint64))
    want = [[0, 0, 0, 0, 1, 1, 0], [2, 2, 0, 0, 1, 0, 1], [2, 0, 0, 0, 1, 1, 2]]
    return tr, want


@pytest.mark.parametrize("n", [8, 64])
def test_classes_of_a_mixed_unit(prover, n):
    tr, want = _mixed_unit(n, 3100 + n)
    assert _classes_np(tr).tolist() == want
    got, vals = prover.debug_col_classes(tr, values=True)
    assert got.dtype == np.uint8 and got.tolist() == want
    const = np.array(want) == 1
    assert np.array_equal(vals[const], tr[:, :, 0][const])


def test_one_differing_cell_keeps_a_column_live(prover):
    """n = 2048, two detection blocks per column: proof 1's columns 0, 1, 2 differ from proof 0's in one cell
    each -- row 0, row n - 1, a row of the second block -- and proof 2's in none"""
    n = 2 * DETECT_SPAN
    rng = np.random.default_rng(3200)
    tr = np.empty((3, 7, n), dtype=np.uint64)
    for c in range(7):
        tr[:, c] = _rand(rng, n)
    for c, row in enumerate([0, n - 1, DETECT_SPAN + 476]):
        tr[1, c, row] = (int(tr[1, c, row]) + 1 + int(rng.integers(0, P - 1, dtype=np.uint64))) % P
    want = [[0] * 7, [0, 0, 0, 2, 2, 2, 2], [2] * 7]
    assert _classes_np(tr).tolist() == want
    assert prover.debug_col_classes(tr).tolist() == want


@pytest.mark.parametrize("n", [8, 64, 2 * DETECT_SPAN])
def test_a_lone_trace_shares_nothing(prover, n):
    tr, _ = _mixed_unit(n, 3300 + n)
    for b in range(3):
        got = prover.debug_col_classes(tr[b:b + 1])
        assert got.tolist() == _classes_np(tr[b:b + 1]).tolist() and 2 not in got


# ---------------------------------------------------------------- whole proofs against the oracle
PATTERNS = ["burn", "two_shared", "one_cell", "none", "all_shared"]


def _unit(pattern, n, seed):
    """three traces [3][7][n] (lists of Python integers, as tests/test_const_columns.py _trace)"""
    rng = random.Random(seed)
    live = [_trace("none", n, seed + 10 + b) for b in range(3)]
    if pattern == "burn":  # six per-proof constants, the one live column identical in all three
        tr = [_trace("all", n, seed + 20 + b) for b in range(3)]
        for b in range(3):
            tr[b][4] = list(live[0][4])
        return tr
    if pattern == "two_shared":  # columns 2 and 4 shared, the rest live
        for b in (1, 2):
            live[b][2], live[b][4] = list(live[0][2]), list(live[0][4])
        return live
    if pattern == "one_cell":  # shared in proof 1, one cell off in proof 2
        for c, row in ((1, 0), (4, n - 1), (6, n // 2)):
            live[1][c], live[2][c] = list(live[0][c]), list(live[0][c])
            live[2][c][row] = (live[2][c][row] + 1 + rng.randrange(P - 1)) % P
        return live
    if pattern == "none":
        return live
    assert pattern == "all_shared"  # every column live and shared: proofs 1 and 2 own no plane at all
    return [[list(col) for col in live[0]] for _ in range(3)]


_EXPECT = {
    "burn": [[1, 1, 1, 1, 0, 1, 1], [1, 1, 1, 1, 2, 1, 1], [1, 1, 1, 1, 2, 1, 1]],
    "two_shared": [[0] * 7, [0, 0, 2, 0, 2, 0, 0], [0, 0, 2, 0, 2, 0, 0]],
    "one_cell": [[0] * 7, [0, 2, 0, 0, 2, 0, 2], [0] * 7],
    "none": [[0] * 7] * 3,
    "all_shared": [[0] * 7, [2] * 7, [2] * 7],
}


def _set_options(prover, blowup, ext):
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension = blowup, ext
    prover._options = o


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,blowup", [(8, 8), (64, 2), (1024, 16), (64, 32)])
@pytest.mark.parametrize("ext", [1, 2])
def test_unit_of_three_traces_matches_oracle(prover, ext, n, blowup, pattern):
    seed = 4000 + 1000 * ext + 3 * n + blowup + 7 * PATTERNS.index(pattern)
    tr = _unit(pattern, n, seed)
    airs = [R.small_air(seed + 50 + b) for b in range(3)]  # every proof its own AIR constants
    arr = np.array(tr, dtype=np.uint64)
    assert prover.debug_col_classes(arr).tolist() == _EXPECT[pattern]
    opts = O.options(blowup=blowup, field_extension=ext)
    want = []
    for b in range(3):
        flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr[b] for v in col])
        st, pr = O.prove(_air_of(airs[b]), n, opts, trace=flat)
        assert st == 0
        want.append(pr)
    _set_options(prover, blowup, ext)
    got = prover.prove_traces(arr, airs)
    for b in range(3):
        assert got[b].to_bytes() == want[b], b


def test_first_trace_differs_and_the_others_agree(prover):
    """the representative is proof 0 alone: proofs 1 and 2 agree with each other in every column and share
    nothing, and the unit is still right"""
    n, blowup, ext, seed = 64, 8, 1, 4900
    tr = _unit("all_shared", n, seed)
    tr[0] = _trace("none", n, seed + 1)
    airs = [R.small_air(seed + 50 + b) for b in range(3)]
    arr = np.array(tr, dtype=np.uint64)
    assert prover.debug_col_classes(arr).tolist() == [[0] * 7] * 3
    _set_options(prover, blowup, ext)
    got = prover.prove_traces(arr, airs)
    for b in range(3):
        flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr[b] for v in col])
        st, want = O.prove(_air_of(airs[b]), n, O.options(blowup=blowup, field_extension=ext), trace=flat)
        assert st == 0 and got[b].to_bytes() == want, b


def test_generated_batch_of_three_matches_oracle(prover):
    """prove_batch: the traces are generated on the device and go through the same detection"""
    import xfgstark
    n = 64
    prover._options = xfgstark.ProofOptions.reference()
    inputs = [synthetic.burn_inputs(5100 + i) for i in range(3)]
    want = []
    for kw in inputs:
        st, pr = O.prove(FC.oracle_air(kw), n, O.options())
        assert st == 0
        want.append(pr)
    assert [p.to_bytes() for p in prover.prove_batch(inputs, trace_length=n)] == want


# ---------------------------------------------------------------- OOD and DEEP with a descriptor against dense
# a block takes up to 256 threads x 8 coefficients: 64 is a block of 8 threads, 2048 the largest single
# block, 4096 two blocks (the constant column's partial is v in block 0 and 0 in block 1)
@pytest.mark.parametrize("n", [64, 2048, 4096])
@pytest.mark.parametrize("ext", [1, 2])
def test_ood_deep_with_descriptor_equal_dense(prover, ext, n):
    """two instances; column 5 constant in both (its coefficients (v, 0, ..., 0) written out for the dense
    run), column 2 of instance 1 shared (instance 0's coefficients written out in its place)"""
    rng = np.random.default_rng(6000 + 10 * n + ext)
    coef = rng.integers(0, P, size=(2, 7, n), dtype=np.uint64)
    coef[:, 5, 1:] = 0
    coef[1, 2] = coef[0, 2]
    flags = np.array([[0, 0, 0, 0, 0, 1, 0], [0, 0, 2, 0, 0, 1, 0]], dtype=np.uint8)
    vals = rng.integers(0, P, size=(2, 7), dtype=np.uint64)  # wrong wherever no constant is flagged
    vals[:, 5] = coef[:, 5, 0]
    hcoef = rng.integers(0, P, size=(2, ext, n), dtype=np.uint64)
    zpts = rng.integers(1, P, size=(2, 2, ext), dtype=np.uint64)
    coeffs = rng.integers(0, P, size=(2, 8, ext), dtype=np.uint64)
    want_ood, want_deep = prover.debug_ood_deep_e(coef, hcoef, zpts, coeffs=coeffs)
    want_ood, want_deep = want_ood.copy(), want_deep.copy()
    assert (want_ood[:, 10:12, 0] == coef[:, 5, :1]).all()  # T_5(z) = T_5(zg) = v
    got_ood, got_deep = prover.debug_ood_deep_const(coef, flags, vals, hcoef, zpts, coeffs)
    assert np.array_equal(got_ood, want_ood)
    assert np.array_equal(got_deep, want_deep)
    assert (got_deep < np.uint64(P)).all()
