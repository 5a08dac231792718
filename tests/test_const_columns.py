"""Constant trace columns: detected on the device, skipped by the NTT kernels, filled in by one kernel.

Three layers, each against an independent reference:
  * the detection kernel against numpy (xfg_debug_const_columns),
  * the NTT kernels with a flag vector against the same kernels without one (xfg_debug_lde_skip /
    xfg_debug_interpolate_skip against xfg_debug_lde / xfg_debug_interpolate, bit for bit), one
    forward and one inverse shape per kernel family that tests/ntt_shapes.py reaches,
  * whole proofs of arbitrary traces through xfg_prove_trace against the CPU oracle's bytes."""
import random

import numpy as np
import pytest

import ntt_shapes
import oracle_lib as O
import plain_ref as R

pytestmark = pytest.mark.gpu
P = R.P
DETECT_SPAN = 1024  # rows per detection block (CONST_DETECT_SPAN, csrc/columns.hpp)


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


# ---------------------------------------------------------------- detection against numpy
def _off_rows(n):
    """rows at which a column that is constant but for one element differs: the ends, the middle, and the
    last row of one detection block with the first row of the next (where the column has two blocks)"""
    rows = [0, 1, n // 2, n - 1]
    if n > DETECT_SPAN:
        rows += [DETECT_SPAN - 1, DETECT_SPAN, n - DETECT_SPAN - 1, n - DETECT_SPAN]
    return sorted(set(rows))


def _column_kinds(n):
    return [("random", None)] + [("const", v) for v in (0, 1, P - 1)] + [("off", r) for r in _off_rows(n)]


def _make_column(kind, arg, n, rng):
    if kind == "random":
        return rng.integers(0, P, size=n, dtype=np.uint64)
    if kind == "const":
        return np.full(n, arg, dtype=np.uint64)
    v = int(rng.integers(0, P, dtype=np.uint64))
    col = np.full(n, v, dtype=np.uint64)
    col[arg] = (v + 1 + int(rng.integers(0, P - 1, dtype=np.uint64))) % P  # any other canonical value
    return col


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("n", [8, 64, 256, 1024, 4096])
def test_detection_matches_numpy(prover, n, count):
    """count 5: width 7, every proof a different mix (the kinds rotate through the 35 columns, which
    holds every kind at least once); count 1: one column of every kind (the hook is generic over width)"""
    kinds = _column_kinds(n)
    rng = np.random.default_rng(1000 * n + count)
    width = 7 if count > 1 else len(kinds)
    assert count * width >= len(kinds)
    trace = np.empty((count, width, n), dtype=np.uint64)
    for b in range(count):
        for c in range(width):
            kind, arg = kinds[(b * width + c) % len(kinds)]  # the kinds go round: another mix per proof
            trace[b, c] = _make_column(kind, arg, n, rng)
    want = (trace == trace[:, :, :1]).all(axis=2).astype(np.uint8)
    assert 0 < want.sum() < want.size
    got = prover.debug_const_columns(trace)
    assert got.dtype == np.uint8 and np.array_equal(got, want)


# ---------------------------------------------------------------- flagged transforms against unflagged ones
def _flag_patterns(npoly):
    """first only, last only, alternating (first and last among them when npoly is odd)"""
    first = np.zeros(npoly, dtype=np.uint8)
    first[0] = 1
    last = np.zeros(npoly, dtype=np.uint8)
    last[-1] = 1
    alt = np.zeros(npoly, dtype=np.uint8)
    alt[::2] = 1
    return [first, last, alt]


# (n, blowup, polynomials): forward kernel families, at the smallest launch set that takes the route
_FWD = [
    (8, 2, 3),          # generic pass A / B, one partial tile, XCD renumbering in both passes
    (64, 8, 3),         # generic pass A / B, several cosets, XCD renumbering in both passes
    (4096, 8, 3),       # generic pass A / B, full tiles
    (1 << 16, 8, 32),   # ntt_pass_a_cos2 + ntt_pass_b_tq: the all-coset route, 32 x 16 = 512 blocks
    (1 << 16, 2, 32),   # ntt_pass_a_cos + ntt_pass_b_tq
    (1 << 16, 8, 28),   # below 512 blocks: generic pass A per (tile, poly, coset) + generic pass B
    (1 << 17, 2, 16),   # ntt_pass_a_cos + the generic pass B applying the four-step twiddles
    (1 << 18, 2, 3),    # generic pass A + ntt_pass_b_pers
    (1 << 20, 2, 2),    # generic pass A, R = 1024, cosets of a tile consecutive (xcd_block_coset) + ntt_pass_b_pers
]
# (n, off7, polynomials): inverse kernels are the generic passes only
_INV = [(8, False, 3), (64, True, 3), (1 << 13, False, 3), (1 << 16, False, 3), (1 << 20, False, 2)]


def _routes():
    """every forward / inverse shape above is one that tests/ntt_shapes.py lists (same n and blowup or offset)"""
    fwd = {(n, b) for n, b in ntt_shapes.LDE_3POLY + ntt_shapes.LDE_1POLY}
    fwd |= {(1 << 16, b) for _, b in ntt_shapes.LDE_2P16_SETS} | {(n, b) for n, _, b in ntt_shapes.LDE_ALL_COSET_GENERIC_B}
    inv = {n for n, _ in ntt_shapes.INTERPOLATE_2POLY + ntt_shapes.INTERPOLATE_1POLY}
    return fwd, inv


def test_shapes_are_those_of_ntt_shapes():
    fwd, inv = _routes()
    assert all((n, b) in fwd for n, b, _ in _FWD)
    assert all(n in inv or n == 1 << 16 for n, _, _ in _INV)  # 2^16: the trace interpolation of the headline


def _check_lde_skip(prover, n, blowup, npoly, patterns, seed):
    """Both hooks run in the same device buffers, which keep what the last call left. So that a block
    that wrongly returns, or a fill that misses part of a plane, cannot find the answer already there,
    the flagged hook poisons its output and intermediate buffers before it launches, and here every
    unflagged run comes first: the flagged run of one pattern follows the unflagged run of another
    input (or, with one pattern, starts from the poison alone)."""
    rng = np.random.default_rng(seed)
    inputs, wants = [], []
    for flags in patterns:
        coef = rng.integers(0, P, size=(npoly, n), dtype=np.uint64)
        coef[flags != 0, 1:] = 0  # a flagged polynomial is truly constant
        inputs.append(coef)
        wants.append(np.array(prover.debug_lde(coef, n, blowup)))  # a copy of its own
    for flags, coef, want in zip(patterns, inputs, wants):
        got = np.asarray(prover.debug_lde_skip(coef, n, blowup, flags))
        for k in range(npoly):
            assert np.array_equal(got[k], want[k]), (flags.tolist(), k)
        for k in np.flatnonzero(flags):
            assert (want[k] == coef[k, 0]).all()


@pytest.mark.parametrize("n,blowup,npoly", _FWD)
def test_lde_with_flags_equals_lde_without(prover, n, blowup, npoly):
    pats = _flag_patterns(npoly)[:2 if npoly == 2 else 3]  # two polynomials: alternating is first only
    _check_lde_skip(prover, n, blowup, npoly, pats, n + 100 * blowup + npoly)


def test_lde_r1024_pair_with_one_flagged(prover):
    """ntt_pass_a_r1024 / ntt_pass_b_r1024 (2^20 x 16), two polynomials, one flagged: the skip test sits
    behind the coset-consecutive block renumbering"""
    _check_lde_skip(prover, 1 << 20, 16, 2, [np.array([0, 1], dtype=np.uint8)], 77)


@pytest.mark.parametrize("n,off7,npoly", _INV)
def test_interpolate_with_flags_equals_interpolate_without(prover, n, off7, npoly):
    rng = np.random.default_rng(n + (1 if off7 else 0))
    pats = _flag_patterns(npoly)[:2 if npoly == 2 else 3]
    inputs, wants = [], []
    for flags in pats:  # every unflagged run first, as in _check_lde_skip
        ev = rng.integers(0, P, size=(npoly, n), dtype=np.uint64)
        ev[flags != 0] = ev[flags != 0, :1]  # a flagged polynomial is truly constant
        inputs.append(ev)
        wants.append(np.array(prover.debug_interpolate(ev, n, off7)))
    for flags, ev, want in zip(pats, inputs, wants):
        got = np.asarray(prover.debug_interpolate_skip(ev, n, flags, off7))
        for k in range(npoly):
            assert np.array_equal(got[k], want[k]), (flags.tolist(), k)
        for k in np.flatnonzero(flags):
            assert want[k, 0] == ev[k, 0] and not want[k, 1:].any()


# ---------------------------------------------------------------- whole proofs against the oracle
def _air_of(air):
    oa = O.Air()
    for i in range(12):
        oa.pub[i] = air[0][i]
    oa.secret = 0
    oa.nullifier = air[1]
    oa.commitment = air[2]
    return oa


def _trace(kind, n, seed):
    """7 columns of n canonical values: 'all' constant, 'none' constant, 'one_off' (every column constant
    but for one row, the rows of the detection cases), or ('only', c): column c alone constant"""
    rng = random.Random(seed)
    rand_col = lambda: [rng.randrange(P) for _ in range(n)]
    if kind == "all":
        return [[rng.randrange(P)] * n for _ in range(7)]
    if kind == "none":
        return [rand_col() for _ in range(7)]
    if kind == "one_off":
        rows = _off_rows(n)
        tr = []
        for c in range(7):
            v = rng.randrange(P)
            col = [v] * n
            col[rows[c % len(rows)]] = (v + 1 + rng.randrange(P - 1)) % P
            tr.append(col)
        return tr
    assert kind[0] == "only"
    return [[rng.randrange(P)] * n if c == kind[1] else rand_col() for c in range(7)]


def _prove_and_compare(prover, ext, n, blowup, kind):
    import xfgstark
    seed = 9000 + 100 * ext + 3 * n + blowup
    tr = _trace(kind, n, seed)
    air = R.small_air(seed + 1)
    oa = _air_of(air)
    flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr for v in col])
    opts = O.options(blowup=blowup, field_extension=ext)
    st, want = O.prove(oa, n, opts, trace=flat)
    assert st == 0
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension = blowup, ext
    prover._options = o
    try:
        got = prover.prove_trace(np.array(tr, dtype=np.uint64), air[0], air[1], air[2]).to_bytes()
        assert got == want
        # a false statement: the oracle verifier, the host verifier and the GPU batch verifier reject
        assert O.verify(oa, got, opts) != 0
        v = xfgstark.XfgBurnMintVerifier(proof_options=o)
        assert v.batch_verify([(got, air)]) == [False]
        assert v.batch_verify([(got, air)], gpu=prover) == [False]
    finally:
        prover._options = xfgstark.ProofOptions.reference()


@pytest.mark.parametrize("kind", ["all", "none", "one_off"])
@pytest.mark.parametrize("n,blowup", [(8, 8), (64, 2), (1024, 16), (4096, 8)])
@pytest.mark.parametrize("ext", [1, 2])
def test_prove_trace_bytes_match_oracle(prover, ext, n, blowup, kind):
    """every NTT of the trace skipped, none skipped, and none skipped although every column is constant
    but for one row: the GPU proof equals the oracle's byte for byte"""
    _prove_and_compare(prover, ext, n, blowup, kind)


@pytest.mark.parametrize("col", range(7))
@pytest.mark.parametrize("ext", [1, 2])
def test_prove_trace_single_constant_column(prover, ext, col):
    """one column constant at a time: a swapped flag or column index changes the bytes"""
    _prove_and_compare(prover, ext, 64, 2, ("only", col))
