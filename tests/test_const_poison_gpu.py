"""GPU: whole proofs of caller-supplied traces with the trace LDE buffer set to 0xFF bytes before every
unit (xfg_debug_poison_lde), byte for byte against the CPU oracle.

The LDE planes of constant columns are never written: the leaf kernels, the constraint evaluation, the
opening kernel and the gather of the opened trace values each take such a column's value from the
flags and coefficient 0 (csrc/columns.hpp ColConst). Without the poison a plane that an earlier unit
left in the lane's buffer can hold the right value, and a reader that still goes to memory would pass.
The trace kinds are those of tests/test_const_columns.py; this is the test that sees the gather."""
import numpy as np
import pytest

import oracle_lib as O
import plain_ref as R
from test_const_columns import _air_of, _trace

pytestmark = pytest.mark.gpu

KINDS = ["all", "none", "one_off"] + [("only", c) for c in range(7)]


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    pr.debug_poison_lde(True)
    yield pr
    pr._options = xfgstark.ProofOptions.reference()
    pr.debug_poison_lde(False)
    pr.close()


def _case(ext, n, blowup, kind, seed):
    """(trace [7][n], air, the oracle's proof bytes)"""
    if kind == "all_but_4":  # the burn proof's own pattern: the state column alone varies
        tr = _trace("all", n, seed)
        tr[4] = _trace("none", n, seed + 2)[4]
    else:
        tr = _trace(kind, n, seed)
    air = R.small_air(seed + 1)
    flat = (O.C.c_uint64 * (7 * n))(*[v for col in tr for v in col])
    st, want = O.prove(_air_of(air), n, O.options(blowup=blowup, field_extension=ext), trace=flat)
    assert st == 0
    return np.array(tr, dtype=np.uint64), air, want


def _set_options(prover, blowup, ext):
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension = blowup, ext
    prover._options = o


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k if isinstance(k, str) else f"only{k[1]}")
@pytest.mark.parametrize("n,blowup", [(8, 8), (64, 2), (1024, 16), (64, 32)])
@pytest.mark.parametrize("ext", [1, 2])
def test_prove_trace_bytes_match_oracle_with_poisoned_lde(prover, ext, n, blowup, kind):
    tr, air, want = _case(ext, n, blowup, kind, 7000 + 100 * ext + 3 * n + blowup)
    _set_options(prover, blowup, ext)
    assert prover.prove_trace(tr, air[0], air[1], air[2]).to_bytes() == want


def test_batch_of_three_flag_patterns_in_one_unit(prover):
    """three traces with different constant columns proven as one unit: each proof's flags and values
    are its own in every kernel (blockIdx.y, the entry's proof, the plane of a gathered index)"""
    ext, n, blowup = 1, 64, 8
    cases = [_case(ext, n, blowup, kind, 8100 + 17 * i) for i, kind in enumerate(["all_but_4", ("only", 4), "none"])]
    flags = prover.debug_const_columns(np.stack([c[0] for c in cases]))
    assert flags.tolist() == [[1, 1, 1, 1, 0, 1, 1], [0, 0, 0, 0, 1, 0, 0], [0] * 7]
    _set_options(prover, blowup, ext)
    got = prover.prove_traces(np.stack([c[0] for c in cases]), [c[1] for c in cases])
    for i, (g, c) in enumerate(zip(got, cases)):
        assert g.to_bytes() == c[2], i
