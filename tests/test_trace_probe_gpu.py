"""GPU: the columns of a generated trace are classified from the rows as the generator returns them, and
only the live ones are written (csrc/columns.hip trace_probe_kernel, trace_gen_kernel).

Through xfg_debug_trace_probe, which runs the front end of a generated unit as the chain does on a trace
buffer of 0xFF bytes:
  * a synthetic generator, one pattern per column, makes the probe say something other than the burn
    pattern: its classes and values against the detection on the same trace materialised
    (xfg_debug_col_classes) and against numpy, and the buffer as left against the numpy trace: live planes
    equal, every other plane still 0xFF bytes;
  * the burn generator on real AIR constants;
  * whole generated batches, every buffer poisoned (xfg_debug_poison_lde: the trace too, ahead of the
    generator), byte for byte against the CPU oracle."""
import functools

import numpy as np
import pytest

import fold_cases as FC
import oracle_lib as O
import synthetic

gpu = pytest.mark.gpu  # test_pattern_expectations alone needs no GPU
DETECT_SPAN = 1024  # rows per detection block (CONST_DETECT_SPAN, csrc/columns.hpp)
POISON = np.uint64(0xFFFFFFFFFFFFFFFF)
CONST, ROWS, ROWS_PROOF, CONST_BUT, SHARED_BUT = range(5)  # xfg_probe_pattern kinds


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    pr.debug_poison_lde(True)
    yield pr
    pr._options = xfgstark.ProofOptions.reference()
    pr.debug_poison_lde(False)
    pr.close()


# ---------------------------------------------------------------- the synthetic generator in numpy
def _airs(B, first_differs=False):
    """per-proof values pub[c] (distinct over proofs and columns; first_differs: proofs 1.. agree with each
    other and not with proof 0) and the proof's tag pub[7] = b"""
    airs = []
    for b in range(B):
        v = b if not first_differs else min(b, 1)
        pub = [1000 * (v + 1) + 10 * c for c in range(7)] + [b, 0, 0, 0, 0]
        airs.append((pub, 0, 0))
    return airs


def _synth_np(airs, pattern, n):
    """the trace [B][7][n] of xfg_probe_pattern (include/xfg_stark.h)"""
    kind, row, proof = pattern
    i = np.arange(n, dtype=np.uint64)
    tr = np.empty((len(airs), 7, n), dtype=np.uint64)
    for b, (pub, _, _) in enumerate(airs):
        for c in range(7):
            v, f, hit = np.uint64(pub[c]), np.uint64(3) * i + np.uint64(c), (i == np.uint64(row[c])).astype(np.uint64)
            k = kind[c]
            tr[b, c] = (v if k == CONST else f if k == ROWS else f + v if k == ROWS_PROOF else v + hit
                        if k == CONST_BUT else f + (hit if pub[7] == proof else np.uint64(0)))
    return tr


def _classes_np(tr):
    """0 live, 1 constant, 2 equal to trace 0's column (never trace 0 itself); constant wins"""
    const = (tr == tr[:, :, :1]).all(axis=2)
    same = (tr == tr[:1]).all(axis=2)
    same[0] = False
    return np.where(const, 1, np.where(same, 2, 0)).astype(np.uint8)


def _rows(n):
    return [1, n - 1] + ([DETECT_SPAN - 1, DETECT_SPAN] if n == 4 * DETECT_SPAN else [])


def _cases(family, n, B):
    """(label, airs, pattern)"""
    if family == "basic":
        yield "all constant", _airs(B), ([CONST] * 7, [0] * 7, 0)
        yield "none constant", _airs(B), ([ROWS_PROOF] * 7, [0] * 7, 0)
        yield "all shared", _airs(B), ([ROWS] * 7, [0] * 7, 0)
        yield "first differs", _airs(B, first_differs=True), ([ROWS_PROOF] * 7, [0] * 7, 0)
        yield "one of each", _airs(B), ([CONST, ROWS, ROWS_PROOF, CONST_BUT, SHARED_BUT, ROWS, CONST], [n - 1] * 7, B - 1)
    for c in range(7):
        for r in _rows(n):
            if family == "const_but":  # column c alone is constant except at row r, in every proof
                kind = [CONST] * 7
                kind[c] = CONST_BUT
                yield f"col {c} row {r}", _airs(B), (kind, [r] * 7, 0)
            if family == "shared_but":  # column c equals proof 0's except at row r of the last proof
                kind = [ROWS] * 7
                kind[c] = SHARED_BUT
                yield f"col {c} row {r}", _airs(B), (kind, [r] * 7, B - 1)


@gpu
@pytest.mark.parametrize("family", ["basic", "const_but", "shared_but"])
@pytest.mark.parametrize("B", [1, 2, 3, 33])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])  # one short block, ..., four detection spans
def test_probe_equals_detection_and_only_live_planes_are_written(prover, n, B, family):
    for label, airs, pattern in _cases(family, n, B):
        tr = _synth_np(airs, pattern, n)
        want = _classes_np(tr)
        cls, vals, buf = prover.debug_trace_probe(airs, n, generator=1, pattern=pattern)
        ref_cls, ref_vals = prover.debug_col_classes(tr, values=True)
        assert np.array_equal(cls, ref_cls) and np.array_equal(vals, ref_vals), label
        assert np.array_equal(cls, want) and np.array_equal(vals, tr[:, :, 0]), label
        live = want == 0
        assert np.array_equal(buf[live], tr[live]), label
        assert (buf[~live] == POISON).all(), label


def test_pattern_expectations():
    """what the pattern families are meant to produce, on the CPU alone"""
    n, B = 64, 3
    got = {label: _classes_np(_synth_np(airs, pat, n)).tolist() for label, airs, pat in _cases("basic", n, B)}
    assert got["all constant"] == [[1] * 7] * 3
    assert got["none constant"] == [[0] * 7] * 3
    assert got["all shared"] == [[0] * 7, [2] * 7, [2] * 7]
    assert got["first differs"] == [[0] * 7] * 3
    assert got["one of each"] == [[1, 0, 0, 0, 0, 0, 1], [1, 2, 0, 0, 2, 2, 1], [1, 2, 0, 0, 0, 2, 1]]
    for label, airs, pat in _cases("const_but", n, B):
        c = pat[0].index(CONST_BUT)
        assert _classes_np(_synth_np(airs, pat, n)).tolist() == [[0 if k == c else 1 for k in range(7)]] * 3, label
    for label, airs, pat in _cases("shared_but", n, B):
        c = pat[0].index(SHARED_BUT)
        want = [[0] * 7, [2] * 7, [0 if k == c else 2 for k in range(7)]]
        assert _classes_np(_synth_np(airs, pat, n)).tolist() == want, label


# ---------------------------------------------------------------- the burn generator
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [8, 64, 4096])
def test_burn_generator(prover, n, B):
    import xfgstark
    airs = [xfgstark.air_consts(**synthetic.burn_inputs(7300 + i)) for i in range(B)]
    cls, vals, buf = prover.debug_trace_probe(airs, n)
    assert cls.tolist() == [[1, 1, 1, 1, 0, 1, 1]] + [[1, 1, 1, 1, 2, 1, 1]] * (B - 1)
    assert vals.tolist() == [list(pub[:4]) + [0, nullifier, commitment] for pub, nullifier, commitment in airs]
    state = (4 * np.arange(n, dtype=np.uint64)) >> np.uint64(n.bit_length() - 1)
    assert np.array_equal(buf[0, 4], state)
    buf[0, 4] = POISON
    assert (buf == POISON).all()  # one plane per unit is written


# ---------------------------------------------------------------- whole generated batches, poisoned
@functools.lru_cache(maxsize=None)
def _oracle_proof(i, n, blowup, ext):
    st, pr = O.prove(FC.oracle_air(synthetic.burn_inputs(7400 + i)), n, O.options(blowup=blowup, field_extension=ext))
    assert st == 0
    return pr


@gpu
@pytest.mark.parametrize("B", [1, 3, 33])  # 33: a full unit and a unit of one
@pytest.mark.parametrize("n,blowup", [(8, 8), (64, 2), (1024, 16)])
@pytest.mark.parametrize("ext", [1, 2])
def test_generated_batch_matches_oracle_with_poisoned_buffers(prover, ext, n, blowup, B):
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension = blowup, ext
    prover._options = o
    got = prover.prove_batch([synthetic.burn_inputs(7400 + i) for i in range(B)], trace_length=n)
    for i in range(B):
        assert got[i].to_bytes() == _oracle_proof(i, n, blowup, ext), i
