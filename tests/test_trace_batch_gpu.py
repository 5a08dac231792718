"""GPU: batches of caller-supplied traces (xfg_prove_trace_batch / _submit) and the on-device
Trace::validate (xfg_check_traces, XFG_TRACE_VALIDATE), from host arrays and from device tensors.

  * the check kernel against tests/trace_check_ref.py on traces with planted faults,
  * whole batches against the CPU oracle's bytes, proof by proof (O.prove with the same trace),
  * validation inside a batch, and the refusals.
"""
import ctypes as C
import functools

import numpy as np
import pytest
# before the first import of xfgstark (which every test here makes when it runs), as tests/test_dist.py
# does: a torch wheel that bundles its HIP runtime and the library then share the one runtime torch loaded,
# and a tensor's data_ptr() is a device pointer the library's calls know
import torch

import oracle_lib as O
import plain_ref as R
import trace_check_ref as T

pytestmark = pytest.mark.gpu
P = R.P


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _tensor(arr):
    """a uint64 numpy array as an int64 tensor on the prover's device (the bits are kept)"""
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")


def _input(arr, where):
    return arr if where == "host" else _tensor(arr)


def _fault_tuple(f):
    return None if f is None else f.astuple()


# ---------------------------------------------------------------- the check kernel against the reference
@functools.lru_cache(maxsize=None)
def _check_batch(n):
    """every planted case of n and three random traces as one batch: (traces [count][7][n], airs, expected)"""
    cases = [(tr, air) for _, tr, air, _ in T.planted_cases(n)] + T.random_cases(n, [n + 1, n + 2, n + 3])
    traces = np.stack([tr for tr, _ in cases])
    airs = [air for _, air in cases]
    return traces, airs, [T.first_fault(tr, air) for tr, air in cases]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", [8, 64, 512, 4096])
def test_check_kernel_matches_reference(prover, n, where):
    """n = 8: a quarter-filled wave; 512: two blocks, the step + 1 read crosses the block edge"""
    traces, airs, want = _check_batch(n)
    names = [c[0] for c in T.planted_cases(n)] + ["random"] * 3
    got = [_fault_tuple(f) for f in prover.check_traces(_input(traces, where), airs)]
    for name, g, w in zip(names, got, want):
        assert g == w, (name, g, w)
    assert None in got and any(g and g[0] == 1 for g in got) and any(g and g[0] == 2 for g in got)


@pytest.mark.parametrize("where", ["host", "device"])
def test_check_words_do_not_leak_between_proofs(prover, where):
    """count = 3, faults in proofs 0 and 2 only; each trace alone gives the same"""
    n = 512
    cases = {c[0]: c for c in T.planted_cases(n)}
    pick = [cases["c4@255"], cases["valid"], cases["two_steps"]]
    traces = np.stack([c[1] for c in pick])
    airs = [c[2] for c in pick]
    got = [_fault_tuple(f) for f in prover.check_traces(_input(traces, where), airs)]
    assert got == [pick[0][3], None, pick[2][3]]
    for i in range(3):
        assert _fault_tuple(prover.check_traces(_input(traces[i:i + 1], where), airs[i:i + 1])[0]) == got[i]


@pytest.mark.parametrize("where", ["host", "device"])
def test_check_reports_a_non_canonical_cell_for_that_proof_only(prover, where):
    import xfgstark
    n = 64
    tr, air = T.valid_trace(n, 5)
    traces = np.stack([tr, tr, tr])
    traces[1][3][17] = P + 4  # and a fault behind it that must not be reported instead
    traces[1][6][20] = 1
    traces[1][5][40] = (1 << 64) - 1  # a later non-canonical cell
    got = prover.check_traces(_input(traces, where), [air] * 3)
    assert got[0] is None and got[2] is None
    assert got[1] == xfgstark.TraceFault(xfgstark.TraceFault.NONCANONICAL, 0, 3, 17, 0, P + 4)


# ---------------------------------------------------------------- whole batches against the oracle
def _flat(tr):
    return (O.C.c_uint64 * tr.size)(*[int(v) for v in tr.reshape(-1)])


@functools.lru_cache(maxsize=None)
def _proof_batch(count, n, blowup, ext, q):
    """count different traces with their AIRs and the oracle's proof of each: make_trace kinds with
    distinct seeds and valid build_trace ones with distinct AIRs in turn, so that a unit reading
    another unit's slice cannot pass"""
    opts = O.options(blowup=blowup, field_extension=ext, num_queries=q)
    traces, airs, wants = [], [], []
    for i in range(count):
        if i % 4 == 3:
            tr, air = T.valid_trace(n, i)
        else:
            cols, air = R.make_trace(("random", "edge", "wide_consts")[i % 4], n, 500 + 7 * i)
            tr = np.array(cols, dtype=np.uint64)
        st, want = O.prove(T.oracle_air(air), n, opts, trace=_flat(tr))
        assert st == 0
        traces.append(tr)
        airs.append(air)
        wants.append(want)
    return np.stack(traces), airs, wants


def _with_options(prover, blowup, ext, q):
    import xfgstark
    o = xfgstark.ProofOptions.reference()
    o.blowup_factor, o.field_extension, o.num_queries = blowup, ext, q
    prover._options = o
    return o


def _restore(prover):
    import xfgstark
    prover._options = xfgstark.ProofOptions.reference()


def _bytes(res):
    return [r.to_bytes() if hasattr(r, "to_bytes") else ("error", r.status) for r in res]


# 33 and 70 cross the 32-proof unit, 70 leaves a ragged last unit; a lone batch also has its units halved
# for the idle lanes, so slices start at 16-proof offsets too. n = 8 at blowup 2 has a 16-point LDE domain
# and the number of queries must stay below the domain size (42 is refused by prover and oracle alike): 8
PARITY = [(1, 64, 8, 1, 42), (3, 64, 8, 1, 42), (33, 64, 8, 1, 42), (70, 64, 8, 1, 42), (33, 8, 2, 1, 8),
          (5, 4096, 16, 2, 24)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("count,n,blowup,ext,q", PARITY)
def test_batch_bytes_match_oracle(prover, count, n, blowup, ext, q, where):
    big = 70 if (n, blowup) == (64, 8) else count  # the n = 64 cases are prefixes of one batch
    traces, airs, wants = _proof_batch(big, n, blowup, ext, q)
    traces, airs, wants = traces[:count], airs[:count], wants[:count]
    _with_options(prover, blowup, ext, q)
    try:
        inp = _input(traces, where)
        got = _bytes(prover.prove_traces(inp, airs))
        for i in range(count):
            assert got[i] == wants[i], i
        if where == "device":  # the caller's buffer is only read
            assert np.array_equal(inp.cpu().numpy().view(np.uint64), traces)
    finally:
        _restore(prover)


def test_two_submissions_back_to_back(prover):
    """submit_traces twice (host array, device tensor), then both waits: the same bytes"""
    traces, airs, wants = _proof_batch(70, 64, 8, 1, 42)
    a = prover.submit_traces(traces[:33], airs[:33])
    b = prover.submit_traces(_tensor(traces[33:]), airs[33:])
    assert _bytes(a.result()) + _bytes(b.result()) == wants


def test_one_trace_equals_prove_trace(prover):
    traces, airs, wants = _proof_batch(70, 64, 8, 1, 42)
    one = prover.prove_trace(traces[2], *airs[2]).to_bytes()
    assert _bytes(prover.prove_traces(traces[2:3], airs[2:3])) == [one] and one == wants[2]


# ---------------------------------------------------------------- validation inside a batch
@functools.lru_cache(maxsize=None)
def _validation_batch():
    """33 valid traces of 33 AIRs, with a fault planted at 0, 31 and 32 (the last proof of the first
    unit, the lone proof of the second): (traces, airs, oracle proofs of the traces as they are, expected faults)"""
    n, opts = 64, O.options()
    traces, airs, wants, faults = [], [], [], []
    for i in range(33):
        tr, air = T.valid_trace(n, 100 + i)
        if i == 0:
            tr[4][n - 1] = 2  # assertion 7
        elif i == 31:
            tr[5][n - 2] = 77  # constraint 5 at the last checked step
        elif i == 32:
            tr[4][9] = 6  # constraint 4, reported by the step before
        st, want = O.prove(T.oracle_air(air), n, opts, trace=_flat(tr))
        assert st == 0
        traces.append(tr)
        airs.append(air)
        wants.append(want)
        faults.append(T.first_fault(tr, air))
    assert [i for i, f in enumerate(faults) if f] == [0, 31, 32]
    assert faults[0] == (1, 7, 4, n - 1, 3, 2) and faults[31] == (2, 5, 0, n - 2, 0, 0) and faults[32] == (2, 4, 0, 8, 0, 0)
    return np.stack(traces), airs, wants, faults


@pytest.mark.parametrize("where", ["host", "device"])
def test_validation_rejects_the_invalid_traces_only(prover, where):
    import xfgstark
    traces, airs, wants, faults = _validation_batch()
    pending = prover.submit_traces(_input(traces, where), airs, validate=True)
    res = pending.result()
    verifier = xfgstark.XfgBurnMintVerifier()
    for i in range(33):
        if faults[i]:
            assert isinstance(res[i], xfgstark.XfgStarkError) and res[i].status == 11 and res[i].kind == "INVALID_TRACE"
            assert res[i].fault.astuple() == faults[i] and str(res[i]) == str(res[i].fault)
            assert pending._lens[i] == 0 and pending._sts[i] == 11
        else:
            assert res[i].to_bytes() == wants[i], i
            assert verifier.verify_with_public_inputs(res[i], airs[i])
    # xfg_last_error: Winterfell's message for the last invalid proof
    assert str(prover._err(11)) == "main transition constraint 4 did not evaluate to ZERO at step 8"


@pytest.mark.parametrize("where", ["host", "device"])
def test_without_validation_every_trace_is_proven(prover, where):
    traces, airs, wants, _ = _validation_batch()
    assert _bytes(prover.prove_traces(_input(traces, where), airs)) == wants


@pytest.mark.parametrize("where", ["host", "device"])
def test_validation_leaves_valid_batches_alone(prover, where):
    traces, airs, wants, faults = _validation_batch()
    ok = [i for i in range(33) if not faults[i]]
    inp = _input(traces[ok], where)
    sel = [airs[i] for i in ok]
    with_check = _bytes(prover.prove_traces(inp, sel, validate=True))
    assert with_check == _bytes(prover.prove_traces(inp, sel)) == [wants[i] for i in ok]


# ---------------------------------------------------------------- refusals
def _status_of(call):
    import xfgstark
    with pytest.raises(xfgstark.XfgStarkError) as e:
        call()
    assert str(e.value)
    return e.value.status


def test_refused_arguments(prover):
    import xfgstark
    traces, airs, _ = _proof_batch(70, 64, 8, 1, 42)
    three, airs3 = traces[:3], airs[:3]
    assert _status_of(lambda: prover.prove_traces(three[:, :6, :], airs3)) == 9  # width 6
    assert _status_of(lambda: prover.check_traces(three[:, :6, :], airs3)) == 9
    assert _status_of(lambda: prover.prove_traces(three[:0], [])) == 9  # count 0
    assert _status_of(lambda: prover.check_traces(three[:0], [])) == 9
    assert _status_of(lambda: prover.prove_traces(three, airs[:2])) == 9
    bad_air = (list(airs3[0][0][:11]) + [P], airs3[0][1], airs3[0][2])
    assert _status_of(lambda: prover.prove_traces(three, [airs3[0], bad_air, airs3[2]])) == 9
    # options check_request refuses: n = 4 with folding factor 3
    o = xfgstark.ProofOptions.reference()
    o.fri_folding_factor = 3
    prover._options = o
    try:
        assert _status_of(lambda: prover.prove_traces(np.zeros((2, 7, 4), dtype=np.uint64), airs[:2])) == 6
    finally:
        _restore(prover)


def test_null_arrays_are_refused(prover):
    import xfgstark
    lib = xfgstark._lib
    traces, airs, _ = _proof_batch(70, 64, 8, 1, 42)
    tr = np.ascontiguousarray(traces[:2])
    _, ptr, count, width, n, air_p, flags = prover._trace_args(tr, airs[:2])
    o = prover._options._c()
    outs = (xfgstark._u8p * 2)()
    lens = (C.c_size_t * 2)(0, 0)
    sts = (C.c_int * 2)()
    ticket = C.c_uint64(0)
    args = [prover._ctx, count, ptr, width, n, air_p, C.byref(o), flags, outs, lens, sts, None, C.byref(ticket)]
    for null_at in (2, 5, 6, 9, 10, 12):
        a = list(args)
        a[null_at] = None
        assert lib.xfg_prove_trace_batch_submit(*a) == 9
        assert str(prover._err(9)) == "null argument"
    faults = (xfgstark._TraceFault * 2)()
    assert lib.xfg_check_traces(prover._ctx, 2, None, n, air_p, 0, faults) == 9
    assert lib.xfg_check_traces(prover._ctx, 2, ptr, n, None, 0, faults) == 9
    assert lib.xfg_check_traces(prover._ctx, 2, ptr, n, air_p, 0, None) == 9
    assert lib.xfg_check_traces(prover._ctx, 2, ptr, n, air_p, 4, faults) == 9  # an unknown flag


@pytest.mark.parametrize("where", ["host", "device"])
def test_non_canonical_cell_fails_that_proof_only(prover, where):
    import xfgstark
    traces, airs, wants = _proof_batch(70, 64, 8, 1, 42)
    three = traces[:3].copy()
    three[1][2][5] = P
    pending = prover.submit_traces(_input(three, where), airs[:3])
    res = pending.result()
    assert isinstance(res[1], xfgstark.XfgStarkError) and res[1].status == 9
    assert res[1].fault == xfgstark.TraceFault(3, 0, 2, 5, 0, P)
    assert res[0].to_bytes() == wants[0] and res[2].to_bytes() == wants[2]


def test_tensors_the_lanes_cannot_read_are_refused(prover):
    traces, airs, _ = _proof_batch(70, 64, 8, 1, 42)
    host = torch.from_numpy(traces[:2].view(np.int64))
    assert _status_of(lambda: prover.prove_traces(host, airs[:2])) == 9  # not on the prover's device
    assert _status_of(lambda: prover.check_traces(host, airs[:2])) == 9
    dev = _tensor(traces[:2])
    assert _status_of(lambda: prover.prove_traces(dev.transpose(1, 2), airs[:2])) == 9  # not contiguous
    assert _status_of(lambda: prover.prove_traces(dev.to(torch.int32), airs[:2])) == 9  # wrong dtype
