"""GPU: batches of caller-supplied traces in strided layouts (xfg_prove_trace_batch_strided / _submit,
xfg_check_traces_strided) and the two ingest kernels behind them (xfg_debug_trace_ingest), on the layouts of
tests/trace_layout_cases.py.

  * the ingest kernels against tests/trace_check_ref.py and a numpy classification, layout by layout,
  * check_traces on a view against check_traces on the materialised copy,
  * whole batches against the CPU oracle's bytes (the batches and oracle proofs of tests/test_trace_batch_gpu.py,
    computed once for both files),
  * a poisoned workspace, and the refusals.
"""
import ctypes as C
import functools

import numpy as np
import pytest
# before the first import of xfgstark, as tests/test_trace_batch_gpu.py does: one HIP runtime for torch and the library
import torch

import oracle_lib as O
import test_trace_batch_gpu as TB
import trace_check_ref as T
import trace_layout_cases as L

pytestmark = pytest.mark.gpu
P = L.P
FF = np.uint64((1 << 64) - 1)
SIZES = [8, 64, 512, 4096]


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _ingest(prover, case, airs, validate=False):
    """the hook on a layout's buffer from cell (0, 0, 0) on: exactly the extent, no word more"""
    return prover.debug_trace_ingest(case.flat[case.offset:], case.layout, case.count, case.n, airs, validate)


def _expected_faults(traces, airs):
    """first_fault of every trace, computed once per distinct (trace, AIR): a broadcast batch repeats trace 0"""
    memo = {}
    out = []
    for tr, air in zip(traces, airs):
        key = (tr.tobytes(), repr(air))
        if key not in memo:
            memo[key] = T.first_fault(tr, air)
        out.append(memo[key])
    return out


@functools.lru_cache(maxsize=None)
def _check_case(name, n):
    """the planted and random cases of n in layout `name`: (Layout, airs, names, expected faults of what the
    layout names)"""
    traces, airs, names, want = L.check_batch(n)
    case = L.Layout(name, traces)
    if name == "broadcast":
        want = _expected_faults(case.materialise(), airs)
    return case, airs, names, want


# ---------------------------------------------------------------- 1. the ingest kernels against references
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", L.NAMES)
def test_ingest_classes_and_live_planes(prover, name, n):
    """n = 8: a quarter-filled wave and a tile shorter than a block; 512: two blocks; 4096: sixteen"""
    traces, airs = L.class_batch(n)
    case = L.Layout(name, traces)
    dense = case.materialise()
    cls, vals, faults, left = _ingest(prover, case, airs)
    want_cls, want_vals = L.classify(dense)
    assert np.array_equal(cls, want_cls), (cls, want_cls)
    assert np.array_equal(vals, want_vals)
    ref_cls, ref_vals = prover.debug_col_classes(L.canonical(dense), values=True)
    assert np.array_equal(cls, ref_cls) and np.array_equal(vals, ref_vals)
    assert faults == [None] * case.count  # canonical cells, no validation
    for i in range(case.count):
        for c in range(7):
            if cls[i][c] == 0:
                assert np.array_equal(left[i][c], dense[i][c]), (i, c)
            else:
                assert (left[i][c] == FF).all(), (i, c)
    if name != "broadcast":
        assert (cls == 0).any() and (cls == 1).any() and (cls == 2).any() and (cls[2] != 0).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", L.NAMES)
def test_ingest_check_matches_reference(prover, name, n):
    """with validation the faults are first_fault's on the planted and random cases (512: the step + 1 read
    crosses the block edge, and the last block's tile has no extra row); without it nothing but a cell >= p is
    ever reported"""
    case, airs, names, want = _check_case(name, n)
    _, _, got, _ = _ingest(prover, case, airs, validate=True)
    for nm, g, w in zip(names, got, want):
        assert g == w, (nm, g, w)
    if name != "broadcast":
        assert None in got and any(g and g[0] == 1 for g in got) and any(g and g[0] == 2 for g in got)
    _, _, quiet, _ = _ingest(prover, case, airs, validate=False)
    assert quiet == [None] * case.count


@pytest.mark.parametrize("validate", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", L.NAMES)
def test_ingest_reports_a_non_canonical_cell_for_that_proof_only(prover, name, n, validate):
    tr, air = T.valid_trace(n, 5)
    traces = np.stack([tr, tr, tr])
    s = n // 2 + 1
    victim = 0 if name == "broadcast" else 1  # with a broadcast layout there is only trace 0
    traces[victim][3][s] = P + 4
    traces[victim][6][s + 1] = 1  # an AIR fault behind it that must not be reported instead
    traces[victim][5][n - 2] = FF  # a later non-canonical cell
    case = L.Layout(name, traces)
    cls, vals, got, left = _ingest(prover, case, [air] * 3, validate)
    hit = (3, 0, 3, s, 0, P + 4)
    assert got == ([hit] * 3 if name == "broadcast" else [None, hit, None])
    # the cell's column is no longer constant: its plane is written, and holds the canonical value 4
    dense = L.canonical(case.materialise())
    assert list(cls[:, 3]) == ([0, 2, 2] if name == "broadcast" else [1, 0, 1])
    assert np.array_equal(left[victim][3], dense[victim][3]) and left[victim][3][s] == 4
    assert np.array_equal(vals, dense[:, :, 0])
    if validate and name != "broadcast":  # without the cell the fault behind it is what is reported
        traces[1][3][s] = 4
        traces[1][5][n - 2] = tr[5][n - 2]
        _, _, got, _ = _ingest(prover, L.Layout(name, traces), [air] * 3, True)
        assert got[0] is None and got[2] is None and got[1] == T.first_fault(traces[1], air) and got[1][0] in (1, 2)


# ---------------------------------------------------------------- 2. check_traces on views
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", [8, 512])
@pytest.mark.parametrize("name", L.NAMES)
def test_check_traces_on_a_view_equals_the_materialised_copy(prover, name, n, where):
    traces, airs, _, _ = L.check_batch(n)
    traces = traces.copy()
    traces[0 if name == "broadcast" else 1][2][n - 3] = P + 4  # one trace gets a cell >= p (broadcast: there is only trace 0)
    case = L.Layout(name, traces)
    dense = case.materialise()
    view = case.view if where == "host" else case.tensor()
    got = [TB._fault_tuple(f) for f in prover.check_traces(view, airs)]
    text = str(prover._err(9))
    want = [TB._fault_tuple(f) for f in prover.check_traces(TB._input(dense, where), airs)]
    assert got == want and text == str(prover._err(9))
    assert (3, 0, 2, n - 3, 0, P + 4) in got
    if where == "device":  # the caller's buffer is only read
        back = torch.as_strided(view, (len(case.flat),), (1,), 0).cpu().numpy().view(np.uint64)
        assert np.array_equal(back, case.flat)


# ---------------------------------------------------------------- 3. proof bytes
SHAPES = [(3, 64, 8, 1, 42), (70, 64, 8, 1, 42), (33, 8, 2, 1, 8), (5, 4096, 16, 2, 24)]
PROOF_CASES = ([(name, where) + sh for sh in SHAPES for name in ("rows7", "rows8") for where in ("device", "host")] +
               [(name, "device") + SHAPES[0] for name in ("batch_inner", "broadcast")])


def _batch(count, n, blowup, ext, q):
    big = 70 if (n, blowup) == (64, 8) else count  # the n = 64 cases are prefixes of one batch, as in TB
    traces, airs, wants = TB._proof_batch(big, n, blowup, ext, q)
    return traces[:count], airs[:count], wants[:count]


@pytest.mark.parametrize("name,where,count,n,blowup,ext,q", PROOF_CASES)
def test_view_bytes_match_oracle(prover, name, where, count, n, blowup, ext, q):
    """70 crosses the 32-proof units, leaves a ragged last unit and, as a lone batch, has its units halved: every
    slice starts trace_stride words per proof further on"""
    traces, airs, wants = _batch(count, n, blowup, ext, q)
    case = L.Layout(name, traces)
    TB._with_options(prover, blowup, ext, q)
    try:
        view = case.view if where == "host" else case.tensor()
        got = TB._bytes(prover.prove_traces(view, airs))
        if name == "broadcast":  # every proof on trace 0 under its own AIR: what the dense run makes of that
            wants = TB._bytes(prover.prove_traces(TB._input(case.materialise(), where), airs))
            assert wants[0] == _batch(count, n, blowup, ext, q)[2][0]
        for i in range(count):
            assert got[i] == wants[i], i
        if where == "device":
            back = torch.as_strided(view, (len(case.flat),), (1,), 0).cpu().numpy().view(np.uint64)
            assert np.array_equal(back, case.flat)
    finally:
        TB._restore(prover)


@pytest.mark.parametrize("where", ["host", "device"])
def test_dense_layout_spelled_out_is_the_dense_run(prover, where):
    """{7n, n, 1} at the raw strided entries (the package sends a contiguous array to the entries without a
    layout): the oracle's bytes, the faults of check_traces on the dense array, and a device buffer only read"""
    import xfgstark
    lib = xfgstark._lib
    count, n, blowup, ext, q = SHAPES[0]
    traces, airs, wants = _batch(count, n, blowup, ext, q)
    dense = np.ascontiguousarray(traces)
    held = TB._input(dense, where)
    ptr, flags = (dense.ctypes.data, 0) if where == "host" else (held.data_ptr(), xfgstark.TRACE_ON_DEVICE)
    air_np, air_p = xfgstark._marshal.air_array(airs)
    at = xfgstark._TraceLayout(7 * n, n, 1)
    want_faults = [TB._fault_tuple(f) for f in prover.check_traces(held, airs)]
    assert any(want_faults)  # the random traces violate the AIR: the faults compared below are not all None
    faults = (xfgstark._TraceFault * count)()
    assert lib.xfg_check_traces_strided(prover._ctx, count, ptr, n, C.byref(at), air_p, flags, faults) == 0
    assert [TB._fault_tuple(xfgstark.TraceFault._from_c(faults[i])) for i in range(count)] == want_faults
    TB._with_options(prover, blowup, ext, q)
    try:
        o, cap = prover._options._c_and_bound(n)
        bufs = [C.create_string_buffer(cap) for _ in range(count)]
        outs = (xfgstark._u8p * count)(*[C.cast(b, xfgstark._u8p) for b in bufs])
        lens, sts = (C.c_size_t * count)(*[cap] * count), (C.c_int * count)()
        assert lib.xfg_prove_trace_batch_strided(prover._ctx, count, ptr, n, C.byref(at), air_p, C.byref(o), flags, outs,
                                                 lens, sts, None) == 0
    finally:
        TB._restore(prover)
    assert list(sts) == [0] * count
    for i in range(count):
        assert C.string_at(bufs[i], lens[i]) == wants[i], i
    if where == "device":
        assert np.array_equal(held.cpu().numpy().view(np.uint64), dense)


def test_two_submissions_back_to_back(prover):
    """submit_traces twice, from a row-major view and from a dense tensor, then both waits"""
    traces, airs, wants = _batch(70, 64, 8, 1, 42)
    a = prover.submit_traces(L.Layout("rows8", traces[:33]).tensor(), airs[:33])
    b = prover.submit_traces(TB._tensor(traces[33:]), airs[33:])
    assert TB._bytes(a.result()) + TB._bytes(b.result()) == wants


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["rows7", "rows8"])
def test_validation_in_a_view_equals_the_dense_run(prover, name, where):
    """valid traces, traces with planted faults and a non-canonical one: statuses, faults, texts and the
    untouched proofs' bytes"""
    traces, airs, wants, faults = TB._validation_batch()
    traces = traces.copy()
    traces[5][2][5] = P
    case = L.Layout(name, traces)

    def run(inp):
        pending = prover.submit_traces(inp, airs, validate=True)
        res = pending.result()
        return ([(r.status, TB._fault_tuple(r.fault), str(r)) if isinstance(r, Exception) else r.to_bytes() for r in res],
                list(pending._sts), list(pending._lens), str(prover._err(11)))

    got = run(case.view if where == "host" else case.tensor())
    want = run(TB._input(traces, where))
    assert got == want
    res = got[0]
    assert res[5] == (9, (3, 0, 2, 5, 0, P), "trace element is not a canonical field element")
    for i in (0, 31, 32):
        assert res[i][0] == 11 and res[i][1] == faults[i]
    for i in range(33):
        if i not in (0, 5, 31, 32):
            assert res[i] == wants[i], i


# ---------------------------------------------------------------- 4. poison
@pytest.mark.parametrize("ext", [1, 2])
def test_poisoned_workspace_changes_nothing(prover, ext):
    """the ingest leaves the planes of constant and shared columns unwritten: with the trace, coefficient and
    LDE buffers set to 0xFF bytes first, the bytes are still the oracle's, so nothing reads such a plane"""
    n = 64
    traces, airs = L.class_batch(n)
    opts = O.options(field_extension=ext)
    wants = []
    for tr, air in zip(traces, airs):
        st, want = O.prove(T.oracle_air(air), n, opts, trace=TB._flat(tr))
        assert st == 0
        wants.append(want)
    TB._with_options(prover, 8, ext, 42)
    prover.debug_poison_lde(True)
    try:
        got = TB._bytes(prover.prove_traces(L.Layout("rows7", traces).tensor(), airs))
    finally:
        prover.debug_poison_lde(False)
        TB._restore(prover)
    assert got == wants


# ---------------------------------------------------------------- 5. refusals
def test_refused_views(prover):
    traces, airs, _ = _batch(3, 64, 8, 1, 42)
    rows = L.Layout("rows7", traces)
    status = TB._status_of
    for call in (prover.prove_traces, prover.check_traces):
        assert status(lambda: call(rows.view[:, :6, :], airs)) == 9  # width 6
        assert status(lambda: call(rows.tensor()[:, :6, :], airs)) == 9
        assert status(lambda: call(rows.view[:0], [])) == 9  # count 0
        assert status(lambda: call(rows.tensor()[:0], [])) == 9
        assert status(lambda: call(rows.tensor().to(torch.int32), airs)) == 9  # an int32 tensor
        assert status(lambda: call(traces[:, :, ::-1], airs)) == 9  # a negative-stride view
        assert status(lambda: call(rows.view[:, :, ::-1], airs)) == 9


def test_refused_raw_arguments(prover):
    """through ctypes: a device view whose extent exceeds its allocation, null pointers, an unknown flag, a
    stride of 2^63; each XFG_INVALID_ARGUMENT with a text, and nothing is launched"""
    import xfgstark
    lib = xfgstark._lib
    n = 1 << 18
    _, airs, _ = _batch(3, 64, 8, 1, 42)
    air_np, air_p = xfgstark._marshal.air_array(airs[:2])
    # n rows are asked of a tensor allocated for n / 2 of them: 14.7 MB short. torch gives a request of this size a
    # segment of its own, rounded up to 2 MB, once no cached segment is left to carve it from
    torch.cuda.empty_cache()
    half = torch.zeros(2 * 7 * (n // 2), dtype=torch.int64, device="cuda:0")
    rows7 = xfgstark._TraceLayout(7 * n, 1, 7)
    faults = (xfgstark._TraceFault * 2)()
    o = prover._options._c()
    outs, lens, sts, ticket = (xfgstark._u8p * 2)(), (C.c_size_t * 2)(0, 0), (C.c_int * 2)(), C.c_uint64(0)

    def check(where, layout, flags=2, air=air_p, f=faults):
        return lib.xfg_check_traces_strided(prover._ctx, 2, where, n, layout, air, flags, f)

    def submit(where, layout, flags=2):
        return lib.xfg_prove_trace_batch_strided_submit(prover._ctx, 2, where, n, layout, air_p, C.byref(o), flags, outs,
                                                        lens, sts, None, C.byref(ticket))

    assert check(half.data_ptr(), C.byref(rows7)) == 9 and "allocation" in str(prover._err(9))
    assert submit(half.data_ptr(), C.byref(rows7)) == 9 and "allocation" in str(prover._err(9))
    assert check(half.data_ptr(), C.byref(xfgstark._TraceLayout(7 * n // 2, 1, 7))) == 9  # n steps: still too long
    full = torch.zeros(2 * 7 * n, dtype=torch.int64, device="cuda:0")
    where = full.data_ptr()
    assert check(None, C.byref(rows7)) == 9 and str(prover._err(9)) == "null argument"
    assert check(where, C.byref(rows7), air=None) == 9
    assert check(where, C.byref(rows7), f=None) == 9
    assert submit(None, C.byref(rows7)) == 9 and str(prover._err(9)) == "null argument"
    assert check(where, C.byref(rows7), flags=4) == 9  # an unknown flag
    assert submit(where, C.byref(rows7), flags=8) == 9 and str(prover._err(9)) == "unknown trace flag"
    for bad in (xfgstark._TraceLayout(1 << 63, 1, 7), xfgstark._TraceLayout(7 * n, 1 << 63, 7),
                xfgstark._TraceLayout(7 * n, 1, 1 << 63)):
        assert check(where, C.byref(bad)) == 9 and "extent" in str(prover._err(9))
        assert submit(where, C.byref(bad)) == 9 and "extent" in str(prover._err(9))
    assert ticket.value == 0
    # the all-zero traces fail the AIR's assertions; that the check runs at all is the point here
    assert check(where, C.byref(rows7)) == 0 and faults[0].kind == 1
    assert check(where, None) == 0 and faults[1].kind == 1  # layout NULL: dense
    # the hook: an extent above the buffer it is given
    buf = np.zeros(2 * 7 * 64 - 1, dtype=np.uint64)
    assert TB._status_of(lambda: prover.debug_trace_ingest(buf, (7 * 64, 1, 7), 2, 64, airs[:2])) == 9
    assert TB._status_of(lambda: prover.debug_trace_ingest(buf, (1 << 63, 1, 7), 2, 64, airs[:2])) == 9
