"""Traces in strided layouts, on the CPU: the host side of the strided entries (xfg-stark_amd/csrc/trace_layout.hpp)
under a sanitizer, and a check that the fixtures of tests/test_trace_layout_gpu.py are not vacuous.

tests/sanitize/trace_layout.cpp is plain C++ with its own main: the extent and its refusals, is_dense, the gather
against a naive triple loop and the strided canonicity key against the dense one, for every layout of
tests/trace_layout_cases.py at n = 8 and 64 (see its header). Here it is built with ASan + UBSan
(`make -C xfg-stark_amd sanitize`) and the binary is run directly: exit 0, nothing from a sanitizer."""
import os
import subprocess

import numpy as np
import pytest

import trace_check_ref as T
import trace_layout_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "xfg-stark_amd")
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:abort_on_error=0:detect_leaks=1:exitcode=77",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1:exitcode=78")
TARGET = "build/asan/trace_layout"


def test_driver_is_clean_under_the_sanitizer():
    subprocess.run(["make", "-s", "-C", LIB, TARGET], check=True)
    r = subprocess.run([os.path.join(LIB, TARGET)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    assert r.stdout == "trace_layout ok\n"


def test_sanitize_target_builds_the_driver():
    subprocess.run(["make", "-s", "-C", LIB, "sanitize"], check=True)
    assert os.path.exists(os.path.join(LIB, "build", "asan", "trace_layout"))


@pytest.mark.parametrize("name", L.NAMES)
@pytest.mark.parametrize("n", [8, 64])
def test_layouts_name_the_cells_they_claim(name, n):
    """the fixtures themselves: a layout's view materialises to the dense array (every trace trace 0 with
    broadcast), the cells lie where the strides say, and every other word of the buffer is the fill"""
    dense, _ = L.class_batch(n)
    case = L.Layout(name, dense)
    want = np.stack([dense[0]] * len(dense)) if name == "broadcast" else dense
    assert np.array_equal(case.materialise(), want)
    ts, cs, rs = case.layout
    assert len(case.flat) == case.offset + L.extent(case.layout, case.count, n)
    used = np.zeros(len(case.flat), dtype=bool)
    for i in range(case.count):
        for c in range(7):
            at = case.offset + i * ts + c * cs + np.arange(n) * rs
            assert np.array_equal(case.flat[at], want[i][c])
            used[at] = True
    assert (case.flat[~used] == L.FILL).all()
    if name in ("rows8", "rows12+3", "rows24", "cols_padded"):
        assert not used.all()  # there are pad words to surface


@pytest.mark.parametrize("n", [8, 64, 512, 4096])
def test_class_batch_has_every_class(n):
    """the numpy classification of the class-test batch finds a live, a constant and a shared column, and a
    proof other than proof 0 none of whose seven columns is live"""
    traces, airs = L.class_batch(n)
    cls, vals = L.classify(traces)
    assert (cls == 0).any() and (cls == 1).any() and (cls == 2).any()
    assert not (cls[0] == 2).any()
    assert any((cls[i] != 0).all() for i in range(1, len(cls)))
    assert np.array_equal(vals, traces[:, :, 0])
    assert len(airs) == len(traces) and (traces < np.uint64(L.P)).all()
    # a non-canonical cell classifies as its canonical value
    t = traces.copy()
    t[1][0][3] += np.uint64(L.P)
    assert np.array_equal(L.classify(t)[0], cls)


@pytest.mark.parametrize("n", [8, 64, 512, 4096])
def test_planted_cases_have_every_kind(n):
    """trace_check_ref.first_fault on the planted and random cases returns assertions, transitions and None"""
    _, _, names, want = L.check_batch(n)
    kinds = {w[0] if w else None for w in want}
    assert kinds == {None, T.ASSERTION, T.TRANSITION}, kinds
    for (name, _, _, stated), w in zip(T.planted_cases(n), want):
        if stated != "ref":
            assert w == stated, name
