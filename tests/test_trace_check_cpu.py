"""CPU: the reference of the on-device Trace::validate (tests/trace_check_ref.py) alone, and the presence
of the trace-batch entries in the header, the library and the Python mirror."""
import os
import re

import numpy as np
import pytest

import plain_ref as R
import trace_check_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("xfg_check_traces", "xfg_prove_trace_batch", "xfg_prove_trace_batch_submit")


@pytest.mark.parametrize("n", [8, 64])
def test_oracle_trace_is_valid(n):
    for idx in range(3):
        tr, air = T.valid_trace(n, idx)
        assert T.first_fault(tr, air) is None


@pytest.mark.parametrize("n", [8, 64, 512])
def test_planted_faults_are_classified_as_stated(n):
    cases = T.planted_cases(n)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for k in range(7):  # every constraint at step n - 2, every assertion
        assert f"c{k}@{n - 2}" in names and f"assert{k}" in names
    stated = 0
    for name, tr, air, want in cases:
        got = T.first_fault(tr, air)
        if want == "ref":
            assert n == 8 and got is not None and got[0] == T.TRANSITION, name
            continue
        stated += 1
        assert got == want, (name, got, want)
    assert stated >= len(cases) - 1


def test_order_assertions_then_steps_then_constraints():
    tr, air = T.valid_trace(64, 1)
    t = tr.copy()
    t[6][10] = 1  # constraint 6 at step 10
    t[0][20] = 1  # constraints 0 and 1 at step 20
    assert T.first_fault(t, air) == (T.TRANSITION, 6, 0, 10, 0, 0)
    t[0][10] = 1  # now constraint 0 at step 10 precedes constraint 6 there
    assert T.first_fault(t, air) == (T.TRANSITION, 0, 0, 10, 0, 0)
    t[4][63] = 2  # assertion 7 precedes every transition
    assert T.first_fault(t, air) == (T.ASSERTION, 7, 4, 63, 3, 2)
    t[1][0] = 5  # and assertion 1 precedes assertion 7
    assert T.first_fault(t, air) == (T.ASSERTION, 1, 1, 0, air[0][1], 5)


def test_random_traces_fail_at_the_first_assertion_or_step():
    for tr, air in T.random_cases(64, [1, 2, 3]):
        got = T.first_fault(tr, air)
        assert got is not None and (got[0] == T.ASSERTION or got[3] == 0)


def test_pub_masks_are_applied():
    """constraints 2 and 3 compare with the low 32 bits of the public input, the assertions with all of it"""
    tr, air = T.valid_trace(8, 0)
    pub = list(air[0])
    pub[2] += 1 << 32
    t = tr.copy()
    t[2][0] = pub[2]
    assert T.first_fault(t, (pub, air[1], air[2])) == (T.TRANSITION, 2, 0, 0, 0, 0)
    assert R.transition((pub, air[1], air[2]), [int(t[c][1]) for c in range(7)], [int(t[c][2]) for c in range(7)])[2] == 0


def test_header_library_and_mirror_carry_the_entries():
    import xfgstark
    src = open(os.path.join(ROOT, "include", "xfg_stark.h")).read()
    assert re.search(r"XFG_INVALID_TRACE\s*=\s*11\b", src)
    assert re.search(r"#define\s+XFG_TRACE_VALIDATE\s+1u", src) and re.search(r"#define\s+XFG_TRACE_ON_DEVICE\s+2u", src)
    assert "xfg_trace_fault" in src
    syms = xfgstark.exported_symbols()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in syms, name
    assert xfgstark.STATUS[11] == "INVALID_TRACE"
    for name in ("prove_traces", "submit_traces", "check_traces"):
        assert callable(getattr(xfgstark.XfgBurnMintProver, name))


def test_trace_fault_text():
    import xfgstark
    a = xfgstark.TraceFault(1, 7, 4, 63, 3, 2)
    assert str(a) == "trace does not satisfy assertion main_trace(4, 63) == 3"
    b = xfgstark.TraceFault(2, 5, 0, 17, 0, 0)
    assert str(b) == "main transition constraint 5 did not evaluate to ZERO at step 17"
    assert a == xfgstark.TraceFault(*a.astuple()) and a != b
    assert np.uint64(3) == a.expected
