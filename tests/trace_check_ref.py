"""Reference for the on-device Trace::validate (xfg_check_traces, XFG_TRACE_VALIDATE).

TEST INFRASTRUCTURE ONLY. Winterfell's reporting order restated over plain_ref.transition /
plain_ref.assertions in Python integers: the assertions first, in the order of the AIR, then the steps
0 .. n-2 (the last step has no transition: Winterfell's one exemption), constraints 0..6 at each.
Nothing here shares code with the library.

first_fault(trace, air) -> None for a valid trace, else the fields of xfg_trace_fault:
(kind, index, column, step, expected, found) with kind 1 = assertion, 2 = transition (column, expected
and found are 0 for a transition).

planted_cases(n) -> the traces with planted faults that the CPU and the GPU tests share, each with the
classification the issue states for it where one can be stated without running the reference.
"""
import numpy as np

import oracle_lib as O
import plain_ref as R
import synthetic

P = R.P
ASSERTION, TRANSITION, NONCANONICAL = 1, 2, 3


def first_fault(trace, air):
    cols = [[int(v) for v in col] for col in trace]
    n = len(cols[0])
    for i, (col, step, val) in enumerate(R.assertions(air, n)):
        if cols[col][step] != val:
            return (ASSERTION, i, col, step, val, cols[col][step])
    for s in range(n - 1):
        r = R.transition(air, [cols[c][s] for c in range(7)], [cols[c][s + 1] for c in range(7)])
        for k in range(7):
            if r[k]:
                return (TRANSITION, k, 0, s, 0, 0)
    return None


def oracle_air(air):
    """(pub[12], nullifier, commitment) -> the oracle's Air struct"""
    oa = O.Air()
    for i in range(12):
        oa.pub[i] = air[0][i]
    oa.secret = 0
    oa.nullifier = air[1]
    oa.commitment = air[2]
    return oa


def valid_trace(n, idx):
    """the oracle's build_trace for synthetic burn input `idx`: (trace [7][n] uint64, air tuple)"""
    kw = synthetic.burn_inputs(idx)
    st, oa = O.air_from_inputs(kw["burn_amount"], kw["mint_amount"], kw["tx_prefix_hash"], kw["recipient_address"],
                               kw["secret"], kw["network_id"], kw["target_chain_id"], kw["commitment_version"])
    assert st == 0
    tr = np.frombuffer(O.build_trace(oa, n), dtype=np.uint64).reshape(7, n).copy()
    return tr, (list(oa.pub), int(oa.nullifier), int(oa.commitment))


def _other(v):
    """another canonical value, at a distance from v that is neither 0 nor 1 either way"""
    return (int(v) + 5) % P


def planted_cases(n):
    """[(name, trace [7][n] uint64, air, stated)]: stated = the expected first_fault tuple, None for
    "valid", or the string "ref" where only the reference can say (n = 8, where the last quarter of
    column 4 is two rows long)"""
    base, air = valid_trace(n, 3)
    v0 = [air[0][0], air[0][1], air[0][2], air[0][3], 0, air[1], air[2]]
    cases = []

    def plant(name, cells, stated, air_=air, tr=None):
        t = (base if tr is None else tr).copy()
        for c, s, v in cells:
            t[c][s] = v
        cases.append((name, t, air_, stated))

    plant("valid", [], None)
    # the 8 assertions; a step-0 cell of columns 0..3, 5, 6 also breaks that column's transition
    # constraint at step 0, and the assertion is reported (assertions come first)
    for c in range(7):
        plant(f"assert{c}", [(c, 0, _other(v0[c]))], (ASSERTION, c, c, 0, v0[c], _other(v0[c])))
    plant("assert7", [(4, n - 1, 9)], (ASSERTION, 7, 4, n - 1, 3, 9))
    # each constraint alone at step 0: constraints 0..3 through AIR constants that the (constant)
    # column repeats, so that the assertion holds and the constraint fails; constraint 4 through the
    # cell of step 1; constraints 5 and 6 compare with the asserted constant itself, so at step 0 they
    # cannot fail without their assertion (the cases assert5 / assert6 above)
    for k, val in ((0, 12345), (1, air[0][0] + 1), (2, (1 << 32) + 77), (3, (1 << 33) + 1)):
        pub = list(air[0])
        pub[k] = val
        t = base.copy()
        t[k][:] = val
        plant(f"c{k}@0", [], (TRANSITION, k, 0, 0, 0, 0), air_=(pub, air[1], air[2]), tr=t)
    plant("c4@0", [(4, 1, 5)], (TRANSITION, 4, 0, 0, 0, 0))
    # each constraint at step n - 2 and, for two blocks of 256 steps, on both sides of the block edge
    # (the thread of step 255 reads cell [4][256] of the next block)
    for s in [n - 2] + ([255, 256] if n == 512 else []):
        for k in (0, 1, 2, 3, 5, 6):  # a column-0 cell also breaks constraint 1: constraint 0 is reported
            plant(f"c{k}@{s}", [(k, s, _other(base[k][s]))], (TRANSITION, k, 0, s, 0, 0))
        if s == n - 2:  # cell [4][n-1] is asserted: [4][n-2] = 4 steps up by 1 from 3 and down to 3
            plant(f"c4@{s}", [(4, s, 4)], (TRANSITION, 4, 0, s, 0, 0) if n >= 16 else "ref")
        else:
            plant(f"c4@{s}", [(4, s + 1, int(base[4][s]) + 5)], (TRANSITION, 4, 0, s, 0, 0))
    # the exemption: nothing reads column 0 of the last row
    plant("exempt", [(0, n - 1, _other(base[0][n - 1]))], None)
    # a column-4 cell that differs from both neighbours: the step before it reports
    s = n // 2 + 1
    plant("c4both", [(4, s, int(base[4][s]) + 5)], (TRANSITION, 4, 0, s - 1, 0, 0))
    # two faults: the earlier in the reporting order wins, whichever thread finds it
    plant("two_assert_first", [(5, 3, _other(base[5][3])), (2, 0, _other(v0[2]))],
          (ASSERTION, 2, 2, 0, v0[2], _other(v0[2])))
    if n == 512:
        plant("two_steps", [(6, 300, _other(base[6][300])), (1, 7, _other(base[1][7]))], (TRANSITION, 1, 0, 7, 0, 0))
    return cases


def random_cases(n, seeds):
    """plain_ref.make_trace("random") traces (faults everywhere): [(trace [7][n] uint64, air)]"""
    out = []
    for seed in seeds:
        tr, air = R.make_trace("random", n, seed)
        out.append((np.array(tr, dtype=np.uint64), air))
    return out
