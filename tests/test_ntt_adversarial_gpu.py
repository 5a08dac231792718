"""Every NTT kernel on inputs that put chosen values at its internal boundaries (tests/ntt_adversarial.py),
bit for bit against the oracle.

Random data reaches the non-canonical sliver [p, 2^64) of a weakly reduced value with probability 2^-32,
so bit-exact parity on random inputs (test_gpu_parity.py) is nearly blind to a canonicalisation that is
missing or misplaced. Here the targets -- small values (what add_w returns as p + s), their negatives,
sparse vectors (whose earlier levels cancel to 0 or p), and first-step inputs built to put p + s next to a
tiny minuend -- are pulled back through the transform to its input, for the outputs of the whole transform
(out), of pass A's column DFTs (pass), of the first Stockham step of a multi-step pass (step_a, step_b),
and for the first-step inputs themselves (in_a, in_b). tests/test_ntt_adversarial_cpu.py proves on the CPU
that the generated inputs hit their targets; tests/test_ntt_plan.py that the shapes reach all 48 kernels.

Also the truncated inverse transform of the composition polynomial and the FRI remainder
(xfg_debug_interpolate_keep: keep < n coefficients, `keep` words apart)."""
import numpy as np
import pytest

import ntt_adversarial as A
import ntt_shapes
import oracle_lib as O

pytestmark = pytest.mark.gpu
P = A.P
CASES = ntt_shapes.adversarial_cases()
# What a (shape, boundary) case runs, by the size of one launch. Per boundary kind the target sets, then the
# SPARSE cases (ntt_adversarial.sparse: 0 the single position 0, 1 the single last position, 2 and 3 two and
# three positions with different low, middle and high index digits). Every case runs a multi-position SPARSE
# target; "one" (n >= 2^20, or 2^23 output words) has time for that one alone.
BUDGET = {
    "full": (dict(out=A.TARGET_SETS, pas=A.TARGET_SETS, step=A.TARGET_SETS, inp=("CANCEL", "NEG", "SPARSE")), (2, 3, 0, 1)),
    "two": (dict(out=("SMALL", "SPARSE"), pas=("NEG", "SPARSE"), step=("SMALL", "SPARSE"), inp=("CANCEL", "SPARSE")), (3, 0, 1)),
    "one": (dict(out=("SMALL", "SPARSE"), pas=("SPARSE",), step=("SMALL", "SPARSE"), inp=("CANCEL", "SPARSE")), (2,)),
}
KIND = {"out": "out", "pass": "pas", "step_a": "step", "step_b": "step", "in_a": "inp", "in_b": "inp"}


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def _geometry(shape, t=0, off7=False):
    """the Geometry of natural coset t (forward) of a shape of ntt_shapes; blowups above 16 are composed of
    g = blowup / 16 blowup-16 transforms, coset t being plane t // g of sub-transform t % g (lde_plan)"""
    d, logn, logbeta, npoly, _ = shape
    logr, logc = ntt_shapes.ntt_split(logn)
    ea, eb = ntt_shapes.pass_loge(logn)
    g = 1 << max(logbeta - 4, 0)
    return A.Geometry(d, logn, logr, logc, min(logbeta, 4), t // g, off7, ntt_shapes.step_plan(logr, ea)[1],
                      ntt_shapes.step_plan(logc, eb)[1], ntt_shapes.pass_a_variant(d, logn, min(logbeta, 4), npoly),
                      t % g, g)


def _launches(shape, boundary):
    """the launches of one case: each a list with one (target set, SPARSE case or None, coset or off7) per
    adversarial polynomial (the first, the middle and the last of the launch set).
    One polynomial: a launch per (set, coset) in the "full" budget, else a launch per set with the cosets taken
    in turn; SPARSE always gets a launch per SPARSE case of the budget.
    Three polynomials: a launch per set, the polynomials on different cosets; the one SPARSE launch gives them
    the budget's multi-position case, case 0 and case 1.
    Inverse: the "coset" is off7, the same for the whole launch; off7 = False comes first (only without the
    7^-k multiply does the store's own canonicalisation show)."""
    d, logn, logbeta, npoly, _ = shape
    beta = 1 << logbeta
    nadv = len({0, npoly // 2, npoly - 1})
    cosets = sorted({0, 1, beta - 1} | ({beta // 16 + 1} if logbeta > 4 else set())) if d == "fwd" else [False, True]
    words = npoly << (logn + logbeta)
    budget = "one" if (logn >= 20 or words >= 1 << 23) else "two" if words >= 1 << 18 else "full"
    sets, cases = BUDGET[budget]
    out, turn = [], 0  # turn: which coset the next launch starts with
    for name in sets[KIND[boundary]]:
        if nadv > 1:
            sc = (cases[0], 0, 1) if name == "SPARSE" else (None,) * 3
            out.append([(name, sc[k], cosets[(turn + k) % len(cosets)]) for k in range(nadv)])
            turn += 1
        elif name == "SPARSE":
            for c in cases:
                out.append([(name, c, cosets[turn % len(cosets)])])
                turn += 1
        elif budget == "full":
            out += [[(name, None, v)] for v in cosets]
        else:
            out.append([(name, None, cosets[turn % len(cosets)])])
            turn += 1
    return out


def _first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else (int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), int(bad.size))


@pytest.mark.parametrize("shape,boundary", CASES, ids=[f"{s[0]}-2p{s[1]}x{1 << s[2]}-{s[3]}poly-{b}" for s, b in CASES])
def test_adversarial_inputs_match_oracle(prover, shape, boundary):
    d, logn, logbeta, npoly, _ = shape
    n, beta = 1 << logn, 1 << logbeta
    adv = sorted({0, npoly // 2, npoly - 1})
    rng = np.random.default_rng([logn, logbeta, npoly, A.BOUNDARIES.index(boundary)])
    for launch in _launches(shape, boundary):
        data = rng.integers(0, P, size=(npoly, n), dtype=np.uint64)
        plan = dict(zip(adv, launch))  # polynomial -> (target set, SPARSE case, coset or off7)
        targets = {}
        for p, (name, case, v) in plan.items():
            geo = _geometry(shape, v, False) if d == "fwd" else _geometry(shape, 0, v)
            targets[p] = A.make_target(name, geo, boundary, rng, case=case)
            data[p] = A.pull_back(geo, boundary, targets[p])
        if d == "fwd":
            got = np.asarray(prover.debug_lde(data, n, beta))
            want = [O.evaluate_lde_np(data[p], beta, 7) for p in range(npoly)]
        else:
            assert len(adv) == 1
            off7 = launch[0][2]
            got = np.asarray(prover.debug_interpolate(data, n, off7))
            want = [O.interpolate_np(data[p], 7 if off7 else 1) for p in range(npoly)]
        for p in range(npoly):
            if boundary == "out" and p in targets:  # the oracle agrees that the input hits its target
                plane = want[p][plan[p][2]::beta] if d == "fwd" else want[p]
                assert np.array_equal(plane, targets[p]), (shape, plan[p], p, "the generator missed its target")
            diff = _first_diff(got[p], want[p])
            assert diff is None, (f"shape {shape} boundary {boundary} polynomial {p}"
                                  f" ({'(set, SPARSE case, coset/off7) = ' + str(plan[p]) if p in plan else 'random'}):"
                                  f" first differing index, got, want, differing words = {diff}")


# ---------------------------------------------------------------- the truncated inverse transform
# the smallest size of each inverse ntt_pass_b<2..12> (ntt_shapes.ADVERSARIAL, subject b)
KEEP_SIZES = [s[1] for s in ntt_shapes.ADVERSARIAL if s[0] == "inv" and "b" in s[4]]
GUARD = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.mark.parametrize("logn", KEEP_SIZES)
def test_interpolate_keep_matches_oracle_and_stays_in_bounds(prover, logn):
    """launch_interpolate as the prover calls it (keep < n coefficients per polynomial, stored `keep` words
    apart): polynomial 0 random, polynomial 1 with small coefficients (B_out SMALL); the first `keep` oracle
    coefficients come back and nothing is written behind them (the guard words keep their 0xFF bytes; a
    store at k = keep of the last polynomial would land on the first of them)"""
    n, off7 = 1 << logn, bool(KEEP_SIZES.index(logn) % 2)
    rng = np.random.default_rng(logn)
    ev = rng.integers(0, P, size=(2, n), dtype=np.uint64)
    geo = _geometry(("inv", logn, 0, 1, ""), 0, off7)
    coef1 = A.small((n,), rng)
    ev[1] = A.pull_back(geo, "out", coef1)
    want = np.stack([O.interpolate_np(ev[0], 7 if off7 else 1), coef1])
    for keep in sorted({1, max(1, n // 16), n // 2}):
        got, guard = prover.debug_interpolate_keep(ev, n, keep, off7)
        assert got.shape == (2, keep)
        for p in range(2):
            assert _first_diff(got[p], want[p][:keep]) is None, (logn, keep, off7, p, _first_diff(got[p], want[p][:keep]))
        assert np.all(guard == GUARD), (logn, keep, [hex(int(g)) for g in guard])


def test_interpolate_keep_refuses_bad_arguments(prover):
    import xfgstark
    ev = np.zeros((1, 64), dtype=np.uint64)
    for n, keep in ((64, 0), (64, 65), (64, 1 << 40), (48, 8), (4, 2)):
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.debug_interpolate_keep(ev[:, :n] if n <= 64 else ev, n, keep)
        assert e.value.status == 9, (n, keep)
    got, guard = prover.debug_interpolate_keep(ev, 64, 64)  # keep = n is the whole transform
    assert got.shape == (1, 64) and not got.any() and np.all(guard == GUARD)
