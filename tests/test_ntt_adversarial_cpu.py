"""The adversarial NTT generators (tests/ntt_adversarial.py) on the CPU: the numpy field arithmetic
against Python integers, and every pull-back against the boundary values recomputed BY DEFINITION from
the generated input -- naive sums over Python integers, none of the pull-back code. A generator that
misses its target would silently degrade the GPU test to a random one, so every position must match."""
import random

import numpy as np
import pytest

import ntt_adversarial as A
import ntt_shapes
import test_ntt_adversarial_gpu as G
from test_gpu_parity import _EDGE

P = A.P


def test_mulmod_matches_python_integers():
    rng = random.Random(5)
    a = [x for x in _EDGE for _ in _EDGE] + [rng.randrange(1 << 64) for _ in range(10000)]
    b = [y for _ in _EDGE for y in _EDGE] + [rng.randrange(1 << 64) for _ in range(10000)]
    got = A.mulmod(np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)).tolist()
    assert got == [x * y % P for x, y in zip(a, b)]
    ca, cb = [x % P for x in a], [y % P for y in b]
    na, nb = np.array(ca, dtype=np.uint64), np.array(cb, dtype=np.uint64)
    assert A.addmod(na, nb).tolist() == [(x + y) % P for x, y in zip(ca, cb)]
    assert A.submod(na, nb).tolist() == [(x - y) % P for x, y in zip(ca, cb)]
    assert A.pow_table(7, 37).tolist() == [pow(7, i, P) for i in range(37)]
    e = [0, 1, 5, 63, 64, 1000, (1 << 11) - 1]
    assert A.pow_of(A.root(11), np.array(e, dtype=np.uint64), 11).tolist() == [pow(A.root(11), i, P) for i in e]
    w = A.root(3)
    x = [rng.randrange(P) for _ in range(8)]
    want = [sum(x[r] * pow(w, r * q, P) for r in range(8)) % P for q in range(8)]
    assert A.dft_axis0(np.array(x, dtype=np.uint64).reshape(8, 1), w).reshape(8).tolist() == want


def test_target_sets_are_what_they_say():
    rng = np.random.default_rng(3)
    s = A.small((64, 64), rng)
    assert int(s.max()) <= (1 << 32) - 2 and {0, 1, 2, 1 << 31, (1 << 32) - 2} <= set(s.ravel().tolist())
    ng = A.neg((64, 64), rng)
    assert int(ng.min()) >= P - ((1 << 32) - 2) and int(ng.max()) <= P - 1
    assert np.flatnonzero(A.sparse((8, 8), rng, 0)).tolist() == [0]
    assert np.flatnonzero(A.sparse((8, 8), rng, 1)).tolist() == [63]
    for case in (2, 3):
        nz = np.flatnonzero(A.sparse((8, 16), rng, case, 8, 16))
        assert len(nz) == 2 + case % 2 and set(nz.tolist()) <= {0, 1, 8, 15, 64, 127}
    m = A.mixed((128,), rng)
    assert int(m[0::2].max()) <= (1 << 32) - 2 and int(m.max()) < P and int(m[1::2].max()) > 1 << 60
    # cancel: a[2] + a[3] = p + s exactly next to a[0] + a[1] = 0 in some group (radix 16, groups down axis 0)
    c = A.cancel((32, 4), rng, 4, 0).tolist()  # element r of group j at row j + 2 r; a[i] = in[brev(i)]
    hit = [(c[0 + 2 * 0][l], c[0 + 2 * 8][l], c[0 + 2 * 4][l], c[0 + 2 * 12][l]) for l in range(4)]
    hit += [(c[1 + 2 * 0][l], c[1 + 2 * 8][l], c[1 + 2 * 4][l], c[1 + 2 * 12][l]) for l in range(4)]
    assert any(a0 + a1 == 0 and P < a2 + a3 < 1 << 64 for a0, a1, a2, a3 in hit)
    assert all(v < P for row in c for v in row)


# ---------------------------------------------------------------- the boundaries by definition
def _by_definition(geo, boundary, data):
    """boundary values (a list, in the target's layout) of the transform of `data`, Python integers"""
    n, R, Cc, fwd = geo.n, geo.R, geo.Cc, geo.fwd
    c = [int(v) for v in data]
    sgn = 1 if fwd else -1
    wn, wR, wC = A.root(geo.logn), A.root(geo.logr), A.root(geo.logc)
    if boundary == "out":
        if fwd:  # plane of the natural coset u + g t of the whole LDE
            logg = geo.g.bit_length() - 1
            x = 7 * pow(A.root(geo.logN + logg), geo.u + geo.g * geo.t, P) % P
            return [sum(c[j] * pow(x * pow(wn, m, P) % P, j, P) for j in range(n)) % P for m in range(n)]
        o7 = A.inv(7) if geo.off7 else 1
        ninv = A.inv(n)
        return [sum(c[j] * pow(wn, -j * k % n, P) for j in range(n)) * ninv * pow(o7, k, P) % P for k in range(n)]
    if fwd and geo.u:  # the sub-transform reads twisted coefficients
        wfull = A.root(geo.logN + geo.g.bit_length() - 1)
        c = [c[j] * pow(wfull, geo.u * j, P) % P for j in range(n)]
    wN = A.root(geo.logN)
    o = geo.o if fwd else 1
    seed = [pow(7, j2, P) * pow(wN, j2 * geo.t, P) % P for j2 in range(Cc)] if fwd else [1] * Cc

    def first_in_a(j1, j2):  # what the first step of pass A loads
        if geo.variant == "plain":
            return c[Cc * j1 + j2] * pow(o, j1, P) % P
        G = R >> geo.first_a
        f = pow(o, j1 - j1 % G, P) * (seed[j2] if geo.variant == "r1024" else 1)
        return c[Cc * j1 + j2] * f % P

    def first_step(vals, logr1):  # vals [S] -> Z at j R1 + q
        S, R1 = len(vals), 1 << logr1
        G, w = S // R1, A.root(logr1) if logr1 else 1
        z = [0] * S
        for j in range(G):
            for q in range(R1):
                z[j * R1 + q] = sum(vals[j + r * G] * pow(w, sgn * r * q % R1, P) for r in range(R1)) % P
        return z

    if boundary == "in_a":
        return [[first_in_a(j1, j2) for j2 in range(Cc)] for j1 in range(R)]
    if boundary == "step_a":
        cols = [first_step([first_in_a(j1, j2) for j1 in range(R)], geo.first_a) for j2 in range(Cc)]
        return [[cols[j2][i] for j2 in range(Cc)] for i in range(R)]
    X = [[sum(c[Cc * j1 + j2] * pow(o, j1, P) * pow(wR, sgn * j1 * k1 % R, P) for j1 in range(R)) % P
          for j2 in range(Cc)] for k1 in range(R)]
    if boundary == "pass":
        return [[X[k1][j2] * (seed[j2] if geo.variant == "r1024" else 1) % P for j2 in range(Cc)] for k1 in range(R)]
    if fwd:
        y = [[X[k1][j2] * pow(7, j2, P) * pow(wN, j2 * (geo.t + (k1 << geo.logbeta)), P) % P for j2 in range(Cc)]
             for k1 in range(R)]
    else:
        ninv = A.inv(n)
        y = [[X[k1][j2] * pow(wn, -j2 * k1 % n, P) * ninv % P for j2 in range(Cc)] for k1 in range(R)]
    if boundary == "in_b":
        return y
    assert boundary == "step_b" and wC
    return [first_step(row, geo.first_b) for row in y]


def _geo(direction, logn, logbeta, t, **kw):
    logr, logc = kw.pop("split", None) or ntt_shapes.ntt_split(logn)
    ea, eb = ntt_shapes.pass_loge(logn)
    kw.setdefault("first_a", ntt_shapes.step_plan(logr, ea)[1])
    kw.setdefault("first_b", ntt_shapes.step_plan(logc, eb)[1])
    return A.Geometry(direction, logn, logr, logc, logbeta, t, **kw)


# the planner's own geometry at sizes <= 2^10 (even and odd splits, blowup 2 and 16), then geometries no
# small size has, forced: first radix 4, 8, 16 and 32 in either pass, the models of ntt_pass_a_cos2 and
# ntt_pass_a_r1024, and sub-transforms of the composed blowups 32 and 128
GEOMETRIES = (
    [("fwd", logn, lb, t, {}) for logn in (3, 4, 5, 8, 9, 10) for lb, t in ((1, 0), (1, 1), (4, 1), (4, 15))] +
    [("inv", logn, 0, 0, dict(off7=o7)) for logn, o7 in ((3, False), (4, True), (5, False), (8, True), (9, True), (10, False))] +
    [("fwd", 8, 2, 3, dict(split=(5, 3), first_a=4, first_b=3, variant="cos2")),
     ("fwd", 8, 4, 9, dict(split=(4, 4), first_a=2, first_b=2, variant="cos2")),
     ("fwd", 9, 3, 5, dict(split=(6, 3), first_a=5, first_b=1, variant="r1024")),
     ("fwd", 7, 4, 15, dict(split=(5, 2), first_a=5, first_b=2, variant="r1024")),
     ("fwd", 9, 1, 1, dict(split=(4, 5), first_a=3, first_b=5)),
     ("fwd", 9, 2, 2, dict(split=(4, 5), first_a=4, first_b=4)),
     ("inv", 9, 0, 0, dict(split=(4, 5), first_a=3, first_b=4, off7=True)),
     ("inv", 9, 0, 0, dict(split=(5, 4), first_a=5, first_b=3)),
     ("fwd", 6, 4, 3, dict(u=1, g=2)), ("fwd", 6, 4, 15, dict(u=5, g=8)), ("fwd", 8, 4, 0, dict(u=3, g=4))])


@pytest.mark.parametrize("direction,logn,logbeta,t,kw", GEOMETRIES,
                         ids=[f"{d}-{n}-{b}-{t}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for d, n, b, t, kw in GEOMETRIES])
def test_generated_inputs_hit_their_targets(direction, logn, logbeta, t, kw):
    geo = _geo(direction, logn, logbeta, t, **dict(kw))
    rng = np.random.default_rng(logn * 100 + logbeta * 10 + t)
    for bi, boundary in enumerate(A.BOUNDARIES):
        if boundary == "out" and logn > 8:
            # the definition of the whole transform is O(n^2): `out` is checked by definition up to 2^8 here.
            # At every size the GPU test asserts that the oracle's transform of the generated input equals the
            # target at every position of the plane before it compares the kernel's output
            continue
        names = [A.TARGET_SETS[(bi + logn + t) % 4], "SPARSE"] + (["CANCEL"] if boundary.startswith("in_") else [])
        for name in names:
            target = A.make_target(name, geo, boundary, rng)
            data = A.pull_back(geo, boundary, target)
            assert data.shape == (geo.n,) and data.dtype == np.uint64 and int(data.max()) < P
            got = np.array(_by_definition(geo, boundary, data), dtype=np.uint64)
            bad = np.flatnonzero(got.ravel() != target.ravel())
            assert bad.size == 0, (boundary, name, f"{bad.size} of {target.size} positions miss, first {int(bad[0])}")


def test_python_geometry_is_the_planners():
    """ntt_shapes restates the split, the radix choice and Plan<> of the C++; the kernel names the planner
    prints (tests/test_ntt_plan.py) carry the same numbers -- here only the arithmetic of the restatement"""
    assert [ntt_shapes.ntt_split(k) for k in (3, 16, 17, 18, 19, 20, 21, 22)] == [
        (1, 2), (8, 8), (8, 9), (8, 10), (9, 10), (10, 10), (10, 11), (10, 12)]
    assert ntt_shapes.step_plan(4, 4) == (1, 4) and ntt_shapes.step_plan(5, 4) == (2, 1)
    assert ntt_shapes.step_plan(10, 5) == (2, 5) and ntt_shapes.step_plan(9, 5) == (2, 4)
    assert ntt_shapes.step_plan(11, 4) == (3, 3) and ntt_shapes.step_plan(12, 4) == (3, 4)
    assert ntt_shapes.pass_a_variant("fwd", 16, 2, 32) == "cos2" and ntt_shapes.pass_a_variant("fwd", 16, 1, 32) == "plain"
    assert ntt_shapes.pass_a_variant("fwd", 16, 2, 28) == "plain" and ntt_shapes.pass_a_variant("fwd", 20, 3, 1) == "r1024"
    assert ntt_shapes.pass_a_variant("fwd", 20, 2, 1) == "plain" and ntt_shapes.pass_a_variant("inv", 16, 0, 32) == "plain"


def test_every_gpu_case_runs_the_sparse_family():
    """each (shape, boundary) of the GPU file runs a SPARSE target with two or three non-zeros; those with more
    than one SPARSE target (launches, or adversarial polynomials) also the single non-zero at position 0 and at
    the last position; every case puts a target on coset 0 and on another one (forward), and the inverse
    `out` cases run without the 7^-k multiply"""
    for shape, boundary in G.CASES:
        plan = [entry for launch in G._launches(shape, boundary) for entry in launch]
        sc = [c for name, c, _ in plan if name == "SPARSE"]
        assert any(c in (2, 3) for c in sc), (shape, boundary)
        assert len(sc) == 1 or {0, 1} <= set(sc), (shape, boundary)
        if shape[0] == "inv" and boundary == "out":
            assert plan[0][2] is False and plan[0][0] == "SMALL", (shape, boundary)
        if shape[0] == "fwd" and len(plan) > 1:
            assert len({v for _, _, v in plan}) > 1, (shape, boundary)
