"""GPU: the OOD frame and the DEEP quotient kernels alone (ood_kernel, ood_final_kernel, deep_coin_block,
deep_carry_kernel, deep_final_kernel through xfg_debug_ood_deep_e), in the base field and in the quadratic
extension, against the plain references of tests/ood_deep_ref.py. Every comparison is exact: the whole
frame, every word of the DEEP polynomial, every DEEP parameter, the coin afterwards and the fail words.

Two launch geometries: without transcript step the frame is reduced by a 64-thread block; with it (the
prover's launches) by a 128-thread block that then draws the DEEP coefficients. A case's coefficients are
the ones its coin draws from the reference frame, so both geometries are held to one reference, computed
once per shape and shared.

Reference time per shape on the CPU (Python integers, inputs and coin model included), at most: dense
3 x 4096 0.5 s, 2^14 0.7 s, 2^16 2.2 s; sparse (2, 2^17) 0.4 s, (1, 2^18) 0.3 s, (1, 2^21) 1.9 s,
(2, 2^20) 3.1 s."""
import functools
import random
import types

import numpy as np
import pytest

import ood_deep_ref as D
import plain_ref as R

pytestmark = pytest.mark.gpu
P = R.P
INVALID = 9  # XFG_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def prover():
    import xfgstark
    pr = xfgstark.XfgBurnMintProver()
    yield pr
    pr.close()


def u64(x):
    return np.array(x, dtype=np.uint64)


def words(v, ext):
    return list(v[:ext])


def pack(ext, co, h, zpts):
    """instances (co [7][n] ints, h [n] E, (z, zg)) -> the entry's arrays coef [B,7,n], hcoef [B,ext,n], zpts [B,2,ext]"""
    return (u64(co), u64([D.planes(hb, ext) for hb in h]), u64([[words(z, ext), words(zg, ext)] for z, zg in zpts]))


def coeff_words(models, ext):
    return u64([[words(v, ext) for v in m["a"] + [m["gamma"]]] for m in models])


def check_coin_outputs(got_dp, got_after, got_fail, models, which=None):
    for b in (range(len(models)) if which is None else which):
        m = models[b]
        assert got_dp[b].tolist() == D.dp_words(m), f"DEEP parameters of instance {b}"
        assert got_after[b] == (m["seed"], m["counter"]), f"coin of instance {b} after the step"
        assert got_fail[b] == m["fail"], f"fail word of instance {b}"


# ---- dense shapes
# n: 8 is one thread (no wave reduction, the 15 D > T store loop), 16 and 32 two and four; 256 and 512 half
# a wave and a wave; 1024 two waves through LDS; 2048 the largest single block; 4096 two blocks; 2^14
# eight; 2^16 32 blocks, more than the 8 S partials a thread of the frame's block loads in one trip for
# every geometry but the base field's without the transcript step (S = 4: test_long_*)
DENSE = [8, 16, 32, 256, 512, 1024, 2048, 4096, 1 << 14, 1 << 16]


def dense_count(n):
    return 3 if n <= 4096 else 1


@functools.lru_cache(maxsize=None)
def dense_case(ext, n):
    """inputs, coins, and the model of every output; built once, read by several tests, never changed"""
    rng = random.Random(f"dense-{ext}-{n}")
    B = dense_count(n)
    g = D.domain_generator(n)
    co = [[[rng.randrange(P) for _ in range(n)] for _ in range(7)] for _ in range(B)]
    h = [[D.rand_e(rng, ext) for _ in range(n)] for _ in range(B)]
    zs = [D.rand_e(rng, ext) for _ in range(B)]
    zpts = [(z, R.e_scale(z, g)) for z in zs]
    coins = [(bytes(rng.randrange(256) for _ in range(32)), (0, 3, 0)[b]) for b in range(B)]
    ginv = pow(g, -1, P)
    models, frames, deep = [], [], []
    for b in range(B):
        frame = D.frame_dense(co[b], h[b], *zpts[b])
        m = D.coin_step_model(coins[b][0], frame, *zpts[b], ginv, ext)
        assert m["fail"] == 0
        _, d = D.deep_dense(co[b], h[b], *zpts[b], m["a"], m["gamma"], frame)
        models.append(m)
        frames.append([words(v, ext) for v in frame])
        deep.append(D.planes(d, ext))
    return types.SimpleNamespace(B=B, ginv=ginv, coins=coins, models=models, args=pack(ext, co, h, zpts),
                                 coeffs=coeff_words(models, ext), frames=u64(frames), deep=u64(deep))


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", DENSE)
def test_dense_matches_reference(prover, n, ext):
    c = dense_case(ext, n)
    ood, deep = prover.debug_ood_deep_e(*c.args, coeffs=c.coeffs)
    assert np.array_equal(ood, c.frames)
    assert np.array_equal(deep, c.deep)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", DENSE)
def test_dense_with_coin_step_matches_reference(prover, n, ext):
    """the prover's launches: distinct seeds, counters 0 and 3 (a reseed resets them), every DeepParams field
    (under ext = 1 the second words are zero), the coin afterwards, fail = 0"""
    c = dense_case(ext, n)
    ood, deep, dp, after, fail = prover.debug_ood_deep_e(*c.args, coins=c.coins, ginv=c.ginv)
    assert np.array_equal(ood, c.frames)
    check_coin_outputs(dp, after, fail, c.models)
    assert fail == [0] * c.B
    if ext == 1:
        assert not dp[:, :, 1].any()
    assert np.array_equal(deep, c.deep)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", [8, 4096])
def test_coin_step_with_z_zero_in_the_middle(prover, n, ext):
    """z = 0 cannot come out of a transcript: that instance fails with 1 / z = 0 (its DEEP polynomial is
    not defined and not looked at), and its neighbours are untouched by it"""
    c = dense_case(ext, n)
    coef, hcoef, zp = (a.copy() for a in c.args)
    zp[1] = 0
    ood, deep, dp, after, fail = prover.debug_ood_deep_e(coef, hcoef, zp, coins=c.coins, ginv=c.ginv)
    assert fail == [0, 1, 0]
    assert dp[1][8:12].tolist() == [[0, 0]] * 4  # z, zg, 1 / z, 1 / zg
    check_coin_outputs(dp, after, fail, c.models, which=(0, 2))
    for b in (0, 2):
        assert np.array_equal(ood[b], c.frames[b])
        assert np.array_equal(deep[b], c.deep[b])
    # the failed instance's frame at z = 0 is the constant terms, and its draws follow from that frame
    frame = [(int(coef[1][k][0]), 0) for k in range(7) for _ in range(2)]
    frame.append(tuple(int(hcoef[1][k][0]) for k in range(ext)) + (0,) * (2 - ext))
    assert ood[1].tolist() == [words(v, ext) for v in frame]
    m = D.coin_step_model(c.coins[1][0], frame, D.ZERO, D.ZERO, c.ginv, ext)
    assert m["fail"] == 1 and m["zinv"] == D.ZERO
    check_coin_outputs(dp, after, fail, {1: m}, which=(1,))


# ---- long polynomials, sparse
@functools.lru_cache(maxsize=None)
def sparse_case(ext, n):
    rng = random.Random(f"sparse-{ext}-{n}")
    g = D.domain_generator(n)
    co, h = D.sparse_polys(n, ext, rng)
    z = D.rand_e(rng, ext)
    zg = R.e_scale(z, g)
    coin = (bytes(rng.randrange(256) for _ in range(32)), 3)
    ginv = pow(g, -1, P)
    frame = D.frame_sparse(co, h, z, zg)
    m = D.coin_step_model(coin[0], frame, z, zg, ginv, ext)
    assert m["fail"] == 0
    _, d = D.deep_sparse(n, co, h, z, zg, m["a"], m["gamma"], ext, frame)
    coef = np.zeros((1, 7, n), dtype=np.uint64)
    hcoef = np.zeros((1, ext, n), dtype=np.uint64)
    for k in range(7):
        coef[0, k, list(co[k])] = u64(list(co[k].values()))
    for k in range(ext):
        hcoef[0, k, list(h)] = u64([v[k] for v in h.values()])
    zp = u64([[words(z, ext), words(zg, ext)]])
    return types.SimpleNamespace(B=1, ginv=ginv, coins=[coin], models=[m], args=(coef, hcoef, zp),
                                 coeffs=coeff_words([m], ext), frames=u64([[words(v, ext) for v in frame]]),
                                 deep=u64([d]))


# (ext, n): 64 blocks, the second trip of the frame's block at S = 4; 128 blocks, the second trip at S = 8;
# 1024 blocks, a full deep_carry block; 512 blocks, a long carry chain in E
@pytest.mark.parametrize("ext,n", [(2, 1 << 17), (1, 1 << 18), (1, 1 << 21), (2, 1 << 20)])
def test_long_with_coin_step_matches_reference(prover, ext, n):
    c = sparse_case(ext, n)
    ood, deep, dp, after, fail = prover.debug_ood_deep_e(*c.args, coins=c.coins, ginv=c.ginv)
    assert np.array_equal(ood, c.frames)
    check_coin_outputs(dp, after, fail, c.models)
    assert np.array_equal(deep, c.deep)


def test_long_without_coin_step_matches_reference(prover):
    """base field, 64 threads: S = 4, whose second trip needs the 64 blocks of n = 2^17"""
    c = sparse_case(1, 1 << 17)
    ood, deep = prover.debug_ood_deep_e(*c.args, coeffs=c.coeffs)
    assert np.array_equal(ood, c.frames)
    assert np.array_equal(deep, c.deep)


# ---- edge values (without the transcript step: z, zg and the coefficients are the test's)
def _edge_case(kind, ext, n):
    """(co, h, z, zg, a, gamma) of one instance; what `kind` does not name is random"""
    rng = random.Random(f"edge-{kind}-{ext}-{n}")
    g = D.domain_generator(n)
    co = [[rng.randrange(P) for _ in range(n)] for _ in range(7)]
    h = [D.rand_e(rng, ext) for _ in range(n)]
    z = D.rand_e(rng, ext)
    zg = None
    a, gam = [D.rand_e(rng, ext) for _ in range(7)], D.rand_e(rng, ext)
    if kind == "z_one":
        z = (1, 0)
    elif kind == "z_minus_one":
        z = (P - 1, 0)
    elif kind == "z_in_base_field":
        z = (z[0], 0)
    elif kind == "z_imaginary":
        z = (0, z[1])
    elif kind == "zg_equals_z":
        zg = z
    elif kind == "zg_unrelated":
        zg = D.rand_e(rng, ext)
    elif kind == "a_zero_gamma_one":
        a, gam = [D.ZERO] * 7, D.ONE
    elif kind == "gamma_zero":
        gam = D.ZERO
    elif kind == "all_p_minus_1":
        co = [[P - 1] * n for _ in range(7)]
        h = [(P - 1, P - 1 if ext == 2 else 0)] * n
    elif kind == "edge_cells":
        cells = R.EDGE_CELLS
        co = [[cells[(j + 2 * c) % len(cells)] for j in range(n)] for c in range(7)]
        h = [(cells[(j + 5) % len(cells)], cells[(3 * j + 1) % len(cells)] if ext == 2 else 0) for j in range(n)]
    else:
        raise ValueError(kind)
    return co, h, z, R.e_scale(z, g) if zg is None else zg, a, gam


EDGE_KINDS = ["z_one", "z_minus_one", "zg_equals_z", "zg_unrelated", "a_zero_gamma_one", "gamma_zero",
              "all_p_minus_1", "edge_cells"]
EDGES = [(k, e) for e in (1, 2) for k in EDGE_KINDS] + [("z_in_base_field", 2), ("z_imaginary", 2)]


@pytest.mark.parametrize("n", [64, 4096])
@pytest.mark.parametrize("kind,ext", EDGES)
def test_edge_values_match_reference(prover, kind, ext, n):
    co, h, z, zg, a, gam = _edge_case(kind, ext, n)
    frame, d = D.deep_dense(co, h, z, zg, a, gam)
    args = pack(ext, [co], [h], [(z, zg)])
    ood, deep = prover.debug_ood_deep_e(*args, coeffs=u64([[words(v, ext) for v in a + [gam]]]))
    assert ood[0].tolist() == [words(v, ext) for v in frame]
    assert np.array_equal(deep[0], u64(D.planes(d, ext)))


# ---- refusals: XFG_INVALID_ARGUMENT from the host, before anything is sized or launched
def _zeros(B, n, ext):
    """valid all-zero polynomials with z = zg = 1 (numpy leaves the pages of a zero array untouched)"""
    return [np.zeros((B, 7, n), dtype=np.uint64), np.zeros((B, ext, n), dtype=np.uint64),
            np.ones((B, 2, ext), dtype=np.uint64), np.zeros((B, 8, ext), dtype=np.uint64)]


def _refused(prover, coef, hcoef, zp, coeffs=None, **kw):
    import xfgstark
    with pytest.raises(xfgstark.XfgStarkError) as e:
        prover.debug_ood_deep_e(coef, hcoef, zp, coeffs=coeffs, **kw)
    assert e.value.status == INVALID
    assert "xfg_debug_ood_deep" in str(e.value)
    return str(e.value)


COIN = [(bytes(32), 0)]


@pytest.mark.parametrize("B,n,ext", [(1, 64, 3), (1, 12, 1), (1, 4, 2), (1, 1 << 22, 1), (0, 64, 1), (65536, 8, 1)])
@pytest.mark.parametrize("coin", [False, True])
def test_unsupported_shape_is_refused(prover, B, n, ext, coin):
    """n = 2^22 would ask launch_deep for a block of 2048 threads; it is refused on the shape alone, before an
    array is read or a buffer sized (count = 1)"""
    coef, hcoef, zp, co = _zeros(B, n, ext)
    if coin:
        msg = _refused(prover, coef, hcoef, zp, coins=COIN * B, ginv=1)
    else:
        msg = _refused(prover, coef, hcoef, zp, co)
    assert "power of two in [8, 2^21]" in msg


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("where", ["coef", "hcoef", "zpts", "coeffs", "ginv"])
@pytest.mark.parametrize("bad", [P, (1 << 64) - 1])
def test_non_canonical_word_is_refused(prover, where, ext, bad):
    arrs = _zeros(2, 64, ext)
    if where == "ginv":
        msg = _refused(prover, *arrs[:3], coins=COIN * 2, ginv=bad)
    else:
        a = arrs[["coef", "hcoef", "zpts", "coeffs"].index(where)]
        a.reshape(-1)[-1] = bad  # the last word of the last instance
        msg = _refused(prover, *arrs)
        if where != "coeffs":
            assert msg == _refused(prover, *arrs[:3], coins=COIN * 2, ginv=1)
    assert "canonical" in msg


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("which", [0, 1])
def test_zero_point_is_refused_without_coin_step(prover, which, ext):
    arrs = _zeros(2, 64, ext)
    arrs[2][1][which] = 0
    assert "must not be zero" in _refused(prover, *arrs)


def test_base_field_entry_refuses_the_same(prover):
    """xfg_debug_ood_deep is the ext = 1 case without transcript step"""
    import xfgstark
    for n, z, word in [(1 << 22, 1, 0), (64, 0, 0), (64, 1, P)]:
        coef = np.zeros((1, 7, n), dtype=np.uint64)
        if word:
            coef[0, 6, n - 1] = word
        with pytest.raises(xfgstark.XfgStarkError) as e:
            prover.debug_ood_deep(coef, np.zeros((1, n), dtype=np.uint64), u64([[z, 1]]), np.zeros((1, 8), dtype=np.uint64))
        assert e.value.status == INVALID
