"""The paired sweep's hand-down (csrc/sweep_pair.hip, PW_PUT / PW_GET): a GP with the
training inputs and kernel of the GP in front of it -- the constraints of a SafeOpt problem
-- receives that GP's covariances k(X, x) by LDS-DMA instead of evaluating them again, and
takes alpha . k from the leader's stages.  Every GP is still multiplied by its own L^-1.

The reference for "same bits" is the same build with the feature switched off
(``set_sweep("pair-nohand")`` = ``sgp_ctx_set_sweep(2 | 64)``): the covariances handed down
are the values the twin's own evaluation produces, and its alpha . k is summed in the
order of its own stages, so nothing may differ.  The oracle only bounds both."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _gpu_common import mods, smooth, kernels, check_posterior  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS_WHOLE_AND_CUT = 130 * 130     # 265 tiles on 256 workgroups: whole tiles AND cut remainder tiles
ROWS_TWO_ROUNDS = 200 * 200        # 625 tiles: every workgroup runs TWO whole tiles (the images, the
                                   # parked means and the prefetched rows of a tile are used again
                                   # for the next one), then 113 cut remainder tiles


def _twins(gpy, X, kern_of, noises, seed):
    """GPs on the same inputs with the same kernel: different targets, different noise."""
    return [gpy.models.GPRegression(X, smooth(X, seed + i) + 0.3 + 0.1 * i, kern_of(), noise_var=nv)
            for i, nv in enumerate(noises)]


def _sweep(gps, pts, which, handed=None):
    """One confidence sweep of the paired kernel -> (max l0, Q, S, mean, var).  handed: whether
    the launch must have formed hand-down groups (Context.last_sweep_handed)."""
    from safeopt_amd import _hip
    ctx = gps[0]._fitted().ctx
    G = len(gps)
    old = ctx.set_sweep(which)
    try:
        grid = _hip.DeviceGrid(ctx, pts, G)
        ml = grid.confidence([g._fitted() for g in gps], 2.0, np.full(G, 0.1))
        assert ctx.last_sweep() == "pair"
        if handed is not None:
            assert ctx.last_sweep_handed() == handed
        return (ml, grid.download(_hip.Q), grid.download(_hip.S), grid.download(_hip.MEAN),
                grid.download(_hip.VAR))
    finally:
        ctx.set_sweep(old)


def _same_bits(gps, pts, handed):
    """handed: does the launch qualify?  (With the switch set it never hands down.)"""
    a, b = _sweep(gps, pts, "pair", handed), _sweep(gps, pts, "pair-nohand", False)
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert_array_equal(x, y)
    return a


@pytest.mark.parametrize("N", [197, ROWS_WHOLE_AND_CUT])
@pytest.mark.parametrize("kind", ["Matern52", "RBF"])
@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("n", [260, 500])
def test_twins_same_bits(mods, n, d, kind, N):
    """Three twins, smallest shapes: n = 260 (n_pad 272: a narrow last row block of 4 rows,
    merged two-block stages) and n = 500; 197 rows (ragged, a few tiles, all of them cut into
    runs: the plain sequence inside the instance) and 16 900 rows (whole tiles, which hand
    down, and cut remainder tiles in one launch)."""
    _, gpy, _, _ = mods
    rng = np.random.default_rng(1000 * n + 10 * d + N)
    X = rng.uniform(-2, 2, size=(n, d))
    gps = _twins(gpy, X, lambda: kernels(gpy.kern, kind, d), [0.05 ** 2, 0.08 ** 2, 0.02 ** 2], 3)
    pts = rng.uniform(-3, 3, size=(N, d))
    r = _same_bits(gps, pts, True)
    # (different noise: factors of their own -- the variances differ)
    assert not np.array_equal(r[4][0], r[4][1])


@pytest.mark.parametrize("n,d,kind,handed", [(500, 2, "Matern52", True), (260, 4, "RBF", True),
                                             # three row blocks: two stages per GP, the fewest that
                                             # hand down; two row blocks merge into ONE stage -- the
                                             # leader of the next tile would park its means while the
                                             # twin's are still being read: refused (pair_hand_groups)
                                             (40, 2, "Matern52", True), (20, 2, "RBF", False),
                                             (9, 1, "RBF", False)])
def test_twins_same_bits_two_rounds_of_tiles(mods, n, d, kind, handed):
    """40 000 rows: every workgroup takes two whole tiles through the hand-down sequence, one
    behind the other -- a leader overwrites the images its twins read a tile earlier, the
    parked means are used again, the rows of the next tile are prefetched by the last GP that
    evaluates -- also with the shortest stage sequences."""
    _, gpy, _, _ = mods
    rng = np.random.default_rng(7 * n + d)
    X = rng.uniform(-2, 2, size=(n, d))
    gps = _twins(gpy, X, lambda: kernels(gpy.kern, kind, d), [0.05 ** 2, 0.08 ** 2, 0.02 ** 2], 3)
    _same_bits(gps, rng.uniform(-3, 3, size=(ROWS_TWO_ROUNDS, d)), handed)


def _grouping_cases(gpy, rng):
    n, d = 300, 2
    XA = rng.uniform(-2, 2, size=(n, d))
    XB = rng.uniform(-2, 2, size=(n, d))
    ka = lambda: kernels(gpy.kern, "Matern52", d)                                  # noqa: E731
    kb = lambda: gpy.kern.Matern52(d, variance=1.7, lengthscale=[0.9, 1.7], ARD=True)  # noqa: E731
    nz = [0.05 ** 2, 0.08 ** 2, 0.02 ** 2, 0.03 ** 2, 0.06 ** 2]
    X1 = XA.copy()
    X1[7, 1] = np.nextafter(X1[7, 1], 10.0)          # the last bit of one entry
    yield "A A' B B'", _twins(gpy, XA, ka, nz[:2], 1) + _twins(gpy, XA, kb, nz[2:4], 5), d, True
    yield "A B A", (_twins(gpy, XA, ka, nz[:1], 1) + _twins(gpy, XB, ka, nz[1:2], 2) +
                    _twins(gpy, XA, ka, nz[2:3], 3)), d, False
    yield "four twins", _twins(gpy, XA, ka, nz, 1), d, True
    yield "last bit", _twins(gpy, XA, ka, nz[:1], 1) + _twins(gpy, X1, ka, nz[1:2], 2), d, False
    X5 = rng.uniform(-2, 2, size=(n, 5))
    yield "d = 5", _twins(gpy, X5, lambda: kernels(gpy.kern, "RBF", 5), nz[:3], 1), 5, False


@pytest.mark.parametrize("case", range(5))
def test_grouping_same_bits(mods, case):
    """Groups are consecutive, a leader and at most two twins: (A, A', B, B') with B another
    lengthscale on the same inputs; (A, B, A); four twins of one leader (the fourth leads a new
    group); inputs that differ in the last bit of one entry (no twin); d = 5 (plain schedule).
    Whether groups were formed is checked too; two whole tiles per workgroup."""
    _, gpy, _, _ = mods
    rng = np.random.default_rng(77)
    name, gps, d, handed = list(_grouping_cases(gpy, rng))[case]
    pts = rng.uniform(-3, 3, size=(ROWS_TWO_ROUNDS, d))
    _same_bits(gps, pts, handed)


@pytest.mark.parametrize("kind", ["Matern52", "RBF"])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_twins_against_oracle(mods, d, kind):
    """n = 500, 16 900 rows, against the oracle at the tolerance tests/test_gpu_posterior.py uses
    for this kernel (check_posterior: 1e-9 of the prior variance, the mean relative to
    max |mean|, and 1e-5 relative on variances above 1e-6 k(x, x)).  The inputs lie on a box wide
    enough for a lengthscale to hold a few of them, not dozens (d = 1: 200 long, d = 2: 20 x 20):
    500 points on a line 4 long under an RBF kernel leave variances of a few 1e-6 that are the
    difference of two numbers near 1.7, and the relative bound then asks 1e-11 k(x, x) of a
    Cholesky factor -- the oracle's as much as the device's -- that is good for 1e-10."""
    _, gpy, gpn, _ = mods
    n, N, kdiag = 500, ROWS_WHOLE_AND_CUT, 1.7
    wide = {1: 50.0, 2: 5.0, 4: 1.0}[d]
    rng = np.random.default_rng(1000 * n + 10 * d + N)
    X = wide * rng.uniform(-2, 2, size=(n, d))
    noises = [0.05 ** 2, 0.08 ** 2, 0.02 ** 2]
    gps = _twins(gpy, X, lambda: kernels(gpy.kern, kind, d), noises, 3)
    gos = [gpn.GPRegression(X, g.Y, kernels(gpn, kind, d), noise_var=nv) for g, nv in zip(gps, noises)]
    pts = wide * rng.uniform(-3, 3, size=(N, d))
    r = _sweep(gps, pts, "pair", True)
    for i, go in enumerate(gos):
        mo, vo = go.predict_noiseless(pts)
        m, v = r[3][i][:, None], r[4][i][:, None]
        big = vo > 1e-6 * kdiag
        print("GP %d: mean %.2e of max |mean|, variance %.2e of k(x, x), %.2e relative on %d rows" %
              (i, np.max(np.abs(m - mo)) / np.max(np.abs(mo)), np.max(np.abs(v - vo)) / kdiag,
               np.max(np.abs(v[big] - vo[big]) / vo[big]), int(big.sum())))
        check_posterior(m, v, mo, vo, kdiag)


def test_bo_loop_same_choices(mods):
    """Three add_new_data_point + optimize() iterations of a SafeOpt problem with three twins
    (every GP receives the same x: they stay twins), every posterior from a full sweep:
    chosen points and S / M / G equal those of the run with the hand-down switched off."""
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd import _hip
    d, n = 2, 300
    grid = safeopt_amd.linearly_spaced_combinations([(-2., 2.), (-2., 2.)], [96, 64])
    ctx = _hip.Context.default()

    def run(which):
        rng = np.random.default_rng(11)
        X = rng.uniform(-1.5, 1.5, size=(n, d))
        gps = [gpy.models.GPRegression(X, 1.0 + np.exp(-(X ** 2).sum(1, keepdims=True)) * (1 + 0.2 * i),
                                       kernels(gpy.kern, "Matern52", d), noise_var=nv)
               for i, nv in enumerate([0.05 ** 2, 0.08 ** 2, 0.02 ** 2])]
        old = ctx.set_sweep(which)
        try:
            opt = safeopt_amd.SafeOpt(gps, grid, [0.] * 3, threshold=0.2)
            opt._backend.incremental = False
            out = []
            for t in range(4):
                x = opt.optimize()
                assert ctx.last_sweep() == "pair"
                assert ctx.last_sweep_handed() == (which == "pair")
                out.append((x.copy(), opt.S.copy(), opt.M.copy(), opt.G.copy()))
                if t < 3:
                    y = [1.0 + np.exp(-(x ** 2).sum()) * (1 + 0.2 * i) for i in range(3)]
                    opt.add_new_data_point(x, np.array([y]))
            return out
        finally:
            ctx.set_sweep(old)

    a, b = run("pair"), run("pair-nohand")
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            assert_array_equal(x, y)


def test_riders_in_the_launch_keep_the_plain_schedule(mods):
    """The product's default (factors shared): two GPs with the same noise -- the second rides
    with the first -- and a twin with another noise.  A launch with riders hands nothing down;
    the bits are those of the run with the switch set."""
    _, gpy, _, _ = mods
    n, d = 500, 2
    rng = np.random.default_rng(5)
    X = rng.uniform(-2, 2, size=(n, d))
    gps = _twins(gpy, X, lambda: kernels(gpy.kern, "Matern52", d), [0.05 ** 2, 0.05 ** 2, 0.08 ** 2], 3)
    ctx = gps[0]._fitted().ctx
    old = ctx.set_share(True)
    try:
        r = _same_bits(gps, rng.uniform(-3, 3, size=(ROWS_WHOLE_AND_CUT, d)), False)
    finally:
        ctx.set_share(old)
    assert_array_equal(r[4][0], r[4][1])           # (the rider: its leader's variance)
