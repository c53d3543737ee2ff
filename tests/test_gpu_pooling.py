"""GPU tests of ``pool_repeats``: an optimiser whose GPs pool the measurements at a repeated
input (``GPRegression.pool_data`` -- one ``sgp_gp_reweigh`` on the device) against an optimiser
that appends every measurement, driven with the same measurements; taking measurements back;
the likelihood of a pooled handle; ``SafeOptSwarm``.

The problem is the one that motivates pooling: SafeOpt on a 1-d grid under measurement noise
returns the same rows again and again.  200 rows on [-3, 3], RBF(variance 2, lengthscale 1),
noise sd 0.1, f = sin(1.5 x) + 0.3 x + 0.8, fmin = 0, beta = 2, threshold = 0, x0 = 0, noise from
``default_rng(0)``.

Tolerances: 1e-8 on Q and on the likelihood (relative), the project's; sets equal outside the
rows within 1e-8 of the threshold that decides them."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _reweigh_ref as R
from _gpu_common import mods, check_posterior  # noqa: F401

pytestmark = pytest.mark.gpu

Q_TOL = TIE = 1e-8
STEPS = 60
NOISE_SD = 0.1


def f(x):
    x = np.atleast_2d(x)
    return np.sin(1.5 * x[:, :1]) + 0.3 * x[:, :1] + 0.8


def _make(mods, pool, y0, large_grid=False):
    safeopt_amd, gpy, _, _ = mods
    grid = np.linspace(-3, 3, 200)[:, None]
    gp = gpy.models.GPRegression(np.zeros((1, 1)), np.array([[y0]]), gpy.kern.RBF(1, 2.0, 1.0),
                                 noise_var=NOISE_SD ** 2)
    opt = safeopt_amd.SafeOpt(gp, grid, 0.0, beta=2, threshold=0, pool_repeats=pool)
    if large_grid:
        opt._backend.SMALL_STEP_BUDGET = 0       # the posterior then comes from the refreshes
    return opt


def _drive(mods, steps=STEPS, large_grid=False, check=None):
    """Two optimisers, appending and pooling, fed the picks of the appending one."""
    rng = np.random.default_rng(0)
    y0 = float(f([[0.0]])[0, 0] + NOISE_SD * rng.normal())
    plain, pooled = _make(mods, False, y0, large_grid), _make(mods, True, y0, large_grid)
    for step in range(steps):
        x = plain.optimize()
        xp = pooled.optimize()
        if check is not None:
            check(step, plain, pooled, x, xp)
        y = f(x) + NOISE_SD * rng.normal()
        plain.add_new_data_point(x, y)
        pooled.add_new_data_point(x, y)
    return plain, pooled


@pytest.mark.parametrize("path", ["default", "large_grid"])
def test_pooling_equals_not_pooling(mods, path):
    """60 steps: Q within 1e-8, S / M / G equal outside rows within 1e-8 of their threshold, the
    same pick unless the best width leads by less than 1e-8; the pooled GP ends with at most
    0.6 x 60 rows, at most 2 steps are near-ties, no lower bound comes within 1e-8 of fmin; the
    logs are equal."""
    stats = {"ties": 0, "near_fmin": 0, "dq": 0.0}

    def check(step, plain, pooled, x, xp):
        Q, Qp = np.asarray(plain.Q), np.asarray(pooled.Q)
        dq = np.max(np.abs(Q - Qp))
        stats["dq"] = max(stats["dq"], dq)
        assert dq < Q_TOL, (step, dq)
        lo, up = Q[:, 0], Q[:, 1]
        S, M, G = (np.asarray(a, dtype=bool) for a in (plain.S, plain.M, plain.G))
        near_s = np.abs(lo - 0.0) < TIE
        stats["near_fmin"] += int(near_s.sum())
        max_l = np.max(lo[S])
        near_m = near_s | (np.abs(up - max_l) < TIE)
        assert_array_equal(S[~near_s], np.asarray(pooled.S, dtype=bool)[~near_s])
        assert_array_equal(M[~near_m], np.asarray(pooled.M, dtype=bool)[~near_m])
        assert_array_equal(G[~near_m], np.asarray(pooled.G, dtype=bool)[~near_m])
        w = (up - lo) / plain.scaling[0]
        cand = np.flatnonzero(M | G)
        order = cand[np.argsort(-w[cand])]
        lead = w[order[0]] - (w[order[1]] if len(order) > 1 else -np.inf)
        if lead > TIE:
            assert_array_equal(x, xp)
        else:
            stats["ties"] += 1
            ip = int(np.argmin(np.abs(plain.inputs[:, 0] - xp[0])))
            assert w[order[0]] - w[ip] < TIE, (step, w[order[0]], w[ip])

    plain, pooled = _drive(mods, large_grid=(path == "large_grid"), check=check)
    n_pooled = pooled.gp.X.shape[0]
    print("%s: pooled GP %d rows of %d measurements, %d near-tie steps, max |dQ| %.2e"
          % (path, n_pooled, plain.t, stats["ties"], stats["dq"]))
    assert plain.gp.X.shape[0] == STEPS + 1
    assert n_pooled <= 0.6 * STEPS
    assert stats["ties"] <= 2
    assert stats["near_fmin"] == 0
    assert_array_equal(plain.x, pooled.x)
    assert_array_equal(plain.y, pooled.y)
    assert plain.t == pooled.t == STEPS + 1
    assert int(pooled.gp.pooled_counts().sum()) == STEPS + 1
    if path == "large_grid":
        assert pooled.gp._dev.reweighed or pooled.gp._dev.appended


def _twin_from_log(mods, opt):
    """An appending GP fitted to the log as it stands."""
    _, gpy, _, _ = mods
    return gpy.models.GPRegression(opt.x.copy(), opt.y.copy(), gpy.kern.RBF(1, 2.0, 1.0),
                                   noise_var=NOISE_SD ** 2)


def _same_posterior(gp, twin, what):
    rows = np.linspace(-3, 3, 200)[:, None]
    m, v = gp.predict_noiseless(rows)
    mt, vt = twin.predict_noiseless(rows)
    print("%s: mean %.2e  var %.2e  (%d rows for %d)" % (
        what, np.max(np.abs(m - mt)), np.max(np.abs(v - vt)), gp.X.shape[0], twin.X.shape[0]))
    check_posterior(m[:, 0], v[:, 0], mt[:, 0], vt[:, 0], 2.0)


def test_taking_back(mods):
    """``remove_last_data_point`` after a pooled step, ``remove_data_point`` of a pooled and of
    a single measurement: the GP equals a GP fitted to the remaining log.  A planted outlier
    among repeats is the first of ``suspect_data_points``, and removing it restores the GP."""
    plain, pooled = _drive(mods, steps=30)
    counts = pooled.gp.pooled_counts()
    book = pooled._pool
    assert counts.max() >= 3 and (counts == 1).sum() >= 2
    row_many = int(np.argmax(counts))
    # a pooled step, taken back
    x_rep = pooled.gp.X[row_many].copy()
    n, t = pooled.gp.X.shape[0], pooled.t
    pooled.add_new_data_point(x_rep, f(x_rep) + 0.05)
    assert pooled.gp.X.shape[0] == n and pooled.t == t + 1 and pooled.gp._dev.reweighed
    _same_posterior(pooled.gp, _twin_from_log(mods, pooled), "pooled step")
    pooled.remove_last_data_point()
    assert pooled.t == t and pooled.gp.X.shape[0] == n
    assert_array_equal(pooled.x, plain.x)
    _same_posterior(pooled.gp, _twin_from_log(mods, pooled), "taken back")
    # a pooled measurement in the middle of the log
    j = book.members(0, row_many)[1]
    pooled.remove_data_point(j)
    assert pooled.t == t - 1 and pooled.gp.X.shape[0] == n
    assert pooled.gp.pooled_counts()[row_many] == counts[row_many] - 1
    _same_posterior(pooled.gp, _twin_from_log(mods, pooled), "pooled measurement removed")
    # a measurement that has its row to itself (not the first row: x0 anchors the safe set)
    row_one = int(np.flatnonzero(pooled.gp.pooled_counts() == 1)[-1])
    j = book.members(0, row_one)[0]
    pooled.remove_data_point(j)
    assert pooled.t == t - 2 and pooled.gp.X.shape[0] == n - 1 and pooled.gp._dev.removed
    _same_posterior(pooled.gp, _twin_from_log(mods, pooled), "single measurement removed")
    pooled.optimize()                                   # the optimiser goes on
    # one outlier among the repeats of a row
    row_many = int(np.argmax(pooled.gp.pooled_counts()))
    x_rep = pooled.gp.X[row_many].copy()
    before = pooled.gp.predict_noiseless(np.linspace(-3, 3, 200)[:, None])
    pooled.add_new_data_point(x_rep, f(x_rep) + 1.0)    # 10 noise sd off
    planted = pooled.t - 1
    z = pooled.loo_residuals()
    suspects = pooled.suspect_data_points()
    print("planted |z| %.2f, suspects %r" % (abs(z[planted, 0]), suspects))
    assert suspects and suspects[0] == planted
    pooled.remove_data_point(suspects[0])
    after = pooled.gp.predict_noiseless(np.linspace(-3, 3, 200)[:, None])
    check_posterior(after[0][:, 0], after[1][:, 0], before[0][:, 0], before[1][:, 0], 2.0)
    _same_posterior(pooled.gp, _twin_from_log(mods, pooled), "outlier removed")


def test_likelihood_and_fit_of_a_pooled_handle(mods):
    """``log_likelihood()`` and the gradient of ``_evaluate`` of a pooled handle against the
    appending handle on the same measurements (1e-8, relative, every slot) and against central
    differences of the long-double likelihood of all the measurements; ``optimize()`` of both
    ends at the same optimum."""
    _, gpy, _, _ = mods
    from safeopt_amd import hyper
    plain, pooled = _drive(mods, steps=40)
    spec = (("RBF", (0,), 2.0, (1.0,)),)
    X, Y = plain.x.copy(), plain.y[:, 0].copy()
    noise = NOISE_SD ** 2
    got_p, got_u = pooled.gp.log_likelihood(), plain.gp.log_likelihood()
    want = float(R.ScaledGP(spec, X, Y, None, noise=noise).log_likelihood())
    print("log likelihood: pooled %.12g  appended %.12g  long double %.12g" % (got_p, got_u, want))
    assert abs(got_p - got_u) < 1e-8 * abs(got_u)
    assert abs(got_p - want) < 1e-8 * abs(want)
    desc = pooled.gp.kern._desc(1)
    ev_p = pooled.gp._evaluate(desc[2], desc[3], noise)
    ev_u = plain.gp._evaluate(desc[2], desc[3], noise)
    pooled.gp._settle()
    plain.gp._settle()
    assert ev_p[4] == 0 and ev_u[4] == 0
    slots_p = np.r_[ev_p[0], ev_p[1], np.ravel(ev_p[2]), np.ravel(ev_p[3])]
    slots_u = np.r_[ev_u[0], ev_u[1], np.ravel(ev_u[2]), np.ravel(ev_u[3])]
    print("slots pooled   %r\nslots appended %r" % (slots_p, slots_u))
    assert np.all(np.abs(slots_p - slots_u) < 1e-8 * np.abs(slots_u))

    def ll(variance, inv_ls, nv):
        s = (("RBF", (0,), variance, (1.0 / inv_ls,)),)
        return R.ScaledGP(s, X, Y, None, noise=nv).log_likelihood()

    h = R.LD(1e-7)
    fd = [float((ll(2.0, 1.0, noise + float(h)) - ll(2.0, 1.0, noise - float(h))) / (2 * h)),
          float((ll(2.0 + float(h), 1.0, noise) - ll(2.0 - float(h), 1.0, noise)) / (2 * h)),
          float((ll(2.0, 1.0 + float(h), noise) - ll(2.0, 1.0 - float(h), noise)) / (2 * h))]
    print("central differences %r" % (fd,))
    for got, d in zip(slots_p[1:], fd):
        assert abs(got - d) < 1e-6 * max(abs(d), 1.0)

    res_p, res_u = pooled.gp.optimize(), plain.gp.optimize()
    n = len(Y)
    print("optimize: pooled f %.9f (%s)  appended f %.9f (%s)" % (
        res_p.f_opt, res_p.status, res_u.f_opt, res_u.status))
    print("   pooled   variance %.6f lengthscale %.6f noise_var %.6g" % (
        pooled.gp.kern.variance[0], pooled.gp.kern.lengthscale[0], pooled.gp.noise_var))
    print("   appended variance %.6f lengthscale %.6f noise_var %.6g" % (
        plain.gp.kern.variance[0], plain.gp.kern.lengthscale[0], plain.gp.noise_var))
    assert abs(res_p.f_opt - res_u.f_opt) <= 1e-6 * n
    # the pooled optimum is a stationary point of the appending handle's objective, within ten
    # times L-BFGS-B's projected-gradient tolerance (1e-5), as tests/test_gpu_hyper.py asks
    fresh = gpy.models.GPRegression(X, Y[:, None], gpy.kern.RBF(
        1, pooled.gp.kern.variance[0], pooled.gp.kern.lengthscale[0]), noise_var=pooled.gp.noise_var)
    params = hyper.Parameters(fresh.kern, fresh.noise_var, 1)
    f_at, g_at = params.objective(res_p.x_opt, fresh._evaluate)
    print("   appending objective at the pooled optimum: f %.9f  |g|_inf %.3e" % (
        f_at, np.max(np.abs(g_at))))
    assert abs(f_at - res_p.f_opt) <= 1e-8 * max(abs(f_at), 1.0)
    assert np.max(np.abs(g_at)) < 10 * 1e-5


def test_swarm_noise_scale_and_pooling(mods):
    """``SafeOptSwarm``: ``noise_scale=`` reaches the GP, and ``pool_repeats=True`` pools a
    repeated point instead of appending it."""
    safeopt_amd, gpy, _, _ = mods
    x0 = np.zeros((1, 2))

    def make(pool):
        gp = gpy.models.GPRegression(x0, np.array([[1.0]]), gpy.kern.RBF(2, 2.0, 1.0),
                                     noise_var=0.01)
        return safeopt_amd.SafeOptSwarm(gp, 0.0, [(-2., 2.)] * 2, threshold=0.2,
                                        pool_repeats=pool)

    opt = make(False)
    opt.add_new_data_point([0.3, 0.1], 1.1, noise_scale=0.25)
    assert_array_equal(opt.gp.noise_scale, [1.0, 0.25])
    assert_array_equal(opt.gp._fitted().noise_scale(), [1.0, 0.25])
    opt.add_new_data_point([0.3, 0.1], 1.2)
    assert opt.gp.X.shape[0] == 3 and opt.t == 3

    pooled = make(True)
    pooled.add_new_data_point([0.3, 0.1], 1.1, noise_scale=0.25)
    pooled.add_new_data_point([0.3, 0.1], 1.2)
    assert pooled.gp.X.shape[0] == 2 and pooled.t == 3
    assert_array_equal(pooled.gp.pooled_counts(), [1, 2])
    assert pooled.gp.noise_scale[1] == pytest.approx(0.2)
    rows = np.random.default_rng(1).uniform(-2, 2, (50, 2))
    m, v = pooled.gp.predict_noiseless(rows)
    mt, vt = opt.gp.predict_noiseless(rows)
    check_posterior(m[:, 0], v[:, 0], mt[:, 0], vt[:, 0], 2.0)
    x = pooled.optimize()
    assert np.all(np.isfinite(x))
