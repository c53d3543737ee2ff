"""Marginal likelihood, its gradient and ``optimize()`` on the device (needs an MI355X),
through the public handle and the C ABI, against scikit-learn and a NumPy likelihood.

PARITY_TOL: see profiles/hyper/parity.txt -- 100 x the largest
``|device - scikit-learn| / max(1, |scikit-learn|)`` measured over the 384 cases of
``test_value_and_gradient_match_sklearn`` (8.03e-10, at n = 2000), never above the 1e-6 of
the CPU test.
"""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _hyper_numpy as hn

pytestmark = pytest.mark.gpu

PARITY_TOL = 8.1e-8

KINDS = ["RBF", "Matern32", "Matern52"]
SIZES = [1, 7, 16, 17, 48, 129, 500, 2000]


@pytest.fixture(scope="module")
def mods(hip_device):
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, hyper
    return safeopt_amd, gpy, _hip, hyper


def problem(n, d, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X).sum(1) + 0.1 * rng.normal(size=n)
    return X, y[:, None]


def sk_kernel(kind, ls):
    from sklearn.gaussian_process.kernels import RBF, Matern
    ls = np.atleast_1d(ls)
    ls = ls if ls.size > 1 else float(ls[0])
    return RBF(ls) if kind == "RBF" else Matern(ls, nu=1.5 if kind == "Matern32" else 2.5)


def sk_lml(kind, X, y, v, ls, nv):
    """log p and its gradient in the LOG-parameters [v, ls..., nv] from scikit-learn; the
    WhiteKernel holds nv + 1e-8, its derivative is scaled to d/d log nv."""
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import ConstantKernel as C, WhiteKernel
    g = GPR(C(v) * sk_kernel(kind, ls) + WhiteKernel(nv + 1e-8), alpha=0, optimizer=None)
    g.fit(X, y[:, 0])
    ll, gr = g.log_marginal_likelihood(g.kernel_.theta, eval_gradient=True)
    gr = gr.copy()
    gr[-1] *= nv / (nv + 1e-8)
    return ll, gr


def dev_log_gradient(out, v, inv_ls, nv, ard):
    """theta d/dtheta of the device's result in scikit-learn's order."""
    ll, g_noise, g_var, g_ils, info = out
    assert info == 0
    g_ls = -inv_ls[0] * g_ils[0]               # l d/dl = -s d/ds
    g_ls = g_ls if ard else np.array([g_ls.sum()])
    return ll, np.r_[v * g_var[0], g_ls, nv * g_noise]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_value_and_gradient_match_sklearn(mods, n, d):
    _, gpy, _hip, _ = mods
    X, Y = problem(n, d)
    worst = 0.0
    for kind in KINDS:
        for ard in (True, False):
            for noise in (0.05 ** 2, 0.3 ** 2):
                ls = np.linspace(0.8, 1.6, d) if ard else np.array([1.1])
                k = getattr(gpy.kern, kind)(d, 1.7, ls, ARD=ard)
                gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
                desc = k._desc(d)
                out = gp._fitted().lml(desc[2], desc[3], noise)
                ll, gr = dev_log_gradient(out, 1.7, desc[3], noise, ard)
                ll_sk, gr_sk = sk_lml(kind, X, Y, 1.7, ls, noise)
                err = max(abs(ll - ll_sk) / max(1., abs(ll_sk)),
                          np.max(np.abs(gr - gr_sk) / np.maximum(1., np.abs(gr_sk))))
                print("parity n=%d d=%d %s ard=%d noise=%.4g  err=%.3e  (value %.3e)"
                      % (n, d, kind, ard, noise, err,
                         abs(ll - ll_sk) / max(1., abs(ll_sk))))
                worst = max(worst, err)
                assert gp.log_likelihood() == out[0]
    assert worst < PARITY_TOL, worst


def product_problem(gpy, n, seed=5):
    rng = np.random.default_rng(seed + n)
    X = rng.uniform(-2, 2, (n, 3))
    Y = (np.sin(X).sum(1) + 0.1 * rng.normal(size=n))[:, None]
    k = gpy.kern.Matern52(2, 1.3, [0.7, 1.9], ARD=True, active_dims=[0, 1]) * \
        gpy.kern.RBF(1, 0.8, 1.1, active_dims=[2], name="ctx")
    return X, Y, k


def test_numpy_likelihood_is_pinned_to_sklearn(mods):
    """The reference of the product cases, on the single kernels scikit-learn has."""
    _, gpy, _, _ = mods
    X, Y = problem(129, 4)
    for kind in KINDS:
        ls = np.linspace(0.8, 1.6, 4)
        k = getattr(gpy.kern, kind)(4, 1.7, ls, ARD=True)
        desc = k._desc(4)
        out = hn.lml(list(desc[1]), X, Y, desc[2], desc[3], 0.05 ** 2)
        ll, gr = dev_log_gradient(out, 1.7, desc[3], 0.05 ** 2, True)
        ll_sk, gr_sk = sk_lml(kind, X, Y, 1.7, ls, 0.05 ** 2)
        assert abs(ll - ll_sk) / max(1., abs(ll_sk)) < 1e-9
        assert np.max(np.abs(gr - gr_sk) / np.maximum(1., np.abs(gr_sk))) < 1e-8


@pytest.mark.parametrize("n", [7, 48, 129, 500])
def test_product_of_two_parts(mods, n):
    _, gpy, _, _ = mods
    X, Y, k = product_problem(gpy, n)
    # ... and scikit-learn's product of two kernels on the column subsets, for the value
    from sklearn.gaussian_process.kernels import ConstantKernel as C
    K_sk = (C(1.3) * sk_kernel("Matern52", [0.7, 1.9]))(X[:, :2]) * \
           (C(0.8) * sk_kernel("RBF", [1.1]))(X[:, 2:])
    desc = k._desc(3)
    assert_allclose(hn.cov(list(desc[1]), X, desc[2], desc[3])[0], K_sk, rtol=1e-12, atol=1e-14)
    for noise in (0.05 ** 2, 0.3 ** 2):
        gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
        out = gp._fitted().lml(desc[2], desc[3], noise)
        ref = hn.lml(list(desc[1]), X, Y, desc[2], desc[3], noise)
        assert out[4] == 0
        err = abs(out[0] - ref[0]) / max(1., abs(ref[0]))
        # compared in theta d/dtheta like the single kernels
        for got, want, th in ((out[1], ref[1], noise), (out[2], ref[2], desc[2]),
                              (out[3], ref[3], desc[3])):
            got, want = np.asarray(got) * th, np.asarray(want) * th
            err = max(err, np.max(np.abs(got - want) / np.maximum(1., np.abs(want))))
        print("parity product n=%d noise=%.4g err=%.3e" % (n, noise, err))
        assert err < PARITY_TOL
        assert not out[3][0, 2] and not out[3][1, 0] and not out[3][1, 1]   # unused columns


@pytest.mark.parametrize("n", [17, 300, 2000])
def test_trace_identity(mods, n):
    """sum_ij W_ij Ky_ij = y^T alpha - n:  v_p d/dv_p + (noise + 1e-8) d/dnoise =
    (y^T alpha - n) / 2 for every part, y^T alpha from sgp_gp_get_factor."""
    _, gpy, _, _ = mods
    for X, Y, k in (product_problem(gpy, n),
                    problem(n, 2) + (gpy.kern.Matern32(2, 1.7, [0.8, 1.6], ARD=True),)):
        gp = gpy.models.GPRegression(X, Y, k, noise_var=0.05 ** 2)
        desc = k._desc(X.shape[1])
        dev = gp._fitted()
        ll, g_noise, g_var, _, info = dev.lml(desc[2], desc[3], 0.05 ** 2)
        assert info == 0
        _, alpha = dev.factor()
        want = 0.5 * (Y[:, 0] @ alpha - n)
        for p in range(len(desc[2])):
            got = desc[2][p] * g_var[p] + (0.05 ** 2 + 1e-8) * g_noise
            assert abs(got - want) / max(1., abs(want)) < PARITY_TOL, (got, want)


def test_same_theta_same_bits(mods):
    _, gpy, _, _ = mods
    X, Y = problem(500, 4)
    k = gpy.kern.Matern52(4, 1.7, np.linspace(0.8, 1.6, 4), ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=0.01)
    dev = gp._fitted()
    v, s = np.array([1.3]), 1.0 / np.linspace(0.6, 1.9, 4)[None]
    a = dev.lml(v, s, 0.02)
    dev.lml(v * 1.5, s * 0.7, 0.3)                      # something else in between
    b = dev.lml(v, s, 0.02)
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4] == 0
    assert_array_equal(a[2], b[2])
    assert_array_equal(a[3], b[3])
    # the handle's own likelihood after an edit in place (sgp_gp_set_hyper) is that value
    k.variance[0] = 1.3
    k.lengthscale[:] = np.linspace(0.6, 1.9, 4)
    gp.noise_var = 0.02
    serial = gp._fitted().serial
    assert gp.log_likelihood() == a[0] and gp.objective_function() == -a[0]
    assert gp._fitted().serial == serial


@pytest.mark.parametrize("n", [60, 300])
def test_gp_is_fitted_at_theta_after_lml(mods, n):
    _, gpy, _, _ = mods
    X, Y = problem(n + 1, 2)
    Xn = np.random.default_rng(1).uniform(-2, 2, (257, 2))
    k = gpy.kern.Matern52(2, 2.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X[:n], Y[:n], k, noise_var=0.05 ** 2)
    gp.predict_noiseless(Xn)
    # through the handle: write theta, ask for the likelihood (sgp_gp_lml), predict
    k.variance[0] = 1.4
    k.lengthscale[:] = [0.7, 1.8]
    gp.noise_var = 0.02
    dev = gp._fitted()
    version = dev.version
    gp.log_likelihood()
    assert gp._fitted() is dev and dev.version > version and not dev.appended
    fresh = gpy.models.GPRegression(X[:n], Y[:n], gpy.kern.Matern52(2, 1.4, [0.7, 1.8], ARD=True),
                                    noise_var=0.02)
    for a, b in zip(gp.predict_noiseless(Xn), fresh.predict_noiseless(Xn)):
        assert_array_equal(a, b)
    # one row more, one fewer: as a refit
    gp.set_XY(X, Y)
    assert gp._fitted() is dev and dev.appended
    fresh.set_XY(X, Y)
    for a, b in zip(gp.predict_noiseless(Xn), fresh.predict_noiseless(Xn)):
        assert_array_equal(a, b)
    refit = gpy.models.GPRegression(X, Y, gpy.kern.Matern52(2, 1.4, [0.7, 1.8], ARD=True),
                                    noise_var=0.02)
    m, v = refit.predict_noiseless(Xn)
    assert_allclose(gp.predict_noiseless(Xn)[0], m, rtol=0, atol=1e-9 * np.abs(m).max())
    assert_allclose(gp.predict_noiseless(Xn)[1], v, rtol=0, atol=1e-9 * 1.4)
    gp.set_XY(X[:n], Y[:n])
    fresh.set_XY(X[:n], Y[:n])
    for a, b in zip(gp.predict_noiseless(Xn), fresh.predict_noiseless(Xn)):
        assert_array_equal(a, b)


def test_infeasible_theta_is_reported_and_survived(mods):
    _, gpy, _hip, _ = mods
    X, Y = problem(40, 2)
    X = np.vstack([X, X])                       # duplicated inputs
    Y = np.vstack([Y, Y + 0.01])
    k = gpy.kern.RBF(2, 1.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=0.05 ** 2)
    dev = gp._fitted()
    desc = k._desc(2)
    # Ky = K - 0.9e-8 I on duplicated rows: not positive definite
    out = dev.lml(desc[2], desc[3], -1.9e-8)
    assert out[4] != 0
    with pytest.raises(_hip.HipError):          # not fitted: no silent numbers
        dev.predict(X[:3])
    good = dev.lml(desc[2], desc[3], 0.05 ** 2)
    ref = hn.lml(list(desc[1]), X, Y, desc[2], desc[3], 0.05 ** 2)
    assert good[4] == 0 and abs(good[0] - ref[0]) / max(1., abs(ref[0])) < PARITY_TOL
    assert_allclose(good[3], ref[3], rtol=0, atol=PARITY_TOL * max(1., np.abs(ref[3]).max()))
    m, v = dev.predict(X[:3])
    assert np.all(np.isfinite(m)) and np.all(v > 0)
    # through the handle: the objective is +inf there and the model recovers by itself
    p_bad = gp._evaluate(desc[2], desc[3], -1.9e-8)
    assert p_bad[4] != 0
    m2, _ = gp.predict_noiseless(X[:3])
    assert_allclose(m2, m, rtol=0, atol=1e-9)


END_TO_END = [
    # n, d, kind, seed
    # (seeds chosen on the CPU, on the reference optimiser alone: it converges from these
    # starts AND its last step ends below pgtol rather than on the relative reduction of f,
    # which most seeds stop on with a gradient of 1e-4 .. 1e-2 in x)
    (300, 2, "Matern52", 20),
    (500, 4, "RBF", 62),
]


def end_to_end_problem(gpy, n, d, kind, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (n, d))
    ls = np.linspace(0.9, 1.5, d)
    kinds = [{"RBF": hn.RBF, "Matern52": hn.MATERN52}[kind]]
    Y = hn.draw_gp(kinds, X, np.array([1.5]), (1.0 / ls)[None], 0.05 ** 2, seed + 100)
    # start at twice / half the truth
    start = np.where(np.arange(d) % 2 == 0, 2.0, 0.5) * ls
    make = lambda: getattr(gpy.kern, kind)(d, 3.0, start.copy(), ARD=True)
    return X, Y, make, 2 * 0.05 ** 2


@pytest.mark.parametrize("n, d, kind, seed", END_TO_END)
def test_optimize_reaches_the_reference_optimum(mods, n, d, kind, seed):
    _, gpy, _, hyper = mods
    X, Y, make, noise0 = end_to_end_problem(gpy, n, d, kind, seed)
    k_ref = make()
    p_ref = hyper.Parameters(k_ref, noise0, d)
    ref = hyper.optimize(p_ref, hn.evaluator(k_ref, X, Y))
    assert "CONVERGENCE" in ref.status
    k = make()
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise0)
    f0 = gp.objective_function()
    var_obj = k.variance
    res = gp.optimize()
    print("optimize n=%d d=%d %s: device f=%.9f (%d evals, %s)  reference f=%.9f (%d evals)"
          % (n, d, kind, res.f_opt, res.funct_eval, res.status, ref.f_opt, ref.funct_eval))
    assert res.f_opt < f0 and k.variance is var_obj
    assert abs(res.f_opt - ref.f_opt) <= 1e-6 * n
    # projected gradient (no bounds: the gradient) in x at the device's optimum, by scikit-learn
    ls = k.lengthscale.copy()
    ll_sk, gr_sk = sk_lml(kind, X, Y, float(k.variance[0]), ls, gp.noise_var)
    theta = np.r_[k.variance, ls, gp.noise_var]
    g_x = -(gr_sk / theta) * hyper.softplus_grad(res.x_opt)
    print("   |g|_inf in x by scikit-learn: %.3e" % np.max(np.abs(g_x)))
    assert np.max(np.abs(g_x)) < 10 * 1e-5
    assert abs(-ll_sk - res.f_opt) <= 1e-6 * n
    # the handle is fitted at the result: no refit, and it predicts like a fresh one
    dev = gp._dev
    version = dev.version
    Xn = np.random.default_rng(2).uniform(-3, 3, (100, d))
    m, v = gp.predict_noiseless(Xn)
    assert gp._dev is dev and dev.version == version
    fresh = gpy.models.GPRegression(X, Y, getattr(gpy.kern, kind)(d, k.variance[0], ls, ARD=True),
                                    noise_var=gp.noise_var)
    mf, vf = fresh.predict_noiseless(Xn)
    assert_array_equal(m, mf)
    assert_array_equal(v, vf)


def test_fixed_and_restarts_on_the_device(mods):
    _, gpy, _, _ = mods
    X, Y, make, noise0 = end_to_end_problem(gpy, 120, 2, "Matern52", 9)
    k = make()
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise0)
    res = gp.optimize(fixed=("noise_var", "variance"))
    assert gp.noise_var == noise0 and k.variance[0] == 3.0 and res.x_opt.size == 2
    out = []
    for rep in range(2):
        kk = make()
        g2 = gpy.models.GPRegression(X, Y, kk, noise_var=noise0)
        np.random.seed(5)
        r = g2.optimize_restarts(num_restarts=3)
        out.append((r.f_opt, kk.lengthscale.copy(), g2.noise_var))
        assert g2.objective_function() == r.f_opt
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    assert_array_equal(out[0][1], out[1][1])


def test_fitted_handle_inside_safeopt(mods):
    safeopt_amd, gpy, _, _ = mods
    X, Y, make, noise0 = end_to_end_problem(gpy, 150, 2, "Matern52", 12)
    Y = Y + 2.0
    k = make()
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise0)
    gp.optimize()
    grid = safeopt_amd.linearly_spaced_combinations([(-3., 3.)] * 2, 60)
    fresh = gpy.models.GPRegression(
        X, Y, gpy.kern.Matern52(2, k.variance[0], k.lengthscale.copy(), ARD=True),
        noise_var=gp.noise_var)
    a = safeopt_amd.SafeOpt(gp, grid, 0., threshold=0.2)
    b = safeopt_amd.SafeOpt(fresh, grid, 0., threshold=0.2)
    for step in range(3):
        xa, xb = a.optimize(), b.optimize()
        assert_array_equal(xa, xb)
        for name in ("Q", "S", "M", "G"):
            assert_array_equal(getattr(a, name), getattr(b, name))
        y = float(np.sin(xa).sum()) + 2.0
        a.add_new_data_point(xa, y)
        b.add_new_data_point(xb, y)
    # refit between campaigns: the optimiser object notices the new hyper-parameters
    gp.optimize()
    fresh2 = gpy.models.GPRegression(
        gp.X, gp.Y, gpy.kern.Matern52(2, k.variance[0], k.lengthscale.copy(), ARD=True),
        noise_var=gp.noise_var)
    b2 = safeopt_amd.SafeOpt(fresh2, grid, 0., threshold=0.2)
    b2.scaling = a.scaling
    b2.S[:] = a.S
    assert_array_equal(a.optimize(), b2.optimize())
    assert_array_equal(a.Q, b2.Q)


def test_edit_in_place_keeps_the_device_gp(mods):
    _, gpy, _, _ = mods
    X, Y = problem(200, 2)
    k = gpy.kern.RBF(2, 2.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=0.05 ** 2)
    dev = gp._fitted()
    serial, version = dev.serial, dev.version
    allocs = gp._ctx.alloc_count() if hasattr(gp._ctx, "alloc_count") else None
    k.lengthscale[0] = 1.7
    gp.noise_var = 0.1 ** 2
    m, v = gp.predict_noiseless(X[:5])
    assert gp._fitted() is dev and dev.serial == serial and dev.version == version + 1
    if allocs is not None:
        assert gp._ctx.alloc_count() == allocs
    fresh = gpy.models.GPRegression(X, Y, gpy.kern.RBF(2, 2.0, [1.7, 1.0], ARD=True),
                                    noise_var=0.1 ** 2)
    mf, vf = fresh.predict_noiseless(X[:5])
    assert_array_equal(m, mf)
    assert_array_equal(v, vf)
