"""Host side of the hyper-parameter fit (no GPU): the parameter class of safeopt_amd.hyper
and the L-BFGS-B drivers, with a NumPy likelihood in place of ``DeviceGP.lml``."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _hyper_numpy as hn


@pytest.fixture(scope="module")
def mods():
    import safeopt_amd.gpy as gpy
    from safeopt_amd import hyper
    from oracle import gp_numpy as gpn
    return gpy, hyper, gpn


def make_kernels(ns):
    return {
        "ard": ns.Matern52(3, 1.7, [0.8, 1.3, 2.1], ARD=True),
        "iso": ns.RBF(3, 0.9, 1.4),
        "prod": ns.Matern32(2, 1.3, [0.7, 1.9], ARD=True, active_dims=[0, 1]) *
                ns.RBF(1, 0.8, 1.1, active_dims=[2], name="ctx"),
    }


@pytest.mark.parametrize("which", ["ard", "iso", "prod"])
def test_pack_unpack_round_trip(mods, which):
    gpy, hyper, _ = mods
    k = make_kernels(gpy.kern)[which]
    p = hyper.Parameters(k, 0.05, 3)
    x = p.get_x()
    want = {"ard": 5, "iso": 3, "prod": 6}[which]
    assert x.size == want == len(p.names)
    before = [(np.array(q.variance), np.array(q.lengthscale)) for q in k._parts()]
    ids = [(id(q.variance), id(q.lengthscale)) for q in k._parts()]
    assert p.set_x(x) == pytest.approx(0.05, rel=1e-14)
    for q, (v, ls), (iv, il) in zip(k._parts(), before, ids):
        assert_allclose(q.variance, v, rtol=1e-14)
        assert_allclose(q.lengthscale, ls, rtol=1e-14)
        assert (id(q.variance), id(q.lengthscale)) == (iv, il)       # written in place
    # the descriptor of the vector is the kernel's own
    variances, inv_ls, noise = p.descriptor(p.theta(x))
    desc = k._desc(3)
    assert_allclose(variances, desc[2], rtol=1e-14)
    assert_allclose(inv_ls, desc[3], rtol=1e-14)
    # a new vector lands in the objects
    p.set_x(x + 0.25)
    assert_allclose(p.get_x(), x + 0.25, rtol=1e-12, atol=1e-12)


def test_softplus_is_gpys_logexp(mods):
    _, hyper, _ = mods
    x = np.array([-30., -2., 0., 3., 40.])
    assert_allclose(hyper.softplus(x), np.logaddexp(0., x), rtol=1e-15)
    assert_allclose(hyper.softplus_inv(hyper.softplus(x)), x, rtol=1e-9)


def test_fixed_names_remove_exactly_their_entries(mods):
    gpy, hyper, _ = mods
    ks = make_kernels(gpy.kern)
    p = hyper.Parameters(ks["ard"], 0.05, 3, fixed=("noise_var",))
    assert p.names == ["Mat52.variance"] + ["Mat52.lengthscale"] * 3
    p = hyper.Parameters(ks["ard"], 0.05, 3, fixed=("lengthscale",))
    assert p.names == ["Mat52.variance", "noise_var"]
    p = hyper.Parameters(ks["iso"], 0.05, 3, fixed="variance")
    assert p.names == ["rbf.lengthscale", "noise_var"]
    p = hyper.Parameters(ks["prod"], 0.05, 3, fixed=("ctx.lengthscale", "Mat32.variance"))
    assert p.names == ["Mat32.lengthscale", "Mat32.lengthscale", "ctx.variance", "noise_var"]
    # a fixed entry keeps its value whatever x says
    p.set_x(p.get_x() + 1.0)
    assert ks["prod"].ctx.lengthscale[0] == 1.1 and ks["prod"].Mat32.variance[0] == 1.3
    with pytest.raises(ValueError):
        hyper.Parameters(ks["prod"], 0.05, 3, fixed=("variance",))
    with pytest.raises(ValueError):
        hyper.Parameters(ks["ard"], 0.05, 3, fixed=("nose_var",))


def test_numpy_likelihood_uses_the_oracles_kernels(mods):
    gpy, hyper, gpn = mods
    rng = np.random.default_rng(3)
    X = rng.uniform(-2, 2, (40, 3))
    for name, k in make_kernels(gpy.kern).items():
        ko = make_kernels(gpn)[name]
        d, kinds, variances, inv_ls = k._desc(3)
        assert_allclose(hn.cov(list(kinds), X, variances, inv_ls)[0], ko.K(X), rtol=1e-12,
                        atol=1e-14)


@pytest.mark.parametrize("n", [50, 500])
@pytest.mark.parametrize("which", ["ard", "iso", "prod", "rbf_ard", "m32_ard"])
def test_chain_rule_by_central_differences(mods, which, n):
    """Gradient in x through the class (softplus, 1/lengthscale, the sum over the columns
    of a non-ARD part, fixed entries dropped) against central differences of the value:
    step 1e-5 in x, agreement 1e-6 relative to max(1, |g|)."""
    gpy, hyper, _ = mods
    ks = make_kernels(gpy.kern)
    ks["rbf_ard"] = gpy.kern.RBF(3, 1.7, [0.8, 1.3, 2.1], ARD=True)
    ks["m32_ard"] = gpy.kern.Matern32(3, 1.7, [0.8, 1.3, 2.1], ARD=True)
    k = ks[which]
    rng = np.random.default_rng(n)
    X = rng.uniform(-2, 2, (n, 3))
    y = np.sin(X).sum(1) + 0.1 * rng.normal(size=n)
    ev = hn.evaluator(k, X, y)
    for fixed in ((), ("noise_var",)):
        p = hyper.Parameters(k, 0.05, 3, fixed)
        x = p.get_x()
        f, g = p.objective(x, ev)
        fd = np.empty_like(x)
        for i in range(x.size):
            h = np.zeros_like(x)
            h[i] = 1e-5
            fd[i] = (p.objective(x + h, ev)[0] - p.objective(x - h, ev)[0]) / 2e-5
        err = np.max(np.abs(g - fd) / np.maximum(1., np.abs(g)))
        print(which, n, fixed, "max rel err", err)
        assert err < 1e-6, (g, fd)


def known_problem(gpy, seed=7, n=120):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (n, 2))
    truth = (np.array([1.5]), np.array([[1 / 0.9, 1 / 1.6]]), 0.05 ** 2)
    Y = hn.draw_gp([hn.MATERN52], X, *truth, seed=seed + 1)
    k = gpy.kern.Matern52(2, 3.0, [0.45, 3.2], ARD=True)
    return X, Y, k


def test_optimize_writes_in_place_and_descends(mods):
    gpy, hyper, _ = mods
    X, Y, k = known_problem(gpy)
    var_obj, ls_obj = k.variance, k.lengthscale
    ev = hn.evaluator(k, X, Y)
    p = hyper.Parameters(k, 0.1 ** 2, 2)
    f0 = p.objective(p.get_x(), ev)[0]
    res = hyper.optimize(p, ev)
    assert res.f_opt < f0 - 1.0
    assert k.variance is var_obj and k.lengthscale is ls_obj
    assert_allclose(hyper.softplus(res.x_opt), np.r_[k.variance, k.lengthscale, p.noise_var],
                    rtol=1e-14)
    assert res.noise_var == p.noise_var and res.funct_eval > 3
    assert "CONVERGENCE" in res.status
    # the fitted values are near the ones the data were drawn with
    assert 0.4 < k.lengthscale[0] < 2.0 and 0.7 < k.lengthscale[1] < 3.5
    assert 0.02 ** 2 < p.noise_var < 0.12 ** 2
    # the objective at the result is what the class evaluates there
    assert res.f_opt == p.objective(p.get_x(), ev)[0]


def test_infeasible_trial_step_does_not_end_the_run(mods):
    gpy, hyper, _ = mods
    X, Y, k = known_problem(gpy)
    k_free = k.copy()
    good = hn.evaluator(k, X, Y)
    calls = []

    def ev(variances, inv_ls, noise_var):
        calls.append(1)
        out = good(variances, inv_ls, noise_var)
        if len(calls) == 3:          # (1: the start check, 2: the start, 3: first trial step)
            return out[:4] + (17,)
        return out

    p = hyper.Parameters(k, 0.1 ** 2, 2)
    f0 = p.objective(p.get_x(), good)[0]
    res = hyper.optimize(p, ev)
    assert len(calls) > 5 and res.f_opt < f0 - 1.0
    ref = hyper.optimize(hyper.Parameters(k_free, 0.1 ** 2, 2), hn.evaluator(k_free, X, Y))
    assert abs(res.f_opt - ref.f_opt) < 1e-6 * len(X)
    # an objective reports +inf with a zero gradient there
    f, g = p.objective(p.get_x(), lambda *a: good(*a)[:4] + (3,))
    assert f == np.inf and not g.any()
    # ... and a start that is infeasible is an error, not a result
    with pytest.raises(np.linalg.LinAlgError):
        hyper.optimize(p, lambda *a: good(*a)[:4] + (3,))


def test_optimize_restarts_consumes_the_global_stream_in_order(mods):
    gpy, hyper, _ = mods
    X, Y, k = known_problem(gpy, n=60)
    out = []
    for rep in range(2):
        kk = k.copy()
        p = hyper.Parameters(kk, 0.1 ** 2, 2)
        np.random.seed(11)
        res = hyper.optimize_restarts(p, hn.evaluator(kk, X, Y), num_restarts=3)
        after = np.random.normal()
        out.append((res.f_opt, res.x_opt.copy(), after, kk.lengthscale.copy(), p.noise_var))
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2] and out[0][4] == out[1][4]
    assert_array_equal(out[0][1], out[1][1])
    assert_array_equal(out[0][3], out[1][3])
    # documented order: restart r >= 1 draws its 4 starting values right before its run
    np.random.seed(11)
    np.random.normal(size=4)
    np.random.normal(size=4)
    assert np.random.normal() == out[0][2]
    # the best run is at least as good as the plain one
    kk = k.copy()
    p = hyper.Parameters(kk, 0.1 ** 2, 2)
    single = hyper.optimize(p, hn.evaluator(kk, X, Y))
    assert out[0][0] <= single.f_opt + 1e-9
