"""Leave-one-out diagnostics without a GPU: the closed form (tests/_loo_ref.py, the
specification of ``sgp_gp_loo`` / ``sgp_gp_loo_lml``) against the long-double brute force, its
analytic gradient against central differences of the brute-force ``L_LOO``, the host logic of
``suspect_data_points`` and ``optimize(objective=...)``, and the declarations of the ABI.

Closed form vs brute force: 1e-10 (mean and z absolute, variance relative, ``L_LOO`` relative to
max(1, |L|)); float64 with cond(Ky) <= 1e6 supports about 1e-10, measured worst 8.1e-13 (the
residual z at n = 33, d = 1, Matern-5/2, noise 0.05^2).

Gradient: central differences with the relative step H = 1e-6 in every parameter, compared
in ``theta d/dtheta`` relative to ``max(1, |.|)``.  Long double (eps = 1.1e-19) leaves a
rounding error of eps |L| / H ~ 1e-12 in the difference quotient and the truncation error is
H^2 theta^3 L''' / 6 ~ 1e-12 .. 1e-11 (with H = 1e-5 the error of a well-conditioned case is
2.5e-10, with H = 1e-4 2.5e-8: the h^2 law), so the quotient is good to about 1e-11.  What it
is compared with is the float64 closed form, which holds Ky^-1 twice (C^T C): its error is
bounded by about eps_64 cond(Ky)^2 with cond(Ky) <= 1 + n v / noise = 2.7e4 at n = 40, i.e.
8e-8.  GRAD_TOL = 1e-7; measured worst 3.1e-9 (n = 40, d = 1, RBF: cond(Ky) = 1.3e4), 1.4e-11
on the three-dimensional cases."""
import os
import re

import numpy as np
import pytest

import _hyper_numpy as hn
import _loo_ref as lr
from safeopt_amd import _hip, gp_opt, gpy

LD = np.longdouble
CLOSED_TOL = 1e-10
H = 1e-6
GRAD_TOL = 1e-7


def problem(n, d, spec, seed=0):
    """(kinds, X, y, variances, inv_ls) -- spec: a kind, or 'product' (Matern-5/2 on columns
    0, 1 times RBF on column 2, d = 3)"""
    rng = np.random.default_rng(1000 * n + 10 * d + seed)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X).sum(1) + 0.1 * rng.normal(size=n)
    if spec == "product":
        inv_ls = np.zeros((2, 3))
        inv_ls[0, :2] = 1.0 / np.array([0.7, 1.9])
        inv_ls[1, 2] = 1.0 / 1.1
        return [hn.MATERN52, hn.RBF], X, y, np.array([1.3, 0.8]), inv_ls
    return [spec], X, y, np.array([1.7]), (1.0 / np.linspace(0.8, 1.6, d))[None]


SPECS = [(d, kind) for d in (1, 3) for kind in (hn.RBF, hn.MATERN32, hn.MATERN52)] + \
        [(3, "product")]


@pytest.mark.parametrize("n", [1, 2, 7, 33])
@pytest.mark.parametrize("d, spec", SPECS)
def test_closed_form_equals_brute_force(n, d, spec):
    kinds, X, y, v, s = problem(n, d, spec)
    for noise in (0.05 ** 2, 0.3 ** 2):
        mean, var, z, L = lr.loo(kinds, X, y, v, s, noise)
        bm, bv = lr.brute_loo(kinds, X, y, v, s, noise)
        bz = lr.brute_residuals(kinds, X, y, v, s, noise)
        bL = lr.brute_pseudo_likelihood(kinds, X, y, v, s, noise)
        errs = (np.max(np.abs(mean - bm)), np.max(np.abs(var - bv) / bv),
                np.max(np.abs(z - bz)), abs(L - bL) / max(1.0, abs(bL)))
        print("closed n=%d d=%d %s noise=%.4g  mean %.1e var %.1e z %.1e L %.1e"
              % ((n, d, spec, noise) + tuple(float(e) for e in errs)))
        assert max(errs) < CLOSED_TOL
        assert lr.loo_lml(kinds, X, y, v, s, noise)[0] == L
    if n == 1:                                # the prior
        assert abs(mean[0]) < 1e-15 and abs(var[0] - (np.prod(v) + noise + 1e-8)) < 1e-15


@pytest.mark.parametrize("n", [7, 40])
@pytest.mark.parametrize("d, spec", SPECS)
def test_gradient_equals_central_differences(n, d, spec):
    kinds, X, y, v, s = problem(n, d, spec)
    noise = 0.05 ** 2
    L, g_noise, g_var, g_ils, info = lr.loo_lml(kinds, X, y, v, s, noise)
    assert info == 0

    def quotient(which, p=0, a=0):
        out = []
        for sign in (1, -1):
            vv, ss, nn = np.asarray(v, LD).copy(), np.asarray(s, LD).copy(), LD(noise)
            if which == "noise":
                nn = nn * (1 + sign * LD(H))
            elif which == "var":
                vv[p] = vv[p] * (1 + sign * LD(H))
            else:
                ss[p, a] = ss[p, a] * (1 + sign * LD(H))
            out.append(lr.brute_pseudo_likelihood(kinds, X, y, vv, ss, nn))
        return float((out[0] - out[1]) / (2 * LD(H)))          # = theta d/dtheta

    worst = 0.0
    checks = [("noise", 0, 0, g_noise * noise)]
    for p in range(len(kinds)):
        checks.append(("var", p, 0, g_var[p] * v[p]))
        for a in range(X.shape[1]):
            if s[p, a] != 0.0:
                checks.append(("ils", p, a, g_ils[p, a] * s[p, a]))
            else:
                assert g_ils[p, a] == 0.0
    for which, p, a, got in checks:
        want = quotient(which, p, a)
        worst = max(worst, abs(got - want) / max(1.0, abs(want)))
    print("gradient n=%d d=%d %s: worst %.2e over %d parameters" % (n, d, spec, worst, len(checks)))
    assert worst < GRAD_TOL


# ---- suspect_data_points on a stubbed loo_residuals ---------------------------------------------
def _stub_opt(z):
    opt = object.__new__(gp_opt.GaussianProcessOptimization)
    opt.loo_residuals = lambda: np.array(z, dtype=float)
    return opt


def test_suspects_ordering_ties_and_threshold():
    z = [[0.5, -3.5], [4.0, 0.1], [-3.0, 3.0], [-4.0, 1.0], [3.5, np.nan], [0.0, 7.0]]
    opt = _stub_opt(z)
    assert opt.suspect_data_points() == [5, 1, 3, 0, 4]         # 7, 4, 4 (by index), 3.5, 3.5
    assert opt.suspect_data_points(threshold=3.5) == [5, 1, 3]  # strictly above
    assert opt.suspect_data_points(threshold=2.9) == [5, 1, 3, 0, 4, 2]
    assert opt.suspect_data_points(threshold=10.0) == []
    assert all(type(i) is int for i in opt.suspect_data_points())
    assert _stub_opt(np.zeros((4, 1))).suspect_data_points() == []


def test_loo_residuals_of_a_log_with_gaps():
    """Column g = GP g's z on the rows it observed, nan elsewhere."""
    y = np.array([[1.0, 10.0], [2.0, np.nan], [np.nan, 30.0], [4.0, 40.0]])
    opt = object.__new__(gp_opt.GaussianProcessOptimization)
    opt._y = y

    class _GP(object):
        def __init__(self, z):
            self.z = np.array(z)[:, None]

        def loo_residuals(self):
            return self.z

    opt.gps = [_GP([0.1, 0.2, 0.4]), _GP([1.0, 3.0, 4.0])]
    z = opt.loo_residuals()
    assert z.shape == (4, 2)
    np.testing.assert_array_equal(z, [[0.1, 1.0], [0.2, np.nan], [np.nan, 3.0], [0.4, 4.0]])
    assert opt.suspect_data_points(threshold=2.0) == [3, 2]


# ---- objective= ---------------------------------------------------------------------------------
def test_unknown_objective_raises_before_any_device_use():
    gp = object.__new__(gpy.GPRegression)

    def no_device(*a, **k):
        raise AssertionError("device use")

    gp._fitted = gp._device_gp = no_device
    with pytest.raises(ValueError):
        gp.optimize(objective="nonsense")
    with pytest.raises(ValueError):
        gp.optimize_restarts(num_restarts=2, objective="nonsense")
    assert gp._evaluator("lml") == gp._evaluate and gp._evaluator("loo") == gp._evaluate_loo


def test_loo_objective_is_a_second_evaluate_callback():
    """``hyper.optimize`` takes the LOO evaluator as it takes the likelihood's: it improves
    ``-L_LOO`` from the start and ends where the gradient vanishes."""
    from safeopt_amd import hyper
    kinds, X, y, v, s = problem(40, 1, hn.MATERN52)
    k = gpy.kern.Matern52(1, 3.0, 0.5)
    params = hyper.Parameters(k, 0.1, 1)
    ev = lr.evaluator(k, X, y)
    f0 = params.objective(params.get_x(), ev)[0]
    res = hyper.optimize(params, ev)
    f, g = params.objective(res.x_opt, ev)
    assert res.f_opt < f0 and f == res.f_opt and np.max(np.abs(g)) < 1e-3


# ---- the C ABI ----------------------------------------------------------------------------------
def test_entry_points_are_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "safeopt_hip.h")).read()
    for name in ("sgp_gp_loo", "sgp_gp_loo_lml"):
        assert name in _hip.PROTOTYPES
        assert re.search(r"\bint %s\(" % name, header)
    assert _hip.PROTOTYPES["sgp_gp_loo_lml"] == _hip.PROTOTYPES["sgp_gp_lml"]
    for name in ("loo", "loo_lml"):
        assert callable(getattr(_hip.DeviceGP, name))
    for name in ("loo", "loo_residuals", "log_pseudo_likelihood"):
        assert callable(getattr(gpy.GPRegression, name))
