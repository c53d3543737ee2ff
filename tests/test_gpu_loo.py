"""Leave-one-out predictions, the log pseudo-likelihood with its gradient and
``optimize(objective='loo')`` on the device (needs an MI355X), through the public handle and
the C ABI, against the float64 closed form and the long-double brute force of
tests/_loo_ref.py.

PARITY_TOL: see profiles/loo/parity.txt -- 100 x the largest error measured against the
reference over the 666 cases of ``test_loo_matches_reference``,
``test_loo_lml_matches_reference``, ``test_n_2000`` and ``test_product_of_two_parts``
(1.423e-10, at n = 129, d = 1), never above 1e-6.  Errors: mean, ``L_LOO`` and the gradient
(in ``theta d/dtheta``) relative to ``max(1, |reference|)``, the variance relative to the
reference.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _hyper_numpy as hn
import _loo_ref as lr

pytestmark = pytest.mark.gpu

PARITY_TOL = 1.423e-8                   # 100 x 1.423e-10

KINDS = ["RBF", "Matern32", "Matern52"]
SIZES = [1, 7, 16, 17, 63, 64, 65, 129, 300]     # tile edge 64, k-step edge 16, single tiles
BRUTE_MAX = 33


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


def product_problem(gpy, n, seed=5):
    rng = np.random.default_rng(seed + n)
    X = rng.uniform(-2, 2, (n, 3))
    Y = (np.sin(X).sum(1) + 0.1 * rng.normal(size=n))[:, None]
    k = gpy.kern.Matern52(2, 1.3, [0.7, 1.9], ARD=True, active_dims=[0, 1]) * \
        gpy.kern.RBF(1, 0.8, 1.1, active_dims=[2], name="ctx")
    return X, Y, k


def cases(gpy, n, d):
    """(label, X, Y, kernel, noise) of one (n, d): every kind, ARD on and off, two noises"""
    X, Y = problem(n, d)
    for kind in KINDS:
        for ard in (True, False):
            for noise in (0.05 ** 2, 0.3 ** 2):
                ls = np.linspace(0.8, 1.6, d) if ard else np.array([1.1])
                yield ("n=%d d=%d %s ard=%d noise=%.4g" % (n, d, kind, ard, noise), X, Y,
                       getattr(gpy.kern, kind)(d, 1.7, ls, ARD=ard), noise)


def loo_error(got, ref):
    """(mean, var, sum_log_pred) of the device against (mean, var, ., L) of a reference"""
    mean, var, total = got
    return max(float(np.max(np.abs(mean - ref[0]) / np.maximum(1., np.abs(ref[0])))),
               float(np.max(np.abs(var - ref[1]) / np.abs(ref[1]))),
               float(abs(total - ref[3]) / max(1., abs(ref[3]))))


def gradient_error(out, ref, desc, noise):
    """value and gradient in theta d/dtheta, relative to max(1, |reference|)"""
    assert out[4] == 0 and ref[4] == 0
    err = abs(out[0] - ref[0]) / max(1., abs(ref[0]))
    for got, want, th in ((out[1], ref[1], noise), (out[2], ref[2], desc[2]),
                          (out[3], ref[3], desc[3])):
        got, want = np.asarray(got) * th, np.asarray(want) * th
        err = max(err, float(np.max(np.abs(got - want) / np.maximum(1., np.abs(want)))))
    return err


def check_loo(gpy, label, X, Y, k, noise):
    d = X.shape[1]
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
    desc = k._desc(d)
    kinds = list(desc[1])
    got = gp._fitted().loo()
    ref = lr.loo(kinds, X, Y, desc[2], desc[3], noise)
    err = loo_error(got, ref)
    if len(X) <= BRUTE_MAX:
        bm, bv = lr.brute_loo(kinds, X, Y, desc[2], desc[3], noise)
        bL = lr.brute_pseudo_likelihood(kinds, X, Y, desc[2], desc[3], noise)
        err = max(err, loo_error(got, (np.asarray(bm, float), np.asarray(bv, float), None,
                                       float(bL))))
    print("parity loo %s  err=%.3e" % (label, err))
    # the public methods are the same numbers
    mean, var = gp.loo()
    assert mean.shape == var.shape == (len(X), 1)
    assert_array_equal(mean[:, 0], got[0])
    assert_array_equal(var[:, 0], got[1])
    assert_array_equal(gp.loo_residuals(), (Y - mean) / np.sqrt(var))
    assert np.max(np.abs(gp.loo_residuals()[:, 0] - ref[2])) < PARITY_TOL * max(1., np.abs(ref[2]).max())
    return err


def check_loo_lml(gpy, label, X, Y, k, noise):
    d = X.shape[1]
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
    desc = k._desc(d)
    out = gp._fitted().loo_lml(desc[2], desc[3], noise)
    ref = lr.loo_lml(list(desc[1]), X, Y, desc[2], desc[3], noise)
    err = gradient_error(out, ref, desc, noise)
    print("parity loo_lml %s  err=%.3e  (value %.3e)"
          % (label, err, abs(out[0] - ref[0]) / max(1., abs(ref[0]))))
    assert_array_equal(out[3][desc[3] == 0.0], 0.0)          # unused columns: exactly 0
    return err


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [1, 3, 8])
def test_loo_matches_reference(mods, n, d):
    _, gpy, _, _ = mods
    worst = max(check_loo(gpy, *c) for c in cases(gpy, n, d))
    assert worst < PARITY_TOL, worst


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [1, 3, 8])
def test_loo_lml_matches_reference(mods, n, d):
    _, gpy, _, _ = mods
    worst = max(check_loo_lml(gpy, *c) for c in cases(gpy, n, d))
    assert worst < PARITY_TOL, worst


def test_n_2000(mods):
    _, gpy, _, _ = mods
    X, Y = problem(2000, 3)
    k = gpy.kern.Matern52(3, 1.7, np.linspace(0.8, 1.6, 3), ARD=True)
    label = "n=2000 d=3 Matern52 ard=1 noise=0.0025"
    assert check_loo(gpy, label, X, Y, k, 0.05 ** 2) < PARITY_TOL
    assert check_loo_lml(gpy, label, X, Y, k, 0.05 ** 2) < PARITY_TOL


@pytest.mark.parametrize("n", [7, 33, 65, 129])
def test_product_of_two_parts(mods, n):
    _, gpy, _, _ = mods
    X, Y, k = product_problem(gpy, n)
    for noise in (0.05 ** 2, 0.3 ** 2):
        label = "product n=%d noise=%.4g" % (n, noise)
        assert check_loo(gpy, label, X, Y, k, noise) < PARITY_TOL
        assert check_loo_lml(gpy, label, X, Y, k, noise) < PARITY_TOL
    gp = gpy.models.GPRegression(X, Y, k, noise_var=0.01)
    out = gp._fitted().loo_lml(k._desc(3)[2], k._desc(3)[3], 0.01)
    assert not out[3][0, 2] and not out[3][1, 0] and not out[3][1, 1]   # unused columns


def test_n_1_is_the_prior(mods):
    _, gpy, _, _ = mods
    k = gpy.kern.RBF(2, 1.7, [0.8, 1.6], ARD=True)
    gp = gpy.models.GPRegression(np.array([[0.3, -0.2]]), np.array([[0.7]]), k, noise_var=0.01)
    mean, var = gp.loo()
    assert abs(mean[0, 0]) < 1e-15 and abs(var[0, 0] - (1.7 + 0.01 + 1e-8)) < 1e-15


def test_same_theta_same_bits(mods):
    _, gpy, _, _ = mods
    X, Y = problem(500, 4)
    k = gpy.kern.Matern52(4, 1.7, np.linspace(0.8, 1.6, 4), ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=0.01)
    dev = gp._fitted()
    v, s = np.array([1.3]), 1.0 / np.linspace(0.6, 1.9, 4)[None]
    a = dev.loo_lml(v, s, 0.02)
    la = dev.loo()
    dev.loo_lml(v * 1.5, s * 0.7, 0.3)                  # something else in between
    dev.loo()
    b = dev.loo_lml(v, s, 0.02)
    lb = dev.loo()
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4] == 0
    assert_array_equal(a[2], b[2])
    assert_array_equal(a[3], b[3])
    assert_array_equal(la[0], lb[0])
    assert_array_equal(la[1], lb[1])
    assert la[2] == lb[2] == a[0]                       # one sum, one order
    # the marginal likelihood in between leaves the same factor behind
    dev.lml(v, s, 0.02)
    lc = dev.loo()
    assert_array_equal(la[0], lc[0])
    assert lc[2] == a[0]
    # the handle's own pseudo-likelihood after an edit in place is that value
    k.variance[0] = 1.3
    k.lengthscale[:] = np.linspace(0.6, 1.9, 4)
    gp.noise_var = 0.02
    serial = gp._fitted().serial
    assert gp.log_pseudo_likelihood() == a[0]
    assert gp._fitted().serial == serial


def test_after_incremental_updates(mods):
    """The factor a bordered append, a removal and a pop leave behind: rows and columns >= n
    of L^-1 hold whatever was there."""
    _, gpy, _, _ = mods
    X, Y = problem(62, 2)
    make = lambda: gpy.kern.Matern52(2, 1.7, [0.8, 1.6], ARD=True)
    gp = gpy.models.GPRegression(X[:61], Y[:61], make(), noise_var=0.05 ** 2)
    gp.set_XY(X[:60], Y[:60])                           # row 60 of L^-1 stays behind
    dev = gp._fitted()

    def against_fresh(Xc, Yc, what):
        fresh = gpy.models.GPRegression(Xc, Yc, make(), noise_var=0.05 ** 2)
        got, want = dev.loo(), fresh._fitted().loo()
        err = loo_error(got, (want[0], want[1], None, want[2]))
        ref = lr.loo([hn.MATERN52], Xc, Yc, np.array([1.7]), 1.0 / np.array([[0.8, 1.6]]),
                     0.05 ** 2)
        err = max(err, loo_error(got, ref))
        print("incremental %s: err=%.3e" % (what, err))
        assert err < PARITY_TOL
        assert gp._fitted() is dev

    against_fresh(X[:60], Y[:60], "pop to 60")
    gp.set_XY(X[:61], Y[:61])
    assert dev.appended
    against_fresh(X[:61], Y[:61], "append")
    gp.remove_data(23)
    assert dev.removed
    Xr, Yr = np.delete(X[:61], 23, axis=0), np.delete(Y[:61], 23, axis=0)
    against_fresh(Xr, Yr, "remove 23")
    gp.set_XY(Xr[:-1], Yr[:-1])
    assert dev.n == 59 and not dev.appended
    against_fresh(Xr[:-1], Yr[:-1], "pop")


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
    out = dev.loo_lml(desc[2], desc[3], -1.9e-8)
    assert out[4] != 0
    with pytest.raises(_hip.HipError):          # not fitted: no silent numbers
        dev.predict(X[:3])
    with pytest.raises(_hip.HipError):
        dev.loo()
    good = dev.loo_lml(desc[2], desc[3], 0.05 ** 2)
    ref = lr.loo_lml(list(desc[1]), X, Y, desc[2], desc[3], 0.05 ** 2)
    assert gradient_error(good, ref, desc, 0.05 ** 2) < PARITY_TOL
    m, v = dev.predict(X[:3])
    assert np.all(np.isfinite(m)) and np.all(v > 0)
    # through the handle: the objective is +inf there and the model recovers by itself
    p_bad = gp._evaluate_loo(desc[2], desc[3], -1.9e-8)
    assert p_bad[4] != 0
    m2, _ = gp.predict_noiseless(X[:3])
    assert np.max(np.abs(m2 - m)) < 1e-9
    # ... and so does an optimisation that finds the handle unfitted
    assert gp._evaluate_loo(desc[2], desc[3], -1.9e-8)[4] != 0
    res = gp.optimize(objective='loo', max_iters=30)
    assert np.isfinite(res.f_opt) and res.f_opt == -gp.log_pseudo_likelihood()
    with pytest.raises(ValueError):
        gp.optimize(objective='nonsense')


END_TO_END = [
    # n, d, kind, seed, ARD
    # (seeds chosen on the CPU, on the reference optimiser alone -- hyper.optimize fed by
    # _loo_ref.evaluator: it reports CONVERGENCE from these starts AND its last step ends
    # below pgtol rather than on the relative reduction of f, which most seeds stop on with
    # a gradient of 1e-4 .. 1e-2 in x.  With six free parameters -- 500 x 4, ARD -- none of
    # 150 seeds ends below pgtol; the second problem fits ONE length scale to data drawn with
    # four different ones: the kernel family that does not fit, which is what LOO-CV is for)
    (300, 2, "Matern52", 19, True),
    (500, 4, "RBF", 9, False),
]


def end_to_end_problem(gpy, n, d, kind, seed, ard):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (n, d))
    ls = np.linspace(0.9, 1.5, d)
    kinds = [{"RBF": hn.RBF, "Matern52": hn.MATERN52}[kind]]
    Y = hn.draw_gp(kinds, X, np.array([1.5]), (1.0 / ls)[None], 0.05 ** 2, seed + 100)
    # start at twice / half the truth
    start = np.where(np.arange(d) % 2 == 0, 2.0, 0.5) * ls
    make = lambda: getattr(gpy.kern, kind)(d, 3.0, start.copy() if ard else 2.0, ARD=ard)
    return X, Y, make, 2 * 0.05 ** 2


@pytest.mark.parametrize("n, d, kind, seed, ard", END_TO_END)
def test_optimize_loo_reaches_the_reference_optimum(mods, n, d, kind, seed, ard):
    _, gpy, _, hyper = mods
    X, Y, make, noise0 = end_to_end_problem(gpy, n, d, kind, seed, ard)
    k_ref = make()
    p_ref = hyper.Parameters(k_ref, noise0, d)
    ref = hyper.optimize(p_ref, lr.evaluator(k_ref, X, Y))
    assert "CONVERGENCE" in ref.status and "PGTOL" in ref.status
    k = make()
    gp = gpy.models.GPRegression(X, Y, k, noise_var=noise0)
    f0 = -gp.log_pseudo_likelihood()
    var_obj = k.variance
    res = gp.optimize(objective='loo')
    # the handle is fitted at the result: no refit, and it predicts like a fresh one.  Taken
    # directly after optimize(): anything that evaluates in between (log_pseudo_likelihood
    # factorises at the current values) would leave the device fitted there by itself
    dev = gp._dev
    version = dev.version
    print("optimize loo n=%d d=%d %s: device f=%.9f (%d evals, %s)  reference f=%.9f (%d evals)"
          % (n, d, kind, res.f_opt, res.funct_eval, res.status, ref.f_opt, ref.funct_eval))
    ls = k.lengthscale.copy()
    Xn = np.random.default_rng(2).uniform(-3, 3, (100, d))
    m, v = gp.predict_noiseless(Xn)
    assert gp._dev is dev and dev.version == version
    fresh = gpy.models.GPRegression(X, Y, getattr(gpy.kern, kind)(d, k.variance[0], ls, ARD=ard),
                                    noise_var=gp.noise_var)
    mf, vf = fresh.predict_noiseless(Xn)
    assert_array_equal(m, mf)
    assert_array_equal(v, vf)
    assert res.f_opt < f0 and k.variance is var_obj
    assert abs(res.f_opt - ref.f_opt) <= 1e-6 * n
    assert res.f_opt == -gp.log_pseudo_likelihood()
    # the default objective is the marginal likelihood, bit for bit
    out = []
    for kwargs in ({}, {"objective": "lml"}):
        kk = make()
        g2 = gpy.models.GPRegression(X, Y, kk, noise_var=noise0)
        r = g2.optimize(**kwargs)
        out.append((r.f_opt, r.x_opt, kk.variance.copy(), kk.lengthscale.copy(), g2.noise_var,
                    r.funct_eval))
    assert out[0][0] == out[1][0] and out[0][4] == out[1][4] and out[0][5] == out[1][5]
    for a, b in zip(out[0][1:4], out[1][1:4]):
        assert_array_equal(a, b)
    assert out[0][0] != res.f_opt


# ---- the faulty reading ---------------------------------------------------------------------
# 60 draws of two GPs on shared one-dimensional inputs; measurement FAULTY[1] of the second GP
# is shifted by 8 noise standard deviations.  Seed chosen on the CPU: by the brute-force
# reference the shifted measurement has max_g |z| = 8.60, every other one at most 2.91, and
# after its removal the largest is 2.16.
FAULTY = (11, 29)
FAULTY_SPECS = [("RBF", 1.5, 1.0), ("Matern52", 1.0, 1.2)]


def faulty_problem(gpy):
    seed, idx = FAULTY
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (60, 1))
    Ys = [hn.draw_gp([{"RBF": hn.RBF, "Matern52": hn.MATERN52}[kind]], X, np.array([v]),
                     np.array([[1.0 / ls]]), 0.05 ** 2, seed + 100 + g)
          for g, (kind, v, ls) in enumerate(FAULTY_SPECS)]
    assert int(rng.integers(5, 55)) == idx
    Ys[1][idx, 0] += 8 * 0.05
    gps = lambda: [gpy.models.GPRegression(X, Y, getattr(gpy.kern, kind)(1, v, ls),
                                           noise_var=0.05 ** 2)
                   for Y, (kind, v, ls) in zip(Ys, FAULTY_SPECS)]
    return X, Ys, gps, idx


def brute_z(X, Ys):
    return np.column_stack([
        np.asarray(lr.brute_residuals([{"RBF": hn.RBF, "Matern52": hn.MATERN52}[kind]], X, Y,
                                      np.array([v]), np.array([[1.0 / ls]]), 0.05 ** 2), float)
        for Y, (kind, v, ls) in zip(Ys, FAULTY_SPECS)])


def sets_of(opt):
    if hasattr(opt, "Q"):
        return {name: np.array(getattr(opt, name)) for name in ("Q", "S", "M", "G")}
    return {"S": np.array(opt.S), "greedy_point": np.array(opt.greedy_point),
            "best_lower_bound": np.array(opt.best_lower_bound)}


@pytest.mark.parametrize("which", ["SafeOpt", "SafeOptSwarm"])
def test_the_faulty_reading_is_found_and_removed(mods, which):
    safeopt_amd, gpy, _, _ = mods
    X, Ys, gps, idx = faulty_problem(gpy)

    def make():
        np.random.seed(3)
        if which == "SafeOpt":
            grid = safeopt_amd.linearly_spaced_combinations([(-3., 3.)], 400)
            return safeopt_amd.SafeOpt(gps(), grid, [-10., -10.], threshold=0.1)
        return safeopt_amd.SafeOptSwarm(gps(), [-10., -10.], bounds=[(-3., 3.)], threshold=0.1,
                                        swarm_size=64)

    opt, plain = make(), make()               # `plain` never calls the LOO methods
    np.random.seed(4)
    xa = opt.optimize()
    state = sets_of(opt)
    z = opt.loo_residuals()
    assert z.shape == (60, 2)
    zb = brute_z(X, Ys)
    assert np.argmax(np.abs(zb).max(1)) == idx and np.sum(np.abs(zb).max(1) > 3.0) == 1
    assert np.max(np.abs(z - zb)) < PARITY_TOL * np.abs(zb).max()
    assert opt.suspect_data_points() == [idx]
    for name, value in sets_of(opt).items():          # nothing of the optimiser moved
        assert_array_equal(value, state[name])
    np.random.seed(4)
    xb = plain.optimize()
    assert_array_equal(xa, xb)
    for name, value in sets_of(plain).items():
        assert_array_equal(value, state[name])
    opt.remove_data_point(idx)
    plain.remove_data_point(idx)
    assert opt.suspect_data_points() == []
    keep = np.arange(60) != idx
    fresh = [gpy.models.GPRegression(X[keep], Y[keep], getattr(gpy.kern, kind)(1, v, ls),
                                     noise_var=0.05 ** 2)
             for Y, (kind, v, ls) in zip(Ys, FAULTY_SPECS)]
    zf = np.column_stack([g.loo_residuals()[:, 0] for g in fresh])
    z = opt.loo_residuals()
    assert z.shape == (59, 2)
    assert np.max(np.abs(z - zf)) < PARITY_TOL * np.abs(zf).max()
    np.random.seed(5)
    xa = opt.optimize()
    np.random.seed(5)
    xb = plain.optimize()
    assert_array_equal(xa, xb)
    want = sets_of(plain)
    for name, value in sets_of(opt).items():
        assert_array_equal(value, want[name])
