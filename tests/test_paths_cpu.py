"""Posterior sample paths, host side (no GPU): the spectral draws of safeopt_amd/paths.py, the
NumPy statement of the path (tests/_paths_numpy.py) against the posterior of the oracle, the
order of the draws, and the snapshot rules of ``PosteriorPaths`` with the evaluation replaced
by the NumPy form."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
from _joint_numpy import joint_posterior
from safeopt_amd import paths as P

RBF, M32, M52 = P.RBF, P.MATERN32, P.MATERN52

# kernels as the C ABI describes them: (kinds, variances, inv_ls (P, d)), d = 2
SPECTRAL = {
    "RBF": ([RBF], [1.7], [[1 / 0.8, 1 / 1.6]]),
    "Matern32": ([M32], [1.7], [[1 / 0.8, 1 / 1.6]]),
    "Matern52": ([M52], [1.7], [[1 / 0.8, 1 / 1.6]]),
    "product": ([RBF, M52], [1.3, 0.9], [[1 / 0.7, 0.0], [0.0, 1 / 1.2]]),
}
M_BIG = 2 ** 18
SEED = 20201


def pairs(kern):
    """20 pairs (0, x') at 0 .. 3 lengthscales along a fixed direction (scaled units)."""
    inv_ls = np.asarray(kern[2], dtype=float)
    scale = np.sqrt((inv_ls ** 2).sum(0))            # per column, over the parts
    u = np.array([0.6, 0.8])
    t = np.linspace(0.0, 3.0, 20)
    return np.zeros((20, 2)), t[:, None] * (u / scale)[None, :]


def feature_estimate(kern, dof=None):
    """(2 v / m) sum_i cos(w_i x + b_i) cos(w_i x' + b_i) and k(x, x') at the 20 pairs."""
    rng = np.random.RandomState(SEED)
    Om, b, _, _ = P.draw_path_inputs((kern[0], kern[2]), 0.0, 1, 2, 1, M_BIG, rng=rng, dof=dof)
    x0, x1 = pairs(kern)
    v = pn.prior_variance(kern)
    est = (2 * v / M_BIG) * (np.cos(pn.feature_args(Om, b, x0)) *
                             np.cos(pn.feature_args(Om, b, x1))).sum(1)
    exact = np.array([pn.kernel_matrix(kern, x0[i:i + 1], x1[i:i + 1])[0, 0] for i in range(20)])
    return est, exact, v


@pytest.mark.parametrize("name", sorted(SPECTRAL))
def test_spectral_draws_reproduce_the_kernel(name):
    """Every summand is bounded by 2 v, so the standard deviation of the mean is at most
    2 v / sqrt(m); the bound is four of those, 8 v / sqrt(m) = 0.0156 v."""
    est, exact, v = feature_estimate(SPECTRAL[name])
    err = np.abs(est - exact)
    print("%s: max |estimate - k| = %.3e v (bound %.3e v)" % (name, err.max() / v,
                                                             8 / np.sqrt(M_BIG)))
    assert err.max() <= 8 * v / np.sqrt(M_BIG)


def test_wrong_degrees_of_freedom_fall_outside_the_bound():
    """The bound discriminates: Matern-3/2 drawn with 5 degrees of freedom (the Matern-5/2
    measure) misses it at some pair."""
    wrong = dict(P.SPECTRAL_DOF)
    wrong[M32] = 5
    est, exact, v = feature_estimate(SPECTRAL["Matern32"], dof=wrong)
    assert np.abs(est - exact).max() > 8 * v / np.sqrt(M_BIG)


# ---- the path is a posterior sample ------------------------------------------------------------

NOISE = 0.05 ** 2


def small_problem(n=17, d=2, m=68, S=5, N=63, seed=5):
    rng = np.random.RandomState(seed)
    kern = ([M52], [1.7], [list(1 / np.linspace(0.8, 1.6, d))])
    X = rng.uniform(-2.5, 2.5, (n, d))
    y = np.sin(X).sum(1) + 0.05 * rng.standard_normal(n)
    Xs = rng.uniform(-3, 3, (N, d))
    Om, b, W, E = P.draw_path_inputs((kern[0], kern[2]), NOISE, n, d, S, m, rng=rng)
    return kern, X, y, Xs, Om, b, W, E


def test_zero_draws_give_the_posterior_mean():
    """E = 0, W = 0: V = alpha and the path is the posterior mean -- of the oracle GP (same Ky:
    noise + 1e-8), to the long-double discrepancy of the helper.

    The bound is 4 x disc, disc = max |float64 path - long-double path|.  Both sides of the
    comparison are float64 solves with the same Ky, so each is off the true mean by an error of
    disc's order and their difference by up to the sum of the two (factor 2); disc is one
    realised maximum over 63 x 5 entries, not an upper bound of that error (factor 2).  No
    floor: disc itself is what the format gives at this conditioning.  Measured on this case:
    |path - mean| = 6.5e-15, disc = 2.7e-15, ratio 2.4."""
    from oracle import gp_numpy as gpn
    kern, X, y, Xs, Om, b, W, E = small_problem()
    W0, E0 = np.zeros_like(W), np.zeros_like(E)
    V = pn.path_weights(kern, NOISE, X, y, Om, b, W0, E0)
    f = pn.paths_eval(kern, X, Om, b, W0, V, Xs)
    Vl = pn.path_weights_ld(kern, NOISE, X, y, Om, b, W0, E0)
    fl = pn.paths_eval_ld(kern, X, Om, b, W0, Vl, Xs)
    disc = float(np.abs(f - fl).max())
    g = gpn.GPRegression(X, y[:, None], gpn.Matern52(2, 1.7, np.linspace(0.8, 1.6, 2), ARD=True),
                         noise_var=NOISE)
    mean, _ = joint_posterior(g, Xs)
    err = np.abs(f - mean).max()
    print("path - posterior mean %.3e, long-double discrepancy %.3e, ratio %.2f"
          % (err, disc, err / disc))
    assert err <= 4 * disc
    assert_array_equal(f, np.repeat(f[:, :1], f.shape[1], axis=1))     # every path the same


def test_zero_weights_give_the_prior_draw():
    kern, X, y, Xs, Om, b, W, E = small_problem()
    f = pn.paths_eval(kern, X, Om, b, W, np.zeros((X.shape[0], W.shape[1])), Xs)
    assert_array_equal(f, pn.features(kern, Om, b, Xs).dot(W))


def test_weights_condition_the_path_on_the_data():
    """With E = 0 the path interpolates what the posterior mean does to the prior draw:
    f(X) + noise-weighted residual = y, i.e. Ky V = y - Phi(X) W."""
    kern, X, y, Xs, Om, b, W, E = small_problem()
    V = pn.path_weights(kern, NOISE, X, y, Om, b, W, E)
    Ky = pn.gram(kern, NOISE, X)
    rhs = pn.weight_rhs(kern, X, y, Om, b, W, E)
    assert pn.weights_residual(Ky, V, rhs) < 100 * X.shape[0] * 2.0 ** -53


# ---- draw order and shapes ---------------------------------------------------------------------

def test_draw_order_and_shapes():
    kinds, inv_ls = [RBF, M32], np.array([[2.0, 0.0, 0.0], [0.0, 0.5, 0.0]])
    a = P.draw_path_inputs((kinds, inv_ls), 0.01, 7, 3, 4, 11, rng=np.random.RandomState(3))
    b = P.draw_path_inputs((kinds, inv_ls), 0.01, 7, 3, 4, 11, rng=np.random.RandomState(3))
    for u, v in zip(a, b):
        assert_array_equal(u, v)
    Om, ph, W, E = a
    assert Om.shape == (11, 3) and ph.shape == (11,) and W.shape == (11, 4) and E.shape == (7, 4)
    assert_array_equal(Om[:, 2], np.zeros(11))          # a column no part uses
    assert np.all(Om[:, :2] != 0.0)
    assert np.all((ph >= 0) & (ph < 2 * np.pi))
    # the documented order, drawn by hand from the same stream
    r = np.random.RandomState(3)
    z0 = r.standard_normal((11, 3))
    z1 = r.standard_normal((11, 3))
    u1 = r.chisquare(3, 11)
    assert_array_equal(Om, inv_ls[0] * z0 + inv_ls[1] * (z1 / np.sqrt(u1 / 3)[:, None]))
    assert_array_equal(ph, 2 * np.pi * r.random_sample(11))
    assert_array_equal(W, r.standard_normal((11, 4)))
    assert_array_equal(E, np.sqrt(0.01 + 1e-8) * r.standard_normal((7, 4)))
    # the global generator is the default and advances exactly that far
    np.random.seed(3)
    c = P.draw_path_inputs((kinds, inv_ls), 0.01, 7, 3, 4, 11)
    for u, v in zip(a, c):
        assert_array_equal(u, v)
    assert np.random.random_sample() == r.random_sample()
    # a Generator works as well
    g = P.draw_path_inputs((kinds, inv_ls), 0.01, 7, 3, 4, 11, rng=np.random.default_rng(3))
    assert g[0].shape == (11, 3)
    with pytest.raises(ValueError):
        P.draw_path_inputs((kinds, inv_ls), 0.01, 7, 3, 0, 11)
    with pytest.raises(ValueError):
        P.draw_path_inputs(([7], inv_ls[:1]), 0.01, 7, 3, 1, 11)


# ---- the snapshot ------------------------------------------------------------------------------

class _Handle(object):
    """What GPRegression gives a PosteriorPaths: a version token and an evaluation -- here the
    NumPy form."""

    def __init__(self):
        self.kern, self.X, self.y, self.Xs, Om, b, W, E = small_problem()
        self.token = (1, 0)
        V = pn.path_weights(self.kern, NOISE, self.X, self.y, Om, b, W, E)
        self.paths = P.PosteriorPaths(
            Om, b, W, V, lambda Z: pn.paths_eval(self.kern, self.X, Om, b, W, V, Z),
            lambda: self.token)


def test_posterior_paths_shapes_and_repeats():
    h = _Handle()
    pp = h.paths
    assert (pp.size, pp.features, pp.input_dim) == (5, 68, 2)
    f = pp.paths(h.Xs)
    assert f.shape == (63, 1, 5)
    assert_array_equal(pp.paths(h.Xs), f)
    assert_array_equal(pp.paths(h.Xs[10:20])[:, 0, :], f[10:20, 0, :])
    assert pp.paths(h.Xs[3]).shape == (1, 1, 5)          # one row as a vector
    assert pp.paths(np.empty((0, 2))).shape == (0, 1, 5)


def test_posterior_paths_are_a_snapshot():
    h = _Handle()
    h.paths.paths(h.Xs)
    h.token = (1, 1)                       # set_XY, an append, an edited hyper-parameter
    with pytest.raises(ValueError, match="stale"):
        h.paths.paths(h.Xs)
    with pytest.raises(ValueError, match="stale"):
        h.paths.check()
    h.token = (1, 0)
    h.paths.paths(h.Xs)


def test_posterior_paths_argument_errors():
    h = _Handle()
    with pytest.raises(ValueError, match="2 columns"):
        h.paths.paths(np.zeros((4, 3)))
    pp = h.paths
    with pytest.raises(ValueError, match="inconsistent"):
        P.PosteriorPaths(pp.Omega, pp.phase[:-1], pp.W, pp.V, None, lambda: 0)
    with pytest.raises(ValueError, match="inconsistent"):
        P.PosteriorPaths(pp.Omega, pp.phase, pp.W, pp.V[:, :-1], None, lambda: 0)
