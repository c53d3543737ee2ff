"""Joint prediction (``full_cov=True``) and posterior sample paths on the device against the
NumPy reference of tests/_joint_numpy.py (needs an MI355X).

Shapes: n in {1, 17, 100, 300} training points (no multiple of 16; one, two, seven and nineteen
row blocks of the packed L^-1, the last one narrow for 1, 17 and 100) x N in {1, 17, 257} points
(257: five 64-tiles with a one-column tail, off-diagonal tiles and their mirror images, and a
factorisation padded from 257 to 288).  Tolerances are the project's (tests/_gpu_common.py):
MEAN_TOL of max|mean|, VAR_TOL of the prior variance -- the two forms of the reference differ by
at most 4e-12 of the prior variance over these shapes (tests/test_joint_host.py).
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _gpu_common import MEAN_TOL, VAR_TOL, mods, smooth, kernels, product_kernel  # noqa: F401
from _joint_numpy import joint_posterior

pytestmark = pytest.mark.gpu

NOISE = 0.05 ** 2
KINDS = ["RBF", "Matern32", "Matern52", "product"]
SIZES = [(n, N) for n in (1, 17, 100, 300) for N in (1, 17, 257)]
PRODUCT = [("Matern52", [0, 1]), ("RBF", [1, 2])]        # three columns, column 1 shared


def make_kernel(ns, kind):
    if kind == "product":
        return product_kernel(ns, 3, PRODUCT, 7)
    return kernels(ns, kind, 2)


def data(kind, n, N):
    d = 3 if kind == "product" else 2
    rng = np.random.default_rng(100000 + 1000 * n + N)
    X = rng.uniform(-2.5, 2.5, (n, d))
    Y = smooth(X, n) + 0.05 * rng.normal(size=(n, 1))
    Xs = rng.uniform(-3, 3, (N, d))
    return X, Y, Xs


@functools.lru_cache(maxsize=None)
def reference(kind, n, N):
    """(Xs, mean, cov, prior variance) of the oracle GP: computed once, never modified."""
    from oracle import gp_numpy as gpn
    X, Y, Xs = data(kind, n, N)
    k = make_kernel(gpn, kind)
    g = gpn.GPRegression(X, Y, k, noise_var=NOISE)
    mean, cov = joint_posterior(g, Xs)
    prior = float(k.Kdiag(Xs[:1])[0])
    for a in (Xs, mean, cov):
        a.setflags(write=False)
    return Xs, mean, cov, prior


_GPS = {}


def device_gp(gpy, kind, n, N):
    key = (kind, n, N)
    if key not in _GPS:
        X, Y, _ = data(kind, n, N)
        _GPS[key] = gpy.models.GPRegression(X, Y, make_kernel(gpy.kern, kind), noise_var=NOISE)
    return _GPS[key]


def check_cov(m, c, mean_ref, cov_ref, prior):
    N = mean_ref.shape[0]
    assert m.shape == (N, 1) and c.shape == (N, N)
    dm = np.max(np.abs(m - mean_ref)) / max(np.max(np.abs(mean_ref)), 1e-300)
    dc = np.max(np.abs(c - cov_ref)) / prior
    print("mean %.3e  cov %.3e" % (dm, dc))
    assert dm < MEAN_TOL
    assert dc < VAR_TOL
    assert_array_equal(c, c.T)


@pytest.mark.parametrize("n,N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_full_cov_matches_reference(mods, kind, n, N):
    _, gpy, _, _ = mods
    Xs, mean_ref, cov_ref, prior = reference(kind, n, N)
    gp = device_gp(gpy, kind, n, N)
    m, c = gp.predict_noiseless(Xs, full_cov=True)
    check_cov(m, c, mean_ref, cov_ref, prior)
    # the diagonal against the per-point variance (clipped at 1e-15 there, not here)
    m1, v1 = gp.predict_noiseless(Xs)
    open_ = v1[:, 0] > 1e-15
    assert np.max(np.abs(np.diag(c)[open_] - v1[open_, 0]), initial=0.0) / prior < VAR_TOL
    assert np.max(np.abs(m - m1)) / max(np.max(np.abs(mean_ref)), 1e-300) < MEAN_TOL
    # _raw_predict is the same call; predict adds the noise to the diagonal only
    m2, c2 = gp._raw_predict(Xs, full_cov=True)
    assert_array_equal(m2, m)
    assert_array_equal(c2, c)
    m3, c3 = gp.predict(Xs, full_cov=True)
    assert_array_equal(m3, m)
    off = ~np.eye(N, dtype=bool)
    assert_array_equal(c3[off], c[off])
    assert np.max(np.abs(np.diag(c3) - np.diag(c) - NOISE)) <= 4 * np.finfo(float).eps * prior
    m4, c4 = gp.predict(Xs, full_cov=True, include_likelihood=False)
    assert_array_equal(c4, c)


@pytest.mark.parametrize("n,N", [(17, 17), (300, 257)])
@pytest.mark.parametrize("kind", ["Matern52", "product"])
def test_layouts_and_repeats_give_the_same_bits(mods, kind, n, N):
    _, gpy, _, _ = mods
    Xs = reference(kind, n, N)[0]
    gp = device_gp(gpy, kind, n, N)
    m, c = gp.predict_noiseless(np.ascontiguousarray(Xs), full_cov=True)
    wide = np.zeros((2 * N, 2 * Xs.shape[1] + 1))
    wide[::2, 1::2] = Xs
    for other in (np.asfortranarray(Xs), wide[::2, 1::2], np.ascontiguousarray(Xs)):
        m2, c2 = gp.predict_noiseless(other, full_cov=True)
        assert_array_equal(m2, m)
        assert_array_equal(c2, c)
    Z = np.random.default_rng(3).normal(size=(N, 3))
    a = gp._fitted().draw(Xs, Z)
    b = gp._fitted().draw(np.asfortranarray(Xs), Z)
    assert_array_equal(a[0], b[0])
    assert_array_equal(a[1], b[1])
    assert a[2] == b[2]


@pytest.mark.parametrize("n,N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_draw_factor_and_samples(mods, kind, n, N):
    """Z = I returns the Cholesky factor itself: lower triangular, positive diagonal, and
    C C^T = cov + jitter_used I to VAR_TOL of the prior variance (the backward error of a
    Cholesky factorisation at N = 257 is about N eps = 6e-14 ... 2e-11 of that scale whatever
    the conditioning -- C itself is NOT compared with a host factor, which would amplify by the
    condition number).  Then a general Z against mean + C Z formed on the host."""
    _, gpy, _, _ = mods
    Xs, mean_ref, cov_ref, prior = reference(kind, n, N)
    dev = device_gp(gpy, kind, n, N)._fitted()
    out, mean, jitter = dev.draw(Xs, np.eye(N))
    assert out.shape == (N, N) and mean.shape == (N, 1)
    assert np.max(np.abs(mean - mean_ref)) / max(np.max(np.abs(mean_ref)), 1e-300) < MEAN_TOL
    C = out - mean
    assert_array_equal(C[np.triu_indices(N, 1)], 0.0)
    assert np.all(np.diag(C) > 0.0)
    res = np.max(np.abs(C.dot(C.T) - cov_ref - jitter * np.eye(N))) / prior
    print("jitter %.3e  residual %.3e" % (jitter, res))
    if kind in ("Matern32", "Matern52"):
        # the reference factorises without jitter: smallest eigenvalue >= 8e-7, rounding 1e-12
        assert jitter == 0.0
    else:
        # RBF (and the product with an RBF part): the reference matrix is indefinite at rounding
        # level at N = 257, so a retry may or may not happen -- but only GPy's jitter values
        allowed = [0.0] + [np.mean(np.diag(cov_ref)) * 1e-6 * 10.0 ** k for k in range(5)]
        assert any(abs(jitter - a) <= 1e-6 * a for a in allowed), (jitter, allowed)
    assert res <= VAR_TOL
    # a general Z, S = 3
    Z = np.random.default_rng(11).normal(size=(N, 3))
    out3, mean3, jitter3 = dev.draw(Xs, Z)
    assert_array_equal(mean3, mean)
    assert jitter3 == jitter
    want = mean + C.dot(Z)
    assert np.max(np.abs(out3 - want)) <= 1e-12 * np.max(np.abs(out3))


def test_posterior_samples_use_the_global_stream_once(mods):
    _, gpy, _, _ = mods
    kind, n, N, size = "Matern52", 100, 17, 4
    Xs = reference(kind, n, N)[0]
    gp = device_gp(gpy, kind, n, N)
    np.random.seed(5)
    f = gp.posterior_samples_f(Xs, size=size)
    after = np.random.rand()
    assert f.shape == (N, 1, size)
    np.random.seed(5)
    Z = np.random.randn(N, size)
    assert after == np.random.rand()                 # exactly one randn(N, size) was consumed
    out, _, _ = gp._fitted().draw(Xs, Z)
    assert_array_equal(f[:, 0, :], out)
    # posterior_samples: the same paths plus sqrt(noise_var) times a second draw
    np.random.seed(5)
    y = gp.posterior_samples(Xs, size=size)
    np.random.seed(5)
    np.random.randn(N, size)
    E = np.random.randn(N, 1, size)
    assert y.shape == (N, 1, size)
    assert np.max(np.abs(y - f - np.sqrt(NOISE) * E)) <= 1e-14 * np.max(np.abs(y))


def test_follows_data_and_hyperparameter_changes(mods):
    """One more row through ``set_XY`` (the bordered update) and an in-place edit of
    ``kern.lengthscale``: ``full_cov`` matches a freshly built oracle GP each time."""
    _, gpy, gpn, _ = mods
    kind, n, N = "Matern52", 100, 17
    X, Y, Xs = data(kind, n + 1, N)
    gp = gpy.models.GPRegression(X[:n], Y[:n], make_kernel(gpy.kern, kind), noise_var=NOISE)
    gp.predict_noiseless(Xs, full_cov=True)
    gp.set_XY(X, Y)
    assert gp._dev.appended
    ko = make_kernel(gpn, kind)
    mean_ref, cov_ref = joint_posterior(gpn.GPRegression(X, Y, ko, noise_var=NOISE), Xs)
    m, c = gp.predict_noiseless(Xs, full_cov=True)
    check_cov(m, c, mean_ref, cov_ref, 1.7)
    gp.kern.lengthscale[0] = 1.1
    ko.lengthscale[0] = 1.1
    mean_ref, cov_ref = joint_posterior(gpn.GPRegression(X, Y, ko, noise_var=NOISE), Xs)
    m, c = gp.predict_noiseless(Xs, full_cov=True)
    check_cov(m, c, mean_ref, cov_ref, 1.7)


def test_too_many_rows_and_unfitted_gp(mods):
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    gp = device_gp(gpy, "Matern52", 17, 17)
    big = np.zeros((_hip.MAX_JOINT + 1, 2))
    with pytest.raises(ValueError, match="SGP_MAX_JOINT"):
        gp.predict_noiseless(big, full_cov=True)
    with pytest.raises(ValueError, match="SGP_MAX_JOINT"):
        gp.posterior_samples_f(big, size=1)
    # the C ABI refuses it too, and a GP without data: error returns, nothing is written
    import ctypes as C
    dev = gp._fitted()
    mean = np.full(3, 7.0)
    rc = _hip.lib().sgp_gp_predict_cov(dev.h, _hip.dptr(big), big.shape[0], 2, 1,
                                       _hip.dptr(mean), None)
    assert rc < 0 and b"SGP_MAX_JOINT" in _hip.lib().sgp_last_error(dev.ctx.h)
    assert_array_equal(mean, 7.0)
    empty = _hip.DeviceGP(dev.ctx, make_kernel(gpy.kern, "Matern52")._desc(2), NOISE)
    with pytest.raises(_hip.HipError):
        empty.predict_cov(np.zeros((3, 2)))
    with pytest.raises(_hip.HipError):
        empty.draw(np.zeros((3, 2)), np.zeros((3, 1)))
