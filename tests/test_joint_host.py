"""The reference arithmetic of the joint posterior (tests/_joint_numpy.py) pinned on the CPU, and
the two entry points of the C ABI that compute it on the device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import gp_numpy as gpn
from _joint_numpy import joint_posterior, joint_posterior_woodbury

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 0.05 ** 2


def _problem(kind, n, N, d=2):
    rng = np.random.default_rng(1000 * n + N)
    X = rng.uniform(-2.5, 2.5, (n, d))
    Y = np.sin(X.sum(1))[:, None] + 0.05 * rng.normal(size=(n, 1))
    Xs = rng.uniform(-3, 3, (N, d))
    ls = np.linspace(0.8, 1.6, d)
    return X, Y, Xs, ls


@pytest.mark.parametrize("kind", ["RBF", "Matern32", "Matern52"])
@pytest.mark.parametrize("n,N", [(1, 17), (17, 257), (100, 257), (300, 17)])
def test_two_forms_of_the_covariance_agree(kind, n, N):
    """V^T V against Kx^T Ky^-1 Kx.  1e-10 of the prior variance: both forms carry rounding of
    about cond(Ky) * eps = (1.7 n / noise) * 1e-16 < 3e-11 relative to the prior variance at
    n = 300."""
    X, Y, Xs, ls = _problem(kind, n, N)
    g = gpn.GPRegression(X, Y, getattr(gpn, kind)(2, 1.7, ls, ARD=True), noise_var=NOISE)
    mean, cov = joint_posterior(g, Xs)
    assert mean.shape == (N, 1) and cov.shape == (N, N)
    assert np.max(np.abs(cov - joint_posterior_woodbury(g, Xs))) / 1.7 < 1e-10
    m1, v1 = g.predict_noiseless(Xs)
    assert np.max(np.abs(mean - m1)) <= 1e-12 * max(1.0, np.max(np.abs(m1)))
    big = v1[:, 0] > 1e-15
    assert np.max(np.abs(np.diag(cov)[big] - v1[big, 0])) / 1.7 < 1e-10


@pytest.mark.parametrize("kind", ["RBF", "Matern32", "Matern52"])
def test_covariance_matches_sklearn(kind):
    skgp = pytest.importorskip("sklearn.gaussian_process")
    from sklearn.gaussian_process import kernels as skk
    X, Y, Xs, ls = _problem(kind, 70, 120)
    var = 1.7
    g = gpn.GPRegression(X, Y, getattr(gpn, kind)(2, var, ls, ARD=True), noise_var=NOISE)
    sk = (skk.RBF(ls, "fixed") if kind == "RBF" else
          skk.Matern(ls, "fixed", nu=1.5 if kind == "Matern32" else 2.5))
    gpr = skgp.GaussianProcessRegressor(skk.ConstantKernel(var, "fixed") * sk,
                                        alpha=NOISE + 1e-8, optimizer=None).fit(X, Y)
    mu, cov_sk = gpr.predict(Xs, return_cov=True)
    mean, cov = joint_posterior(g, Xs)
    np.testing.assert_allclose(mean.ravel(), mu.ravel(), rtol=1e-8, atol=1e-10)
    assert np.max(np.abs(cov - cov_sk)) / var < 1e-8


@pytest.mark.parametrize("name", ["sgp_gp_predict_cov", "sgp_gp_posterior_draw"])
def test_abi_declares_and_exports_the_joint_calls(name):
    header = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared"
    assert re.search(r"#define\s+SGP_MAX_JOINT\s+8192\b", header)
    from safeopt_amd import _hip
    assert name in _hip.PROTOTYPES
    assert _hip.MAX_JOINT == 8192
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, name), name + " is not exported by the library"
