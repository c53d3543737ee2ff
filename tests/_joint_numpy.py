"""Joint posterior of a set of points from an ``oracle.gp_numpy.GPRegression`` -- the reference
of tests/test_joint_host.py and tests/test_gpu_joint.py (the oracle itself has no ``full_cov``).
Only the oracle's public attributes are used: ``X``, ``kern``, ``L``, ``woodbury_inv``,
``woodbury_vector``."""
import numpy as np
from scipy.linalg import solve_triangular


def joint_posterior(g, Xs):
    """``(mean (N, 1), cov (N, N))`` through the whitened cross-covariance V = L^-1 k(X, X*)."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=float))
    k = g.kern
    V = solve_triangular(g.L, k.K(g.X, Xs), lower=True)
    cov = k.K(Xs) - V.T.dot(V)
    mean = k.K(Xs, g.X).dot(g.woodbury_vector)
    return mean, cov


def joint_posterior_woodbury(g, Xs):
    """The same covariance in GPy's own form, k(X*, X*) - Kx^T Ky^-1 Kx."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=float))
    k = g.kern
    Kx = k.K(g.X, Xs)
    return k.K(Xs) - Kx.T.dot(g.woodbury_inv).dot(Kx)
