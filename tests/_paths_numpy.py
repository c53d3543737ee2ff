"""Posterior sample paths by pathwise conditioning, stated in NumPy -- the reference of
tests/test_paths_cpu.py and tests/test_gpu_paths.py (same standing as tests/_joint_numpy.py).

    phi_i(x)   = sqrt(2 v / m) cos(omega_i . x + b_i)          i = 1 .. m,  v = prod_p v_p
    V[:, s]    = alpha - Ky^-1 (Phi(X) W[:, s] + E[:, s])      Ky = K + (noise_var + 1e-8) I
    f_s(x)     = sum_i W[i, s] phi_i(x) + sum_j k(x, X_j) V[j, s]

The kernel is given as the C ABI gives it: ``kern = (kinds, variances, inv_ls (P, d))``,
k = prod_p v_p f_p(r_p), r_p^2 = sum_a ((x_a - x'_a) inv_ls[p, a])^2.  Every function takes a
``dtype``: float64, or ``np.longdouble`` for the discrepancy the tolerances are built from (the
Cholesky factorisation is then a plain column loop -- LAPACK has no long double).
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

RBF, MATERN32, MATERN52 = 0, 1, 2


def kernel_matrix(kern, X1, X2, dtype=np.float64):
    kinds, variances, inv_ls = kern
    X1 = np.asarray(X1, dtype=dtype)
    X2 = np.asarray(X2, dtype=dtype)
    inv_ls = np.asarray(inv_ls, dtype=dtype).reshape(len(kinds), X1.shape[1])
    out = np.ones((X1.shape[0], X2.shape[0]), dtype=dtype)
    for p, kind in enumerate(kinds):
        diff = (X1[:, None, :] - X2[None, :, :]) * inv_ls[p]
        r2 = (diff * diff).sum(-1)
        if kind == RBF:
            f = np.exp(-r2 / dtype(2))
        else:
            r = np.sqrt(r2)
            if kind == MATERN32:
                a = np.sqrt(dtype(3)) * r
                f = (1 + a) * np.exp(-a)
            else:
                a = np.sqrt(dtype(5)) * r
                f = (1 + a + dtype(5) / dtype(3) * r2) * np.exp(-a)
        out = out * (dtype(variances[p]) * f)
    return out


def prior_variance(kern):
    return float(np.prod(np.asarray(kern[1], dtype=float)))


def feature_args(Omega, phase, X, dtype=np.float64):
    """omega_i . x + b_i, (N, m)"""
    return np.asarray(X, dtype=dtype).dot(np.asarray(Omega, dtype=dtype).T) + \
        np.asarray(phase, dtype=dtype)[None, :]


def features(kern, Omega, phase, X, dtype=np.float64):
    """Phi (N, m)"""
    m = Omega.shape[0]
    amp = np.sqrt(dtype(2) * dtype(prior_variance(kern)) / dtype(m))
    return amp * np.cos(feature_args(Omega, phase, X, dtype))


def _cholesky_solve(A, B, dtype):
    if dtype == np.float64:
        return cho_solve(cho_factor(A, lower=True), B)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] * L[j, :j]).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    Y = np.array(B, dtype=dtype)
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j].dot(Y[:j])) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j].dot(Y[j + 1:])) / L[j, j]
    return Y


def gram(kern, noise_var, X, dtype=np.float64):
    """Ky = K + (noise_var + 1e-8) I"""
    X = np.asarray(X, dtype=dtype)
    return kernel_matrix(kern, X, X, dtype) + \
        (dtype(noise_var) + dtype(1e-8)) * np.eye(X.shape[0], dtype=dtype)


def weight_rhs(kern, X, y, Omega, phase, W, E, dtype=np.float64):
    """y 1^T - Phi(X) W - E, (n, S): V = Ky^-1 of it"""
    Phi = features(kern, Omega, phase, X, dtype)
    return np.asarray(y, dtype=dtype).reshape(-1, 1) - Phi.dot(np.asarray(W, dtype=dtype)) - \
        np.asarray(E, dtype=dtype)


def path_weights(kern, noise_var, X, y, Omega, phase, W, E, dtype=np.float64):
    """V (n, S) = alpha - Ky^-1 (Phi(X) W + E) through Cholesky solves."""
    return _cholesky_solve(gram(kern, noise_var, X, dtype),
                           weight_rhs(kern, X, y, Omega, phase, W, E, dtype), dtype)


def paths_eval(kern, X, Omega, phase, W, V, Xnew, dtype=np.float64):
    """f (N, S) at the rows of Xnew."""
    Phi = features(kern, Omega, phase, Xnew, dtype)
    Kx = kernel_matrix(kern, Xnew, X, dtype)
    return Phi.dot(np.asarray(W, dtype=dtype)) + Kx.dot(np.asarray(V, dtype=dtype))


def path_weights_ld(*a):
    return path_weights(*a, dtype=np.longdouble)


def paths_eval_ld(*a):
    return paths_eval(*a, dtype=np.longdouble)


def abs_budget(kern, X, Omega, phase, W, V, Xnew):
    """sum_i |W[i, s]| amplitude + sum_j |k(x, X_j) V[j, s]| per (row, path): the sum of the
    absolute terms of f_s(x), the scale of its rounding error."""
    m = Omega.shape[0]
    amp = np.sqrt(2.0 * prior_variance(kern) / m)
    Kx = kernel_matrix(kern, Xnew, X)
    return amp * np.abs(W).sum(0)[None, :] + np.abs(Kx).dot(np.abs(V))


def weights_residual(Ky, V, rhs):
    """|Ky V - rhs|_inf / (|Ky|_inf |V|_inf + |rhs|_inf): the backward error of V as the
    solution of Ky V = rhs, free of cond(Ky).  (inf-norms: largest absolute row sum)"""
    norm = lambda A: np.abs(A).sum(1).max()
    return norm(Ky.dot(V) - rhs) / (norm(Ky) * norm(V) + norm(rhs))
