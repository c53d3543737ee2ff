"""Leave-one-out references in the device descriptor's layout (NumPy only).

``brute_*``: the independent one, in ``np.longdouble``: delete row ``i``, refit
``Ky = K + (noise + 1e-8) I`` on the rest, predict the noisy ``y_i``.  Nothing of the closed
form enters it (its own covariance code, its own Cholesky factorisation).

``loo`` / ``loo_lml``: the closed form in float64 (Rasmussen & Williams 5.4.2) with the
analytic gradient of the log pseudo-likelihood, the specification of ``sgp_gp_loo`` /
``sgp_gp_loo_lml``:

    P_ii = (Ky^-1)_ii,  mu_-i = y_i - alpha_i / P_ii,  var_-i = 1 / P_ii,  z_i = alpha_i / sqrt(P_ii)
    L_LOO = sum_i [-1/2 log var_-i - 1/2 z_i^2 - 1/2 log 2 pi]
    dL_LOO/dtheta = sum_ij G_ij dKy_ij/dtheta,   G = 1/2 (u alpha^T + alpha u^T) - C^T C,
    a_i = alpha_i / P_ii,  b_i = 1/2 (1 + alpha_i^2 / P_ii) / P_ii,  u = Ky^-1 a,
    C = diag(sqrt(b)) Ky^-1
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

import _hyper_numpy as hn

LD = np.longdouble
LOG_2PI_LD = np.log(2 * np.arccos(LD(-1)))


# ---- brute force, long double ---------------------------------------------------------------
def _cov_ld(kinds, X1, X2, variances, inv_ls):
    X1, X2 = np.asarray(X1, LD), np.asarray(X2, LD)
    variances, inv_ls = np.asarray(variances, LD), np.asarray(inv_ls, LD)
    K = np.ones((len(X1), len(X2)), LD) * np.prod(variances)
    for p, kind in enumerate(kinds):
        r2 = sum(((X1[:, None, a] - X2[None, :, a]) * inv_ls[p, a]) ** 2
                 for a in range(X1.shape[1]))
        if kind == hn.RBF:
            K = K * np.exp(-r2 / 2)
            continue
        r = np.sqrt(r2)
        if kind == hn.MATERN32:
            s = np.sqrt(LD(3)) * r
            K = K * (1 + s) * np.exp(-s)
        else:
            s = np.sqrt(LD(5)) * r
            K = K * (1 + s + LD(5) / 3 * r2) * np.exp(-s)
    return K


def _chol_ld(A):
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not piv > 0:
            raise np.linalg.LinAlgError("pivot %d" % (j + 1))
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _fwd_ld(L, B):
    """L^-1 B for the columns of B"""
    T = np.array(B, LD)
    for j in range(len(L)):
        T[j] = (T[j] - L[j, :j] @ T[:j]) / L[j, j]
    return T


def brute_loo(kinds, X, y, variances, inv_ls, noise_var):
    """(mean[n], var[n]) of the noisy y_i predicted from all other rows, long double."""
    X = np.asarray(X, LD)
    y = np.asarray(y, LD).reshape(-1)
    n = len(X)
    add = LD(noise_var) + LD(1e-8)
    K = _cov_ld(kinds, X, X, variances, inv_ls)
    mean, var = np.zeros(n, LD), np.zeros(n, LD)
    for i in range(n):
        keep = np.arange(n) != i
        prior = K[i, i] + add
        if n == 1:
            mean[i], var[i] = 0, prior
            continue
        L = _chol_ld(K[np.ix_(keep, keep)] + add * np.eye(n - 1, dtype=LD))
        T = _fwd_ld(L, np.column_stack([K[keep, i], y[keep]]))
        mean[i] = T[:, 0] @ T[:, 1]
        var[i] = prior - T[:, 0] @ T[:, 0]
    return mean, var


def brute_residuals(kinds, X, y, variances, inv_ls, noise_var):
    mean, var = brute_loo(kinds, X, y, variances, inv_ls, noise_var)
    return (np.asarray(y, LD).reshape(-1) - mean) / np.sqrt(var)


def brute_pseudo_likelihood(kinds, X, y, variances, inv_ls, noise_var):
    mean, var = brute_loo(kinds, X, y, variances, inv_ls, noise_var)
    z2 = (np.asarray(y, LD).reshape(-1) - mean) ** 2 / var
    return np.sum(-np.log(var) / 2 - z2 / 2 - LOG_2PI_LD / 2)


# ---- closed form, float64 -------------------------------------------------------------------
def _closed(kinds, X, y, variances, inv_ls, noise_var):
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float).reshape(-1)
    n = len(X)
    K, d2, fs, cs = hn.cov(kinds, X, np.asarray(variances, float), np.asarray(inv_ls, float))
    c = cho_factor(K + (noise_var + 1e-8) * np.eye(n), lower=True)
    Kinv = cho_solve(c, np.eye(n))
    alpha = cho_solve(c, y)
    return y, K, d2, fs, cs, c, Kinv, alpha, np.diag(Kinv).copy()


def loo(kinds, X, y, variances, inv_ls, noise_var):
    """(mean[n], var[n], z[n], L_LOO)"""
    y, _, _, _, _, _, _, alpha, P = _closed(kinds, X, y, variances, inv_ls, noise_var)
    z = alpha / np.sqrt(P)
    L = np.sum(0.5 * np.log(P) - 0.5 * alpha ** 2 / P - 0.5 * np.log(2 * np.pi))
    return y - alpha / P, 1.0 / P, z, float(L)


def loo_lml(kinds, X, y, variances, inv_ls, noise_var):
    """(L_LOO, d/d noise, d/d variances[P], d/d inv_ls[P, d], info) like ``hn.lml``."""
    variances = np.asarray(variances, dtype=float)
    inv_ls = np.asarray(inv_ls, dtype=float)
    Pn, d = len(kinds), np.asarray(X).shape[1]
    try:
        y, K, d2, fs, cs, c, Kinv, alpha, P = _closed(kinds, X, y, variances, inv_ls, noise_var)
    except np.linalg.LinAlgError:
        return np.nan, np.nan, np.full(Pn, np.nan), np.full((Pn, d), np.nan), 1
    if not (np.all(P > 0) and np.all(np.isfinite(P))):
        return np.nan, np.nan, np.full(Pn, np.nan), np.full((Pn, d), np.nan), 1
    z2 = alpha ** 2 / P
    L = np.sum(0.5 * np.log(P) - 0.5 * z2 - 0.5 * np.log(2 * np.pi))
    a = alpha / P
    b = 0.5 * (1.0 + z2) / P
    u = cho_solve(c, a)
    C = np.sqrt(b)[:, None] * Kinv
    G = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - C.T @ C
    g_noise = np.trace(G)
    g_var = np.sum(G * K) / variances
    g_ils = np.zeros((Pn, d))
    for p in range(Pn):
        others = np.prod(variances) * np.prod([fs[o] for o in range(Pn) if o != p], axis=0) \
            if Pn > 1 else np.prod(variances)
        H = G * others * cs[p]
        for k in range(d):
            g_ils[p, k] = np.sum(H * d2[k]) * inv_ls[p, k]
    return float(L), float(g_noise), g_var, g_ils, 0


def evaluator(kern, X, y, d=None):
    """``evaluate(variances, inv_ls, noise_var)`` of the data for a safeopt_amd.gpy kernel."""
    kinds = list(kern._desc(d if d is not None else np.asarray(X).shape[1])[1])
    return lambda variances, inv_ls, noise_var: loo_lml(kinds, X, y, variances, inv_ls,
                                                        noise_var)
