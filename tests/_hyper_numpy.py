"""NumPy marginal likelihood with analytic gradient in the device descriptor's layout: the
stand-in the CPU tests pass to ``safeopt_amd.hyper`` and the reference of the product-kernel
cases on the GPU (pinned to scikit-learn on single kernels there, to central differences
and the oracle's kernels in tests/test_hyper_host.py)."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

RBF, MATERN32, MATERN52 = 0, 1, 2


def _part(kind, r2):
    """f(r) and c(r) with df/ds_a = c(r) D_a^2 s_a"""
    if kind == RBF:
        f = np.exp(-0.5 * r2)
        return f, -f
    r = np.sqrt(r2)
    if kind == MATERN32:
        e = np.exp(-np.sqrt(3.) * r)
        return (1. + np.sqrt(3.) * r) * e, -3. * e
    e = np.exp(-np.sqrt(5.) * r)
    return (1. + np.sqrt(5.) * r + 5. / 3. * r2) * e, -5. / 3. * (1. + np.sqrt(5.) * r) * e


def cov(kinds, X, variances, inv_ls):
    d2 = [(X[:, None, a] - X[None, :, a]) ** 2 for a in range(X.shape[1])]
    fs, cs = [], []
    for p, kind in enumerate(kinds):
        r2 = sum(d2[a] * inv_ls[p, a] ** 2 for a in range(X.shape[1]))
        f, c = _part(kind, r2)
        fs.append(f)
        cs.append(c)
    K = np.prod(variances) * np.prod(fs, axis=0)
    return K, d2, fs, cs


def lml(kinds, X, y, variances, inv_ls, noise_var):
    """(log p, d/d noise, d/d variances[P], d/d inv_ls[P, d], info) -- info = 1 when Ky is
    not positive definite."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float).reshape(-1)
    variances = np.asarray(variances, dtype=float)
    inv_ls = np.asarray(inv_ls, dtype=float)
    n, P, d = len(X), len(kinds), X.shape[1]
    K, d2, fs, cs = cov(kinds, X, variances, inv_ls)
    Ky = K + (noise_var + 1e-8) * np.eye(n)
    try:
        c = cho_factor(Ky, lower=True)
    except np.linalg.LinAlgError:
        return np.nan, np.nan, np.full(P, np.nan), np.full((P, d), np.nan), 1
    alpha = cho_solve(c, y)
    ll = -0.5 * y @ alpha - np.log(np.diag(c[0])).sum() - 0.5 * n * np.log(2 * np.pi)
    W = np.outer(alpha, alpha) - cho_solve(c, np.eye(n))
    g_noise = 0.5 * np.trace(W)
    g_var = 0.5 * np.sum(W * K) / variances
    g_ils = np.zeros((P, d))
    for p in range(P):
        others = np.prod(variances) * np.prod([fs[o] for o in range(P) if o != p], axis=0) \
            if P > 1 else np.prod(variances)
        H = W * others * cs[p]
        for a in range(d):
            g_ils[p, a] = 0.5 * np.sum(H * d2[a]) * inv_ls[p, a]
    return float(ll), float(g_noise), g_var, g_ils, 0


def evaluator(kern, X, y, d=None):
    """``evaluate(variances, inv_ls, noise_var)`` of the data for a safeopt_amd.gpy kernel."""
    kinds = list(kern._desc(d if d is not None else np.asarray(X).shape[1])[1])
    return lambda variances, inv_ls, noise_var: lml(kinds, X, y, variances, inv_ls, noise_var)


def draw_gp(kinds, X, variances, inv_ls, noise_var, seed):
    """A sample path of the GP at X plus noise, (n, 1)."""
    rng = np.random.default_rng(seed)
    K = cov(kinds, X, np.asarray(variances, float), np.asarray(inv_ls, float))[0]
    L = np.linalg.cholesky(K + 1e-10 * np.eye(len(X)))
    return (L @ rng.normal(size=len(X)) + np.sqrt(noise_var) * rng.normal(size=len(X)))[:, None]
