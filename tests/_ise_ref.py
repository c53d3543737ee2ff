"""The yardsticks of the information-theoretic safe exploration tests (tests/test_ise_cpu.py,
tests/test_gpu_ise.py): the float64 restatement of the device's stable form (csrc/ise_term.h),
the closed form of Bottero et al. 2022 in mpmath at 80 digits, pairs / alpha / pick from the
long-double GP of tests/_incremental_ref.py, and the candidate selection of ``ise_point``.

The unit of a term's error:  ``u = EPS (1 + t) sqrt(kappa) ln2 e^-t``,  ``kappa = (s + vx) /
(s + vx (1 - r2))``.  ``ln2 e^-t`` is the scale of the term, ``1 + t`` the amplification of a
rounding error of ``t`` in ``e^-t``, and ``sqrt(kappa)`` that of the rounding of ``r2`` in
``1 - r2`` (the term is ``ln2 e^-t (1 - sqrt(A / B) ...)`` with ``A = s + vx (1 - r2)``: inherent
in the inputs, not in the form).
"""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
C1 = 1.0 / (np.pi * np.log(2.0))
LN2 = np.log(2.0)
VMIN = 1e-15


def term(mu, vz, vx, c, s):
    """The stable form in float64, operation by operation as csrc/ise_term.h has it."""
    mu, vz, vx, c = (np.asarray(a, dtype=np.float64) for a in (mu, vz, vx, c))
    with np.errstate(all='ignore'):
        vz = np.maximum(vz, VMIN)
        vx = np.maximum(vx, VMIN)
        t = C1 * (mu * mu) / vz
        r2 = np.minimum((c * c) / (vx * vz), 1.0)
        q = r2 * vx
        B = (s + vx) + (2.0 * C1 - 1.0) * q
        e = q / B
        w = np.minimum(2.0 * C1 * e, 1.0)
        return -LN2 * np.exp(-t) * np.expm1(0.5 * np.log1p(-w) - t * ((1.0 - 2.0 * C1) * e))


def naive(mu, vz, vx, c, s):
    """The closed form as the paper writes it, in float64: a difference of nearly equal numbers
    for small r2."""
    vz, vx = np.maximum(vz, VMIN), np.maximum(vx, VMIN)
    t = C1 * mu * mu / vz
    r2 = np.minimum(c * c / (vx * vz), 1.0)
    A = s + vx * (1.0 - r2)
    B = s + vx + (2.0 * C1 - 1.0) * r2 * vx
    return LN2 * (np.exp(-t) - np.sqrt(A / B) * np.exp(-t * (s + vx) / B))


def _mp():
    import mpmath
    mpmath.mp.dps = 80
    return mpmath


def term_mp(mu, vz, vx, c, s):
    """``(I, u)`` per point: ln2 [e^-t - sqrt(A / B) e^(-t (s + vx) / B)] at 80 digits from the
    float64 inputs as they are (variances clipped at 1e-15, r2 at 1), rounded to float64, and
    the unit ``u`` of its error (module docstring)."""
    mp = _mp()
    mu, vz, vx, c, s = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64)
                                             for a in (mu, vz, vx, c, s)))
    out, unit = np.empty(mu.shape), np.empty(mu.shape)
    c1 = 1 / (mp.pi * mp.log(2))
    ln2 = mp.log(2)
    for i in np.ndindex(mu.shape):
        m, z, x, cc, ss = (mp.mpf(float(a[i])) for a in (mu, vz, vx, c, s))
        z, x = max(z, mp.mpf(VMIN)), max(x, mp.mpf(VMIN))
        t = c1 * m * m / z
        r2 = min(cc * cc / (x * z), mp.mpf(1))
        A = ss + x * (1 - r2)
        B = ss + x + (2 * c1 - 1) * r2 * x
        val = ln2 * (mp.exp(-t) - mp.sqrt(A / B) * mp.exp(-t * (ss + x) / B))
        out[i] = float(val)
        kappa = (ss + x) / A if A > 0 else mp.inf
        unit[i] = float(EPS * (1 + t) * mp.sqrt(kappa) * ln2 * mp.exp(-t))
    return out, unit


def units(got, exact, unit):
    """|got - exact| in the points' units (0 where the unit is infinite)."""
    with np.errstate(all='ignore'):
        return np.where(np.isfinite(unit), np.abs(got - exact) / unit, 0.0)


@functools.lru_cache(maxsize=None)
def point_set(n=6000, seed=2022):
    """``(mu, vz, vx, c, s)``: t in [0, 650], variances in [1e-12, 1e3], s / vx in [1e-12, 10],
    1 - |rho| down to 1e-12, both signs of mu and of c."""
    rng = np.random.default_rng(seed)
    vz = 10.0 ** rng.uniform(-12, 3, n)
    vx = 10.0 ** rng.uniform(-12, 3, n)
    t = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 650.0, n), 10.0 ** rng.uniform(-6, 1, n))
    t[:40] = 0.0
    mu = np.sqrt(t * vz / C1) * rng.choice([-1.0, 1.0], n)
    rho = np.where(rng.random(n) < 0.5, 1.0 - 10.0 ** rng.uniform(-12, 0, n),
                   10.0 ** rng.uniform(-8, 0, n))
    rho = np.minimum(rho, 1.0) * rng.choice([-1.0, 1.0], n)
    c = rho * np.sqrt(vx * vz)
    s = vx * 10.0 ** rng.uniform(-12, 1, n)
    return mu, vz, vx, c, s


@functools.lru_cache(maxsize=None)
def point_reference():
    """``(exact, unit, the restatement's error in units)`` on ``point_set()``, once."""
    p = point_set()
    exact, unit = term_mp(*p)
    return exact, unit, units(term(*p), exact, unit)


# ---- pairs, alpha and the pick from a long-double GP -------------------------------------------

def ref_cov(gp, Z, Xc):
    """Posterior covariance (rows of ``Z``) x (rows of ``Xc``) of a ``RefGP``, long double:
    ``kern(z, x) - kern(z, X) solve(kern(X, x))``."""
    from _incremental_ref import kern
    kz = kern(gp.spec, gp.X, Z)                      # (n, N)
    kx = kern(gp.spec, gp.X, Xc)                     # (n, K)
    W = np.stack([gp.solve(kx[:, j]) for j in range(kx.shape[1])], axis=1)
    return kern(gp.spec, Z, Xc) - kz.T @ W           # (N, K)


def pairs(mean, var, fmin, cov, s, cand):
    """``(K, N)``: the in-order sum over the active GPs of ``term``; ``mean`` / ``var`` ``(G,
    N)``, ``cov`` ``(G, K, N)``, ``s`` ``(G,)``, ``cand`` ``(K,)`` rows."""
    out = np.zeros(cov.shape[1:])
    for g in range(len(fmin)):
        if np.isfinite(fmin[g]):
            out = out + term((mean[g] - fmin[g])[None, :], var[g][None, :],
                             var[g][cand][:, None], cov[g], s[g])
    return out


def alpha(pr, zmask):
    """``(alpha (K,), target (K,))`` of pairs ``(K, N)`` over the rows of ``zmask``: the
    maximum and the lowest row attaining it; -inf / -1 without a row."""
    if not zmask.any():
        return np.full(pr.shape[0], -np.inf), np.full(pr.shape[0], -1, dtype=np.int64)
    masked = np.where(zmask[None, :], pr, -np.inf)
    tg = np.argmax(masked, axis=1)                   # (the first maximum)
    return masked[np.arange(pr.shape[0]), tg], tg.astype(np.int64)


def pick(al, tg, cand):
    """``(value, row)``: the candidate with the largest alpha, the lowest row among equals;
    -inf / -1 when no candidate has a target."""
    ok = np.flatnonzero(tg >= 0)
    if ok.size == 0:
        return -np.inf, -1
    best = al[ok].max()
    return float(best), int(np.min(np.asarray(cand)[ok][al[ok] == best]))


def select(var, S, s, active, K):
    """The candidate rows of ``ise_point`` for an int ``K``, by a sort of (key, row) tuples:
    the largest ``sum_{g active} log1p(var_g / s_g) / 2`` first, the lower row among equals."""
    ids = [int(i) for i in np.flatnonzero(S)]
    key = {}
    for i in ids:
        k = 0.0
        for g in range(len(s)):
            if active[g]:
                k = k + 0.5 * np.log1p(var[g, i] / s[g])
        key[i] = k
    return np.array(sorted(ids, key=lambda i: (-key[i], i))[:K], dtype=np.int64)
