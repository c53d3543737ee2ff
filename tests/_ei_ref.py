"""Log expected improvement on the host: the float64 restatement of csrc/ei_term.h's stable
forms (SciPy ``erfcx`` / ``erfc``), operation for operation, and a 50-digit ``mpmath``
evaluation of the definitions.

    ln Phi(z)                                   (``log_ndtr``)
    ln h(z),  h(z) = phi(z) + z Phi(z)          (``log_h``)
    z = (mean_0 - tau - xi) / sigma_0,  sigma_g = sqrt(max(var_g, 1e-15))
    EI: alpha = ln(max(var_0, 1e-15)) / 2 + ln h(z)      PI: alpha = ln Phi(z)
    alpha += ln Phi((mean_g - fmin_g) / sigma_g)  for every g with a finite fmin_g, in order

The unit of every comparison is ``EPS * (1 + z^2 / 2)``: for very negative ``z`` both logarithms
are ``-z^2 / 2`` to leading order.
"""
import numpy as np

EPS = 2.2e-16
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
HALF_LN_2PI = 0.91893853320467274178
SQRT_PI = 1.77245385090551602730
Z_DIRECT, Z_ASYMPT = -1.0, -1.0e6          # the branch points of ei_log_h
EI, PI = 0, 1


def log_ndtr(z):
    """``ei_log_ndtr``, operation for operation."""
    from scipy.special import erfcx
    z = np.asarray(z, dtype=np.float64)
    t = np.abs(z) * SQRT1_2
    e = erfcx(t)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        neg = np.log(0.5 * e) - t * t
        pos = np.log1p(-(0.5 * e * np.exp(-(t * t))))
    return np.where(z < 0.0, neg, pos)


def log_h(z):
    """``ei_log_h``, operation for operation."""
    from scipy.special import erfc, erfcx
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore', under='ignore'):
        phi = np.exp(-0.5 * (z * z)) * INV_SQRT_2PI
        Phi = 0.5 * erfc(-z * SQRT1_2)
        direct = np.log(phi + z * Phi)
        tail = -0.5 * (z * z) - HALF_LN_2PI
        asym = tail - 2.0 * np.log(-z)
        t = -z * SQRT1_2
        mid = np.log(1.0 - SQRT_PI * t * erfcx(t)) + tail
    return np.where(z >= Z_DIRECT, direct, np.where(z < Z_ASYMPT, asym, mid))


def alpha(mean, var, tau, xi=0.0, kind=EI, fmin=None):
    """alpha per row from ``mean`` / ``var`` ``(G, N)`` (or ``(N,)``: the objective alone)."""
    mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
    var = np.maximum(np.atleast_2d(np.asarray(var, dtype=np.float64)), 1e-15)
    z = (mean[0] - tau - xi) / np.sqrt(var[0])
    a = 0.5 * np.log(var[0]) + log_h(z) if kind == EI else log_ndtr(z)
    if fmin is not None:
        for g, f in enumerate(np.asarray(fmin, dtype=np.float64).reshape(-1)):
            if np.isfinite(f):
                a = a + log_ndtr((mean[g] - f) / np.sqrt(var[g]))
    return a


def _mp(z, fn):
    import mpmath as mp
    out = []
    with mp.workdps(50):
        for v in np.asarray(z, dtype=np.float64).ravel():
            out.append(fn(mp, mp.mpf(float(v))))
    return out


def log_ndtr_mp(z):
    """``ln Phi`` at the doubles ``z`` from the definition in 50 digits (mpmath values)."""
    return _mp(z, lambda mp, x: mp.log(mp.erfc(-x / mp.sqrt(2)) / 2))


def log_h_mp(z):
    """``ln(phi + z Phi)`` likewise.  The sum cancels to ``phi / z^2`` for very negative ``z``:
    18 of the 50 digits go at z = -1e9, the far end of the point set (against the expansion
    -z^2 / 2 - ln(2 pi) / 2 - 2 ln|z| - 3 / z^2 the values agree to 2e-15 there and to 1e-23 at
    z = -1e6; a unit is 110 and 1.1e-4)."""
    return _mp(z, lambda mp, x: mp.log(mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi) +
                                       x * mp.erfc(-x / mp.sqrt(2)) / 2))


def units(got, z, exact):
    """|got - exact| in units of EPS (1 + z^2 / 2), per point; ``exact``: mpmath values."""
    import mpmath as mp
    got = np.asarray(got, dtype=np.float64).ravel()
    z = np.asarray(z, dtype=np.float64).ravel()
    with mp.workdps(50):
        return np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(got, exact)]) / (
            EPS * (1.0 + 0.5 * z * z))


def point_set():
    """3201 equally spaced points over [-40, 40], 2000 draws of N(0, 3^2), -logspace(0, 9, 400),
    +logspace(0, 9, 100), both zeros and both branch points of ``log_h``."""
    rng = np.random.default_rng(20171)
    return np.concatenate([np.linspace(-40.0, 40.0, 3201), 3.0 * rng.standard_normal(2000),
                           -np.logspace(0.0, 9.0, 400), np.logspace(0.0, 9.0, 100),
                           [0.0, -0.0, Z_DIRECT, Z_ASYMPT]])


_CACHE = {}


def reference():
    """``(z, exact log_h, exact log_ndtr, units of the restatement's log_h, ... of its
    log_ndtr)`` over ``point_set()``, computed once per process."""
    if not _CACHE:
        z = point_set()
        eh, en = log_h_mp(z), log_ndtr_mp(z)
        _CACHE["r"] = (z, eh, en, units(log_h(z), z, eh), units(log_ndtr(z), z, en))
    return _CACHE["r"]
