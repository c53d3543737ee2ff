"""Max-value entropy search on the host: the float64 restatement of csrc/mes.hip's stable form
(SciPy ``erfcx``) and a 50-digit ``mpmath`` evaluation of the definition.

    sigma = sqrt(max(v, 1e-15)),  y_k = max(y*_k, m),  gamma_k = (y_k - mu) / sigma
    alpha = (1 / K) sum_k term(gamma_k)  (added in the order of k)
    term(g) = g phi(g) / (2 Phi(g)) - ln Phi(g)

The unit of every comparison is ``EPS * (1 + g^2 / 2)``: for very negative ``g`` the two parts
of ``term`` cancel from size ``g^2 / 2`` down to ``ln(-g sqrt(2 pi))``.
"""
import numpy as np

EPS = 2.2e-16
SQRT1_2 = 0.70710678118654752440
SQRT_2_OVER_PI = 0.79788456080286535588
SQRT_2PI = 2.50662827463100050242


def term(g):
    """The stable form, operation for operation what ``mes_term`` does on the device."""
    from scipy.special import erfcx
    g = np.asarray(g, dtype=np.float64)
    t = np.abs(g) * SQRT1_2
    e = erfcx(t)
    neg = g < 0.0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        x = np.exp(-(t * t))
        q = 0.5 * e * x
        r = np.where(neg, SQRT_2_OVER_PI / e, x / SQRT_2PI / (1.0 - q))
        lnp = np.where(neg, np.log(0.5 * e) - t * t, np.log1p(-q))
        gr = np.where((x > 0.0) | neg, g * r, 0.0)
    return 0.5 * gr - lnp


def alpha(mean, var, ystar, floor=-np.inf):
    """alpha per row, the terms added in the order of k."""
    mean = np.asarray(mean, dtype=np.float64)
    sigma = np.sqrt(np.maximum(np.asarray(var, dtype=np.float64), 1e-15))
    ys = np.maximum(np.asarray(ystar, dtype=np.float64).reshape(-1), floor)
    acc = np.zeros(mean.shape)
    for y in ys:
        acc = acc + term((y - mean) / sigma)
    return acc / float(ys.size)


def term_mp(g):
    """``term`` at the doubles ``g`` from the definition in 50 digits -> float64 array and the
    mpmath values themselves (for differences below one ulp)."""
    import mpmath as mp
    out = []
    with mp.workdps(50):
        for v in np.asarray(g, dtype=np.float64).ravel():
            gg = mp.mpf(float(v))
            Phi = mp.erfc(-gg / mp.sqrt(2)) / 2
            phi = mp.exp(-gg * gg / 2) / mp.sqrt(2 * mp.pi)
            out.append(gg * phi / (2 * Phi) - mp.log(Phi))
    return out


def units(got, g, exact):
    """|got - exact| in units of EPS (1 + g^2 / 2), per point; ``exact`` from ``term_mp``."""
    import mpmath as mp
    got = np.asarray(got, dtype=np.float64).ravel()
    g = np.asarray(g, dtype=np.float64).ravel()
    with mp.workdps(50):
        return np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(got, exact)]) / (
            EPS * (1.0 + 0.5 * g * g))


def gamma_set():
    """3201 equally spaced points over [-40, 40] and 2000 draws of N(0, 3^2)."""
    rng = np.random.default_rng(20171)
    return np.concatenate([np.linspace(-40.0, 40.0, 3201), 3.0 * rng.standard_normal(2000)])
