"""Random numbers and the record of posterior sample paths (pathwise conditioning).

NumPy only: the draws are made on the host, as ``posterior_samples_f`` takes its normals
there; the device evaluates (``csrc/paths.hip``).  A path is

    phi_i(x)   = sqrt(2 v / m) cos(omega_i . x + b_i)          i = 1 .. m,  v = prod_p v_p
    V[:, s]    = alpha - Ky^-1 (Phi(X) W[:, s] + E[:, s])
    f_s(x)     = sum_i W[i, s] phi_i(x) + sum_j k(x, X_j) V[j, s]

(Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors").

Order of the draws -- a seed pins a path:

1. for every kernel part ``p`` in order: ``z = standard_normal((m, d))``, then, for a Matern
   part only, ``u = chisquare(2 nu, m)`` (``2 nu`` = 3 / 5); the part's frequencies are
   ``inv_ls[p] * z / sqrt(u / (2 nu))`` (RBF: the divisor is 1) -- zero on the columns the
   part does not use -- and ``Omega`` is the sum over the parts: the spectral measure of a
   product of kernels is the convolution of the parts' measures;
2. ``b = 2 pi random(m)``;
3. ``W = standard_normal((m, size))``;
4. ``E = sqrt(noise_var + 1e-8) standard_normal((n, size))``, row ``i`` times
   ``sqrt(noise_scale[i])`` for a GP with per-observation noise scales.
"""
from __future__ import annotations

import numpy as np

RBF, MATERN32, MATERN52 = 0, 1, 2          # SGP_RBF / SGP_MATERN32 / SGP_MATERN52
#: degrees of freedom 2 nu of the chi-square mixing variable (None: none, the measure is normal)
SPECTRAL_DOF = {RBF: None, MATERN32: 3, MATERN52: 5}


def draw_path_inputs(kern_parts, noise_var, n, d, size, features, rng=np.random, dof=None,
                     noise_scale=None):
    """``(Omega (m, d), b (m), W (m, size), E (n, size))`` for ``size`` paths of ``m =
    features`` random Fourier features each, in the order the module documents.

    ``kern_parts = (kinds, inv_ls)``: the kinds of the kernel's parts and their inverse
    lengthscales ``(P, d)``, zero on the columns a part does not use -- ``kinds`` and
    ``inv_ls`` of the C ABI.  ``rng``: ``np.random`` (the global generator), a ``RandomState``
    or a ``Generator``.  ``dof``: another table than ``SPECTRAL_DOF`` (tests)."""
    kinds, inv_ls = kern_parts
    kinds = [int(k) for k in np.ravel(kinds)]
    m, size, n, d = int(features), int(size), int(n), int(d)
    inv_ls = np.asarray(inv_ls, dtype=float).reshape(len(kinds), d)
    if m < 1 or size < 1:
        raise ValueError("at least one feature and one path (features = %d, size = %d)"
                         % (m, size))
    table = SPECTRAL_DOF if dof is None else dof
    Omega = np.zeros((m, d))
    for p, kind in enumerate(kinds):
        if kind not in table:
            raise ValueError("unknown kernel kind %r" % (kind,))
        z = rng.standard_normal((m, d))
        nu2 = table[kind]
        if nu2 is not None:
            u = rng.chisquare(nu2, m)
            z = z / np.sqrt(u / nu2)[:, None]
        Omega += inv_ls[p] * z
    b = 2.0 * np.pi * rng.random(m)
    W = rng.standard_normal((m, size))
    E = np.sqrt(noise_var + 1e-8) * rng.standard_normal((n, size))
    if noise_scale is not None:     # per-observation noise: variance (noise_var + 1e-8) r_i
        E = E * np.sqrt(np.asarray(noise_scale, dtype=float).reshape(n, 1))
    return Omega, b, W, E


class PosteriorPaths(object):
    """``size`` posterior sample paths of one GP: ``Omega`` (m, d), ``phase`` (m), ``W``
    (m, size) and the data weights ``V`` (n, size).  A snapshot: it belongs to the data and
    hyper-parameters the GP had when it was made, and refuses to be evaluated after they
    changed.

    ``evaluate(X) -> (N, size)`` does the arithmetic (the device call; the CPU tests pass a
    NumPy form); ``current()`` returns the GP's version token as it is now, ``version`` is
    the token the paths were made at."""

    def __init__(self, Omega, phase, W, V, evaluate, current, device=None):
        self.Omega, self.phase, self.W, self.V = Omega, phase, W, V
        m, d = Omega.shape
        if phase.shape != (m,) or W.ndim != 2 or W.shape[0] != m or V.ndim != 2 \
                or V.shape[1] != W.shape[1]:
            raise ValueError("inconsistent shapes: Omega %r, phase %r, W %r, V %r"
                             % (Omega.shape, phase.shape, W.shape, V.shape))
        self._evaluate, self._current = evaluate, current
        self.version = current()
        self.device = device            # the device GP (SafeOpt.thompson_points)

    size = property(lambda self: self.W.shape[1])
    features = property(lambda self: self.Omega.shape[0])
    input_dim = property(lambda self: self.Omega.shape[1])

    def check(self):
        """``ValueError`` when the GP changed since the paths were drawn."""
        if self._current() != self.version:
            raise ValueError("the sample paths are stale: the GP's data or hyper-parameters "
                             "changed since posterior_paths() drew them -- draw new ones")

    def paths(self, X):
        """The paths at the rows of ``X``: ``(N, 1, size)``, the shape of
        ``posterior_samples_f``.  Any number of rows, repeatable bit for bit."""
        self.check()
        X = np.atleast_2d(np.asarray(X, dtype=float))
        if X.ndim != 2 or X.shape[1] != self.input_dim:
            raise ValueError("X must have %d columns, got %r" % (self.input_dim, X.shape))
        out = self._evaluate(X)
        return out[:, None, :]
