"""Parameter bookkeeping of ``GPRegression.optimize`` (NumPy and SciPy only).

The free hyper-parameters of a GP -- per kernel part ``variance`` and ``lengthscale``
(one value, or one per active column with ``ARD=True``), and ``noise_var`` -- as one flat
vector ``x``, kept positive the way GPy does by default: ``theta = log(1 + exp(x))``
(GPy's ``Logexp``), optimised in ``x``.  The likelihood itself is a callable

    evaluate(variances[P], inv_ls[P, d], noise_var)
        -> (log_likelihood, d/d noise_var, d/d variances[P], d/d inv_ls[P, d], info)

in the device descriptor's layout (``kern._desc``); ``info != 0`` or a non-finite value
marks an infeasible point.  The product only ever passes ``_hip.DeviceGP.lml`` or, for
``optimize(objective='loo')``, ``_hip.DeviceGP.loo_lml`` (the leave-one-out log
pseudo-likelihood in the same layout); the seam is what the tests drive with a NumPy
likelihood.
"""
from __future__ import annotations

import numpy as np

__all__ = ["Parameters", "OptimizeResult", "optimize", "optimize_restarts"]

_LIM = 36.0          # GPy's _lim_val: softplus is the identity beyond it, to rounding


def softplus(x):
    x = np.asarray(x, dtype=float)
    return np.where(x > _LIM, x, np.log1p(np.exp(np.minimum(x, _LIM))))


def softplus_inv(theta):
    theta = np.asarray(theta, dtype=float)
    return np.where(theta > _LIM, theta, np.log(np.expm1(np.minimum(theta, _LIM))))


def softplus_grad(x):
    """d theta / d x"""
    x = np.asarray(x, dtype=float)
    return np.where(x > _LIM, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(x, _LIM))))


class Parameters(object):
    """The hyper-parameters of ``(kern, noise_var)`` as a flat vector.

    Order: for every part ``<name>.variance`` then ``<name>.lengthscale`` (its entries),
    last ``noise_var``.  ``fixed`` takes names out: ``'noise_var'``,
    ``'<part name>.variance'``, ``'<part name>.lengthscale'``, and for a single kernel
    also plain ``'variance'`` / ``'lengthscale'``.
    """

    def __init__(self, kern, noise_var, d=None, fixed=()):
        self.kern = kern
        self.parts = kern._parts()
        self.noise_var = float(noise_var)
        self.d = kern._desc(d)[0]
        if isinstance(fixed, str):
            fixed = (fixed,)
        fixed = set(fixed)
        # every entry of the full vector: (name, part index or None, field, position)
        self.entries = []
        known = {"noise_var"}
        for i, p in enumerate(self.parts):
            names = {p.name + ".variance", p.name + ".lengthscale"}
            known |= names
            self.entries.append((p.name + ".variance", i, "variance", 0))
            for j in range(np.asarray(p.lengthscale).size):
                self.entries.append((p.name + ".lengthscale", i, "lengthscale", j))
        self.entries.append(("noise_var", None, "noise_var", 0))
        if len(self.parts) == 1:
            known |= {"variance", "lengthscale"}
            fixed = {self.parts[0].name + "." + f if f in ("variance", "lengthscale") else f
                     for f in fixed}
        unknown = fixed - known
        if unknown:
            raise ValueError("unknown parameter name(s) %s; known: %s"
                             % (sorted(unknown), sorted(known)))
        self.free = np.array([e[0] not in fixed for e in self.entries])
        self.names = [e[0] for e, f in zip(self.entries, self.free) if f]

    # -- full vector of theta <-> the objects
    def _theta_full(self):
        out = np.empty(len(self.entries))
        for k, (_, i, field, j) in enumerate(self.entries):
            if i is None:
                out[k] = self.noise_var
            else:
                out[k] = np.asarray(getattr(self.parts[i], field), dtype=float).ravel()[j]
        return out

    def get_x(self):
        """The free parameters as they are now, transformed."""
        return softplus_inv(self._theta_full()[self.free])

    def theta(self, x):
        """Full vector of (untransformed) parameters with the free ones taken from x."""
        full = self._theta_full()
        full[self.free] = softplus(x)
        return full

    def set_x(self, x):
        """Write the parameters IN PLACE into the kernel objects; returns noise_var."""
        full = self.theta(x)
        for k, (_, i, field, j) in enumerate(self.entries):
            if i is None:
                self.noise_var = float(full[k])
            else:
                p = self.parts[i]
                arr = getattr(p, field)
                if not isinstance(arr, np.ndarray) or arr.dtype != np.float64 or arr.ndim != 1:
                    arr = np.atleast_1d(np.array(arr, dtype=float)).ravel()
                    setattr(p, field, arr)
                arr[j] = full[k]
        return self.noise_var

    # -- device layout
    def descriptor(self, full):
        """(variances[P], inv_ls[P, d], noise_var) of a full parameter vector."""
        P = len(self.parts)
        variances = np.empty(P)
        inv_ls = np.zeros((P, self.d))
        noise = self.noise_var
        ls = [np.empty(np.asarray(p.lengthscale).size) for p in self.parts]
        for k, (_, i, field, j) in enumerate(self.entries):
            if i is None:
                noise = float(full[k])
            elif field == "variance":
                variances[i] = full[k]
            else:
                ls[i][j] = full[k]
        for i, p in enumerate(self.parts):
            inv_ls[i, p.active_dims] = 1.0 / ls[i]       # (one value broadcasts)
        return variances, inv_ls, noise

    def fold(self, inv_ls, g_noise, g_var, g_inv_ls):
        """Gradient in the full parameter vector from the device's:
        d/d lengthscale = -inv_ls^2 d/d inv_ls, summed over the columns of a non-ARD part."""
        out = np.empty(len(self.entries))
        g_ls = -np.asarray(inv_ls) ** 2 * np.asarray(g_inv_ls)
        for k, (_, i, field, j) in enumerate(self.entries):
            if i is None:
                out[k] = g_noise
            elif field == "variance":
                out[k] = g_var[i]
            else:
                p = self.parts[i]
                cols = p.active_dims
                out[k] = g_ls[i, cols].sum() if np.asarray(p.lengthscale).size == 1 \
                    else g_ls[i, cols[j]]
        return out

    def objective(self, x, evaluate):
        """``(-log likelihood, its gradient in x)``; ``(inf, 0)`` where infeasible."""
        x = np.asarray(x, dtype=float)
        full = self.theta(x)
        variances, inv_ls, noise = self.descriptor(full)
        ll, g_noise, g_var, g_inv_ls, info = evaluate(variances, inv_ls, noise)
        if info != 0 or not np.isfinite(ll):
            return np.inf, np.zeros(x.size)
        g = self.fold(inv_ls, g_noise, g_var, g_inv_ls)[self.free] * softplus_grad(x)
        if not np.all(np.isfinite(g)):
            return np.inf, np.zeros(x.size)
        return -float(ll), -g


class OptimizeResult(object):
    """What ``optimize`` returns: ``f_opt`` (objective = -log likelihood), ``x_opt`` (the
    transformed free parameters), ``funct_eval``, ``status`` (SciPy's message), ``names``
    and ``noise_var`` (the fitted value)."""

    def __init__(self, f_opt, x_opt, funct_eval, status, names, noise_var):
        self.f_opt, self.x_opt, self.funct_eval = f_opt, x_opt, funct_eval
        self.status, self.names, self.noise_var = status, names, noise_var

    def __repr__(self):
        return "OptimizeResult(f_opt=%r, funct_eval=%d, status=%r)" % (
            self.f_opt, self.funct_eval, self.status)


def optimize(params, evaluate, x0=None, max_iters=1000, messages=False):
    """L-BFGS-B on the negative log likelihood from ``x0`` (default: the current values).
    The result is written in place into the kernel objects of ``params`` and the
    likelihood is evaluated at it last, so the evaluator (the device GP) is left fitted
    at the result."""
    from scipy.optimize import fmin_l_bfgs_b
    x0 = params.get_x() if x0 is None else np.asarray(x0, dtype=float)
    if x0.size == 0:
        raise ValueError("every parameter is fixed: nothing to optimise")
    best = [np.inf, x0.copy()]
    calls = [0]

    def fun(x):
        calls[0] += 1
        f, g = params.objective(x, evaluate)
        if f < best[0]:
            best[0], best[1] = f, x.copy()
        if not np.isfinite(f):
            # +inf tells the caller "infeasible"; the line search interpolates with the
            # value, so it gets a finite one far above everything seen (inf - inf = nan)
            f = best[0] + 1e6 * max(1.0, abs(best[0]))
        return f, g

    if not np.isfinite(params.objective(x0, evaluate)[0]):
        raise np.linalg.LinAlgError("the likelihood is not defined at the starting values")
    x, f, info = fmin_l_bfgs_b(fun, x0, maxfun=int(max_iters), maxiter=int(max_iters),
                               iprint=1 if messages else -1)
    if best[0] < f:                                  # (a line search that ended uphill)
        x, f = best[1], best[0]
    noise_var = params.set_x(x)
    f_last = fun(x)[0]                               # leaves the evaluator fitted at x
    status = info["task"]
    if isinstance(status, bytes):
        status = status.decode()
    return OptimizeResult(float(f_last), np.array(x), calls[0] + 1, status,
                          list(params.names), noise_var)


def optimize_restarts(params, evaluate, num_restarts=10, robust=True, **kwargs):
    """``num_restarts`` runs of ``optimize``: the first from the current values, every
    other from ``x ~ N(0, 1)`` per free parameter (GPy's ``randomize()`` default), drawn
    from NumPy's global generator right before its run.  The best result is written in
    place and returned; with ``robust`` a run that raises is skipped."""
    runs = []
    for r in range(int(num_restarts)):
        x0 = None if r == 0 else np.random.normal(size=int(params.free.sum()))
        try:
            runs.append(optimize(params, evaluate, x0=x0, **kwargs))
        except Exception:
            if not robust:
                raise
    if not runs:
        raise np.linalg.LinAlgError("no restart produced a likelihood")
    best = min(runs, key=lambda res: res.f_opt)
    params.set_x(best.x_opt)
    best.f_opt = float(params.objective(best.x_opt, evaluate)[0])   # evaluator left at the best
    best.noise_var = params.noise_var
    return best
