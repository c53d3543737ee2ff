"""GPy-model-like handle backed by the HIP library.

``import safeopt_amd.gpy as GPy`` gives the slice of GPy's API that SafeOpt
touches (``/root/reference/safeopt/gp_opt.py:83, 121-126, 227, 267, 275, 469,
591, 847, 929, 973, 1093, 1117, 1132``; ``utilities.py:89, 135, 203, 282,
355``)::

    kernel = GPy.kern.RBF(input_dim=2, variance=2., lengthscale=1.0, ARD=True)
    gp = GPy.models.GPRegression(x0, y0, kernel, noise_var=0.05**2)
    gp.set_XY(X, Y); mean, var = gp.predict_noiseless(Xnew); gp.kern.K(X, X2)

Every number is produced on the GPU: ``set_XY`` builds the covariance matrix,
factorises it and inverts the factor on the device; ``predict_noiseless`` and
``kern.K`` run HIP kernels; ``log_likelihood`` and every evaluation of
``optimize`` (value and gradient of the marginal likelihood) are one device
call.  The Python objects only carry hyper-parameters and the host copies of
``X`` / ``Y`` that SafeOpt's plumbing reads back.
"""
from __future__ import annotations

import copy as _copy
import types as _types

import numpy as np

from . import _hip
from . import hyper as _hyper
from . import paths as _paths

__all__ = ["kern", "models"]


class _Kern(object):
    name = "kern"

    def __init__(self, input_dim, active_dims=None, name=None):
        self.input_dim = int(input_dim)
        if active_dims is None:
            active_dims = np.arange(self.input_dim)
        self.active_dims = np.atleast_1d(np.asarray(active_dims, dtype=int))
        if name is not None:
            self.name = name

    def __mul__(self, other):
        return Prod([self, other])

    def copy(self):
        return _copy.deepcopy(self)

    # -- device descriptor: (d, kinds, variances, inv_ls[n_parts, d])
    def _parts(self):
        raise NotImplementedError

    def _desc(self, d=None):
        parts = self._parts()
        need = max(int(p.active_dims.max()) + 1 for p in parts)
        d = need if d is None else int(d)
        if d < need:
            raise ValueError("kernel acts on column %d but inputs have %d "
                             "columns" % (need - 1, d))
        if d > _hip.MAX_D or len(parts) > _hip.MAX_PARTS:
            raise ValueError("at most %d input columns and %d kernel factors "
                             "are supported" % (_hip.MAX_D, _hip.MAX_PARTS))
        kinds = np.array([p._kind for p in parts], dtype=np.int32)
        variances = np.array([float(np.asarray(p.variance).ravel()[0])
                              for p in parts])
        inv_ls = np.zeros((len(parts), d))
        for i, p in enumerate(parts):
            ls = np.asarray(p.lengthscale, dtype=float).ravel()
            if ls.size == 1:
                inv_ls[i, p.active_dims] = 1.0 / ls[0]
            else:
                inv_ls[i, p.active_dims] = 1.0 / ls
        return d, kinds, variances, inv_ls

    def _signature(self):
        """The hyper-parameters as they are NOW (cheap: a few byte strings): the GP
        handle compares it with the one it was fitted with, so that an edit in place
        (``kern.lengthscale[0] = 2.``, ``kern.variance = 3.``) takes effect at the next
        use, as GPy's parameter observers make it."""
        return tuple((np.asarray(p.variance, dtype=float).tobytes(),
                      np.asarray(p.lengthscale, dtype=float).tobytes())
                     for p in self._parts())

    def K(self, X, X2=None):
        """Covariance matrix ``k(X, X2)`` (``X2=None``: ``k(X, X)``)."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        X2 = X if X2 is None else np.atleast_2d(np.asarray(X2, dtype=float))
        desc = self._desc(X.shape[1])
        return _hip.Context.default().kern_K(desc, X, X2)

    def Kdiag(self, X):
        """``k(x, x)`` = product of the variances (stationary kernels)."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        out = np.empty(X.shape[0])
        out[:] = np.prod([float(np.asarray(p.variance).ravel()[0])
                          for p in self._parts()])
        return out


class _Stationary(_Kern):
    _kind = None

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False,
                 active_dims=None, name=None):
        super(_Stationary, self).__init__(input_dim, active_dims, name)
        if self.active_dims.size != self.input_dim:
            raise ValueError("active_dims must list input_dim columns")
        self.ARD = bool(ARD)
        if lengthscale is None:
            lengthscale = np.ones(self.input_dim if self.ARD else 1)
        lengthscale = np.atleast_1d(np.asarray(lengthscale, dtype=float))
        if self.ARD and lengthscale.size == 1:
            lengthscale = np.ones(self.input_dim) * lengthscale
        if not self.ARD and lengthscale.size != 1:
            raise ValueError("a non-ARD kernel takes one lengthscale")
        if self.ARD and lengthscale.size != self.input_dim:
            raise ValueError("ARD needs one lengthscale per input dimension")
        self.lengthscale = lengthscale
        self.variance = np.atleast_1d(np.asarray(variance, dtype=float))

    def _parts(self):
        return [self]


class RBF(_Stationary):
    """``variance * exp(-r^2 / 2)``"""
    name = "rbf"
    _kind = _hip.RBF


class Matern32(_Stationary):
    """``variance * (1 + sqrt(3) r) exp(-sqrt(3) r)``"""
    name = "Mat32"
    _kind = _hip.MATERN32


class Matern52(_Stationary):
    """``variance * (1 + sqrt(5) r + 5/3 r^2) exp(-sqrt(5) r)``"""
    name = "Mat52"
    _kind = _hip.MATERN52


class Prod(_Kern):
    """``k1 * k2`` -- factors stay reachable by name (``kernel.context``)."""
    name = "mul"

    def __init__(self, parts):
        flat = []
        for p in parts:
            flat.extend(p.parts if isinstance(p, Prod) else [p])
        self.parts = flat
        dims = np.unique(np.concatenate([p.active_dims for p in flat]))
        super(Prod, self).__init__(int(dims.max()) + 1, dims)
        for p in flat:
            setattr(self, p.name, p)

    def _parts(self):
        return self.parts


class GPRegression(object):
    """Exact GP regression with Gaussian noise, zero mean, no normaliser.

    Mirrors ``GPy.models.GPRegression(X, Y, kernel=None, noise_var=1.)`` as
    SafeOpt uses it.  Hyper-parameters are taken from the kernel object each
    time the model is (re)fitted; an edit in place refits the resident data on
    the device.  ``optimize()`` / ``optimize_restarts()`` fit them by maximum
    marginal likelihood (L-BFGS-B, softplus-transformed as in GPy) and write the
    result back into ``kern.variance`` / ``kern.lengthscale`` / ``noise_var``.
    The reference never calls ``gp.optimize()``: fit first, then build the
    ``SafeOpt`` object (its ``scaling='auto'`` reads ``kern.Kdiag`` once).
    ``predict_noiseless`` / ``predict`` / ``_raw_predict`` take ``full_cov=True``
    (the joint covariance of up to ``SGP_MAX_JOINT`` rows), and
    ``posterior_samples_f`` / ``posterior_samples`` draw sample paths from it; the
    normal numbers come from NumPy's global generator, everything else is computed
    on the device.  ``posterior_paths`` draws sample paths as functions (pathwise
    conditioning): no row limit, evaluated anywhere and again.
    """

    #: noise scales of the observations (None: none were ever given, all ones) and, per row, the
    #: sufficient statistics of the measurements it pools (None: one measurement; ``pool_data``)
    _r = None
    _stats = None

    def _st(self):
        st = self._stats
        if st is None or len(st) != self.X.shape[0]:
            st = self._stats = [None] * self.X.shape[0]
        return st

    def __init__(self, X, Y, kernel=None, noise_var=1., device=None, noise_scale=None):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        Y = np.atleast_2d(np.asarray(Y, dtype=float))
        if Y.shape[1] != 1:
            raise ValueError("one output column per GP (SafeOpt passes a list "
                             "of GPs for several constraints)")
        if kernel is None:
            kernel = RBF(X.shape[1])
        self.kern = kernel
        self.noise_var = float(noise_var)
        self.input_dim = X.shape[1]
        self._ctx = _hip.Context.default(device)
        self._dev = None
        self._dev_key = None
        self._sig = None
        self._dev_fitted = False
        #: one-row changes of the data use bordered updates (set False to
        #: re-factorise from scratch on every ``set_XY`` like GPy)
        self.incremental = True
        self.X = X
        self.Y = Y
        self.set_XY(X, Y, noise_scale=noise_scale)

    @property
    def noise_scale(self):
        """Noise scale ``r_i`` of every observation, ``(n,)``, read-only: observation ``i``
        has noise variance ``(noise_var + 1e-8) r_i``."""
        r = np.ones(self.X.shape[0]) if self._r is None else self._r.copy()
        r.flags.writeable = False
        return r

    def _scales_arg(self, noise_scale, rows):
        if noise_scale is None:
            return None
        r = np.array(np.broadcast_to(np.asarray(noise_scale, dtype=float).reshape(-1),
                                     (rows,)))
        if not (np.all(np.isfinite(r)) and np.all(r > 0)):
            raise ValueError("noise scales must be finite and positive, got %r" % (r,))
        return r

    def _eff(self, r, rows):
        return np.ones(rows) if r is None else r

    @property
    def Gaussian_noise_variance(self):
        return self.noise_var

    def _device_gp(self, in_place=False):
        desc = self.kern._desc(self.input_dim)
        key = (desc[0], desc[1].tobytes(), desc[2].tobytes(),
               desc[3].tobytes(), self.noise_var)
        if self._dev is None or key != self._dev_key:
            if (in_place and self._dev is not None and self._dev_fitted
                    and key[:2] == self._dev_key[:2]):
                # only numbers changed: the same device GP, its data resident, refitted
                self._dev_key = None
                self._dev_fitted = False
                self._dev.set_hyper(desc[2], desc[3], self.noise_var)   # may raise LinAlgError
                self._dev_fitted = True
            else:
                self._dev = _hip.DeviceGP(self._ctx, desc, self.noise_var)
                self._dev_fitted = False
            self._dev_key = key
        self._sig = (self.kern._signature(), self.noise_var)
        return self._dev

    def set_XY(self, X, Y, noise_scale=None):
        """Replace the training data and refit (device Cholesky + inverse).
        ``noise_scale``: one scale per observation (or one for all), None = all ones."""
        X = np.array(np.atleast_2d(X), dtype=float)
        Y = np.array(np.atleast_2d(Y), dtype=float)
        if X.shape[0] != Y.shape[0] or X.shape[1] != self.input_dim:
            raise ValueError("inconsistent X %r / Y %r" % (X.shape, Y.shape))
        r = self._scales_arg(noise_scale, X.shape[0])
        old_X, old_Y, old_r, old_stats = self.X, self.Y, self._r, self._st()
        self.X, self.Y, self._r = X, Y, r
        self._stats = [None] * X.shape[0]
        dev = self._device_gp()
        n = X.shape[0]
        # what SafeOpt does every iteration is one row more (or one fewer):
        # bordered O(n^2) update instead of the O(n^3) re-factorisation
        if self._dev_fitted and dev.n == old_X.shape[0] and self.incremental:
            scaled = r is not None or old_r is not None
            if (n == dev.n + 1 and np.array_equal(X[:-1], old_X)
                    and np.array_equal(Y[:-1], old_Y)
                    and (not scaled or np.array_equal(self._eff(r, n)[:-1],
                                                      self._eff(old_r, n - 1)))):
                if (dev.append(X[-1], Y[-1, 0], self._eff(r, n)[-1]) if scaled
                        else dev.append(X[-1], Y[-1, 0])):
                    self._stats = list(old_stats) + [None]
                    if scaled:
                        self._r = self._eff(r, n)
                    return
            elif (n == dev.n - 1 and n >= 1 and np.array_equal(X, old_X[:-1])
                    and np.array_equal(Y, old_Y[:-1])
                    and (not scaled or np.array_equal(self._eff(r, n),
                                                      self._eff(old_r, n + 1)[:-1]))):
                dev.pop()
                self._stats = list(old_stats[:-1])
                if scaled:
                    self._r = self._eff(r, n)
                return
        if r is None:
            dev.set_data(X, Y[:, 0])
        else:
            dev.set_data(X, Y[:, 0], r)
        self._dev_fitted = True

    def _refit(self):
        """The data as the model holds them, fitted from scratch on the device."""
        dev = self._device_gp()
        if self._r is None:
            dev.set_data(self.X, self.Y[:, 0])
        else:
            dev.set_data(self.X, self.Y[:, 0], self._r)
        self._dev_fitted = True

    def _reweigh(self, index, y, r):
        """Row ``index`` becomes ``(y, r)``: one ``sgp_gp_reweigh`` on the device, or -- with
        ``incremental = False``, a device GP out of step, or a failed pivot -- a refit."""
        n = self.X.shape[0]
        y, r = float(y), float(r)
        if not np.isfinite(y):
            raise ValueError("the value of an observation must be finite, got %r" % (y,))
        if not (np.isfinite(r) and r > 0):
            raise ValueError("noise scales must be finite and positive, got %r" % (r,))
        Y = self.Y.copy()
        Y[index, 0] = y
        rs = self._eff(self._r, n).copy()
        rs[index] = r
        dev = self._device_gp()
        in_step = self._dev_fitted and dev.n == n and self.incremental
        self.Y = Y
        if self._r is not None or r != 1.0:
            self._r = rs
        if not (in_step and dev.reweigh(index, y, r)):
            self._refit()

    def _row(self, index):
        n = self.X.shape[0]
        if not -n <= index < n:
            raise IndexError("observation %d of %d" % (index, n))
        return int(index) % n

    def reweigh_data(self, index, y=None, noise_scale=None):
        """Re-weight and / or replace observation ``index`` in place: its value becomes ``y``
        (None: stays), its noise scale ``noise_scale`` (None: stays).  An O(n^2) update of
        the factor on the device (``sgp_gp_reweigh``), ``n`` does not change: down-weighting
        a suspect reading instead of removing it.  The row's pooling statistics are
        dropped: it counts as one measurement from here on."""
        i = self._row(index)
        y = self.Y[i, 0] if y is None else y
        r = self._eff(self._r, self.X.shape[0])[i] if noise_scale is None else noise_scale
        self._reweigh(i, y, r)
        self._st()[i] = None

    def _row_stats(self, i):
        """[k, sum 1/rho, sum y/rho, sum y^2/rho, sum log rho] of row ``i``."""
        st = self._st()[i]
        if st is None:
            y, r = self.Y[i, 0], self._eff(self._r, self.X.shape[0])[i]
            st = [1, 1.0 / r, y / r, y * y / r, np.log(r)]
        return list(st)

    def pool_data(self, index, y, noise_scale=1.0):
        """One MORE measurement ``y`` (noise scale ``noise_scale``) at the input of row
        ``index``: the row becomes the pooled observation ``r = 1 / sum_j 1/rho_j``, ``y =
        r sum_j y_j/rho_j`` of all its measurements -- for the posterior exactly what a
        separate row per measurement gives, at the cost of one append and without growing
        ``n``.  ``log_likelihood`` and ``optimize`` account for the pooled measurements
        (the model keeps the sufficient statistics per row)."""
        i = self._row(index)
        y, rho = float(y), float(noise_scale)
        if not np.isfinite(y) or not (np.isfinite(rho) and rho > 0):
            raise ValueError("a finite value and a finite positive noise scale, got %r, %r"
                             % (y, rho))
        st = self._row_stats(i)
        st = [st[0] + 1, st[1] + 1.0 / rho, st[2] + y / rho, st[3] + y * y / rho,
              st[4] + np.log(rho)]
        self._reweigh(i, st[2] / st[1], 1.0 / st[1])
        self._st()[i] = st

    def unpool_data(self, index, y, noise_scale=1.0):
        """Take BACK one measurement ``(y, noise_scale)`` that ``pool_data`` (or the row's
        first observation) put into row ``index``.  ``ValueError`` for the last member of a
        row: remove the row instead (``remove_data``)."""
        i = self._row(index)
        y, rho = float(y), float(noise_scale)
        if not np.isfinite(y) or not (np.isfinite(rho) and rho > 0):
            raise ValueError("a finite value and a finite positive noise scale, got %r, %r"
                             % (y, rho))
        st = self._row_stats(i)
        if st[0] < 2:
            raise ValueError("row %d holds one measurement: remove the row instead" % i)
        st = [st[0] - 1, st[1] - 1.0 / rho, st[2] - y / rho, st[3] - y * y / rho,
              st[4] - np.log(rho)]
        if not st[1] > 0:
            raise ValueError("measurement (%r, %r) is not part of row %d" % (y, rho, i))
        self._reweigh(i, st[2] / st[1], 1.0 / st[1])
        self._st()[i] = st if st[0] > 1 else None

    def pooled_counts(self):
        """Number of measurements every row stands for, ``(n,)`` (1 without pooling)."""
        return np.array([1 if st is None else st[0] for st in self._st()], dtype=int)

    def _pool_term(self, noise_var):
        """``log p(measurements) - log p(pooled rows)`` and its derivative in ``noise_var``:
        per pooled row ``-(k-1)/2 log(2 pi s) - 1/2 sum_j log rho_j + 1/2 log r - (sum_j
        y_j^2/rho_j - ybar^2/r) / (2 s)`` with ``s = noise_var + 1e-8``; it depends on the
        data and ``s`` only."""
        s = float(noise_var) + 1e-8
        val = grad = 0.0
        for st in self._st():
            if st is None:
                continue
            k, s1, sy, syy, slog = st
            q = syy - sy * sy / s1             # sum y^2/rho - ybar^2 / r
            val += -0.5 * (k - 1) * np.log(2 * np.pi * s) - 0.5 * slog - 0.5 * np.log(s1) \
                - q / (2 * s)
            grad += -0.5 * (k - 1) / s + q / (2 * s * s)
        return val, grad

    def append_XY(self, X, Y, noise_scale=None):
        """``b >= 1`` more observations (``X`` (b, d), ``Y`` (b, 1)) behind the data: block
        appends on the device (``sgp_gp_append_block``, chunks of at most ``MAX_BLOCK`` rows:
        one O(b n^2) update and one read-back per chunk) when the model is fitted,
        ``incremental`` is on and the device GP is in step; otherwise, or when a chunk is
        refused (no capacity, a pivot not positive), ``set_XY`` with the stacked arrays."""
        Xn = np.array(np.atleast_2d(X), dtype=float)
        Yn = np.array(np.atleast_2d(Y), dtype=float)
        if Yn.shape[0] != Xn.shape[0] and Yn.shape == (1, Xn.shape[0]):
            Yn = Yn.T
        if (Xn.shape[0] != Yn.shape[0] or Xn.shape[1] != self.input_dim or Yn.shape[1] != 1
                or Xn.shape[0] < 1):
            raise ValueError("inconsistent X %r / Y %r" % (Xn.shape, Yn.shape))
        rn = self._scales_arg(noise_scale, Xn.shape[0])
        X, Y = np.vstack([self.X, Xn]), np.vstack([self.Y, Yn])
        r = None
        if rn is not None or self._r is not None:
            r = np.concatenate([self._eff(self._r, self.X.shape[0]),
                                self._eff(rn, Xn.shape[0])])
        stats = list(self._st()) + [None] * Xn.shape[0]
        dev = self._device_gp()
        if self._dev_fitted and dev.n == self.X.shape[0] and self.incremental:
            for s in range(0, Xn.shape[0], _hip.MAX_BLOCK):
                xb, yb = Xn[s:s + _hip.MAX_BLOCK], Yn[s:s + _hip.MAX_BLOCK, 0]
                if not (dev.append_block(xb, yb) if r is None else dev.append_block(
                        xb, yb, self._eff(rn, Xn.shape[0])[s:s + _hip.MAX_BLOCK])):
                    break
            else:
                self.X, self.Y, self._r, self._stats = X, Y, r, stats
                return
        if r is None:
            self.set_XY(X, Y)
        else:
            self.set_XY(X, Y, noise_scale=r)
        self._stats = stats

    def remove_data(self, index):
        """Forget observation ``index`` (0 .. n-1), whichever it is: an O(n^2) downdate
        of the factor on the device (``sgp_gp_remove``) instead of the refit ``set_XY``
        with the reduced arrays costs -- which is what happens with ``incremental =
        False``, or when a pivot of the downdate is not positive.  The row's noise scale and
        pooling statistics go with it."""
        n = self.X.shape[0]
        if not -n <= index < n:
            raise IndexError("observation %d of %d" % (index, n))
        if n < 2:
            raise ValueError("cannot remove the only observation")
        index = int(index) % n
        X, Y = np.delete(self.X, index, axis=0), np.delete(self.Y, index, axis=0)
        r = None if self._r is None else np.delete(self._r, index)
        stats = self._st()[:index] + self._st()[index + 1:]
        dev = self._device_gp()
        if (self._dev_fitted and dev.n == n and self.incremental
                and dev.remove(index)):
            self.X, self.Y, self._r, self._stats = X, Y, r, stats
            return
        if r is None:
            self.set_XY(X, Y)
        else:
            self.set_XY(X, Y, noise_scale=r)
        self._stats = stats

    def _fitted(self):
        """Device GP, fitted.  Hot path: a comparison of the hyper-parameter bytes
        when nothing changed; an edited kernel parameter or ``noise_var`` refits the
        device model here, at the next use (GPy refits through its observers)."""
        if self._dev is not None and self._dev_fitted:
            if (self.kern._signature(), self.noise_var) == self._sig:
                return self._dev
        dev = self._device_gp(in_place=True)
        if not self._dev_fitted:
            if self._r is None:
                dev.set_data(self.X, self.Y[:, 0])
            else:
                dev.set_data(self.X, self.Y[:, 0], self._r)
            self._dev_fitted = True
        return dev

    # -- fitting the hyper-parameters
    def _evaluate(self, variances, inv_ls, noise_var, loo=False):
        """One device call: likelihood and gradient at theta; the device GP is left
        fitted there (or unfitted, data resident, when theta is infeasible).  ``loo``: the
        leave-one-out log pseudo-likelihood instead of the marginal likelihood."""
        dev = self._dev
        if dev is None or dev.n != self.X.shape[0]:
            dev = self._fitted()
        out = (dev.loo_lml if loo else dev.lml)(variances, inv_ls, noise_var)
        if not loo and any(st is not None for st in self._st()):
            # pooled rows: the likelihood of the measurements they stand for
            val, grad = self._pool_term(noise_var)
            out = (out[0] + val, out[1] + grad) + tuple(out[2:])
        self._dev_fitted = out[4] == 0
        self._dev_key = (self.input_dim, self._dev_key[1], np.asarray(variances).tobytes(),
                         np.asarray(inv_ls).tobytes(), float(noise_var))
        self._sig = None
        return out

    def _settle(self):
        """After evaluations: is the device GP fitted at the values the objects hold?"""
        desc = self.kern._desc(self.input_dim)
        key = (desc[0], desc[1].tobytes(), desc[2].tobytes(), desc[3].tobytes(),
               self.noise_var)
        if self._dev_fitted and key == self._dev_key:
            self._sig = (self.kern._signature(), self.noise_var)

    def log_likelihood(self):
        """``log p(y | X, theta)`` at the current hyper-parameters; with pooled rows
        (``pool_data``) the likelihood of all the measurements they stand for."""
        self._fitted()
        desc = self.kern._desc(self.input_dim)
        ll, _, _, _, info = self._evaluate(desc[2], desc[3], self.noise_var)
        self._settle()
        if info != 0:
            raise np.linalg.LinAlgError("not positive definite (pivot %d)" % info)
        return ll

    def objective_function(self):
        return -self.log_likelihood()

    # -- leave-one-out cross-validation (Rasmussen & Williams 5.4.2)
    def _evaluate_loo(self, variances, inv_ls, noise_var):
        return self._evaluate(variances, inv_ls, noise_var, loo=True)

    def _evaluator(self, objective):
        """The evaluate callback of ``optimize(objective=...)``; checked before any device
        use."""
        if objective == 'lml':
            return self._evaluate
        if objective == 'loo':
            return self._evaluate_loo
        raise ValueError("objective %r: 'lml' (marginal likelihood) or 'loo' (leave-one-out "
                         "log pseudo-likelihood)" % (objective,))

    def loo(self):
        """Leave-one-out predictions ``(mean, var)``, ``(n, 1)`` each: every observation
        predicted from all the others at the current hyper-parameters, ``var`` the
        predictive variance of the noisy observation.  Closed form from the resident
        factor, O(n^2) for all of them together (``sgp_gp_loo``).  A pooled row
        (``pool_data``) is ONE observation here, of noise variance ``(noise_var + 1e-8)
        r_i``: it is left out as a whole."""
        mean, var, _ = self._fitted().loo()
        return mean[:, None], var[:, None]

    def loo_residuals(self):
        """Standardised leave-one-out residuals ``z = (y - mean) / sqrt(var)``, ``(n, 1)``:
        about N(0, 1) each when the model explains the data; a faulty reading stands out."""
        mean, var = self.loo()
        return (self.Y - mean) / np.sqrt(var)

    def log_pseudo_likelihood(self):
        """The leave-one-out log pseudo-likelihood ``L_LOO = sum_i log p(y_i | X, y_-i,
        theta)`` at the current hyper-parameters."""
        self._fitted()
        desc = self.kern._desc(self.input_dim)
        ll, _, _, _, info = self._evaluate_loo(desc[2], desc[3], self.noise_var)
        self._settle()
        if info != 0:
            raise np.linalg.LinAlgError("not positive definite (pivot %d)" % info)
        return ll

    def optimize(self, optimizer='lbfgsb', max_iters=1000, messages=False, fixed=(),
                 objective='lml'):
        """Maximise the marginal likelihood over the hyper-parameters (L-BFGS-B on the
        softplus-transformed values, GPy's defaults); every evaluation is one device
        call.  ``fixed``: names to leave alone (``'noise_var'``, ``'<part>.variance'``,
        ``'<part>.lengthscale'``; ``'variance'`` / ``'lengthscale'`` for a single
        kernel).  The fitted values are written in place into ``kern`` / ``noise_var``
        and the model is fitted at them.  Returns an object with ``f_opt``, ``x_opt``,
        ``funct_eval``, ``status``.  ``objective='loo'`` maximises the leave-one-out log
        pseudo-likelihood instead (``f_opt = -L_LOO``): more robust than the marginal
        likelihood when the kernel family does not fit the data; it treats a pooled row
        (``pool_data``) as one observation, where ``'lml'`` accounts for every measurement
        of the row."""
        evaluate = self._evaluator(objective)
        if optimizer not in ('lbfgsb', 'lbfgs', None):
            raise NotImplementedError("optimizer %r (only 'lbfgsb')" % (optimizer,))
        self._fitted()
        params = _hyper.Parameters(self.kern, self.noise_var, self.input_dim, fixed)
        try:
            res = _hyper.optimize(params, evaluate, max_iters=max_iters,
                                  messages=messages)
        finally:
            self.noise_var = params.noise_var
            self._settle()
        return res

    def optimize_restarts(self, num_restarts=10, robust=True, **kwargs):
        """``optimize`` from the current values and from ``num_restarts - 1`` random
        starts (``N(0, 1)`` per transformed parameter, NumPy's global generator);
        keeps the best.  ``objective`` as in ``optimize``."""
        fixed = kwargs.pop('fixed', ())
        evaluate = self._evaluator(kwargs.pop('objective', 'lml'))
        if kwargs.pop('optimizer', 'lbfgsb') not in ('lbfgsb', 'lbfgs', None):
            raise NotImplementedError("only 'lbfgsb'")
        self._fitted()
        params = _hyper.Parameters(self.kern, self.noise_var, self.input_dim, fixed)
        try:
            res = _hyper.optimize_restarts(params, evaluate, num_restarts=num_restarts,
                                           robust=robust, **kwargs)
        finally:
            self.noise_var = params.noise_var
            self._settle()
        return res

    def parameters_changed(self):
        """Refit the device model with the current hyper-parameters NOW.  Not needed
        for correctness -- an edit of ``kern.variance`` / ``kern.lengthscale`` /
        ``noise_var`` is noticed at the next use -- kept for code that called it."""
        self._dev_fitted = False
        self._fitted()

    def predict_noiseless(self, Xnew, full_cov=False):
        """Posterior mean and variance of the latent function, ``(N,1)`` each;
        the variance is clipped to ``[1e-15, inf)`` as in GPy.  ``full_cov=True``: the
        joint covariance ``(N, N)`` instead (exactly symmetric, not clipped -- GPy clips
        only the variance), at most ``SGP_MAX_JOINT`` rows."""
        if full_cov:
            return self._fitted().predict_cov(Xnew)
        return self._fitted().predict(Xnew)

    def _raw_predict(self, Xnew, full_cov=False):
        return self.predict_noiseless(Xnew, full_cov=full_cov)

    def predict(self, Xnew, full_cov=False, include_likelihood=True):
        mean, var = self.predict_noiseless(Xnew, full_cov=full_cov)
        if include_likelihood:
            if full_cov:
                # GPy's Gaussian likelihood: the noise is independent per point
                var[np.diag_indices(var.shape[0])] += self.noise_var
            else:
                var = var + self.noise_var
        return mean, var

    def posterior_samples_f(self, X, size=10):
        """``size`` sample paths of the latent function at the rows of ``X``, ``(N, 1,
        size)`` as in GPy: one ``np.random.randn(N, size)`` on the global generator, then
        one device call (joint covariance, its Cholesky factor -- GPy's jitter when it is
        needed -- and ``mean + C Z``)."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        dev = self._fitted()
        N = X.shape[0]
        if N > _hip.MAX_JOINT:
            raise ValueError("%d rows in one joint prediction: at most SGP_MAX_JOINT = %d"
                             % (N, _hip.MAX_JOINT))
        Z = np.random.randn(N, int(size))
        out, _, _ = dev.draw(X, Z)
        return out[:, None, :]

    def _paths_token(self):
        """What a ``PosteriorPaths`` snapshot belongs to: the device GP and its data version,
        and the hyper-parameters as the objects hold them now."""
        dev = self._dev
        return (None if dev is None else (dev.serial, dev.version),
                self.kern._signature(), self.noise_var)

    def posterior_paths(self, size=16, features=1024):
        """``size`` posterior sample paths as FUNCTIONS (pathwise conditioning, Wilson et al.
        2020): a ``PosteriorPaths`` whose ``paths(X)`` returns ``(N, 1, size)`` like
        ``posterior_samples_f`` -- but for any number of rows, again and again, the same bits
        for the same rows.  ``features`` random Fourier features carry the prior draw; the
        random numbers come from NumPy's global generator in the order ``safeopt_amd.paths``
        documents (``np.random.seed`` pins the paths), the data weights and every evaluation
        are device calls.  A snapshot of the GP as it is now: after ``set_XY`` or an edited
        hyper-parameter ``paths`` raises ``ValueError``.  Approximate in the prior term only
        (error ~ ``features ** -0.5``); the data update is exact."""
        dev = self._fitted()
        desc = self.kern._desc(self.input_dim)
        Om, b, W, E = _paths.draw_path_inputs((desc[1], desc[3]), self.noise_var, dev.n,
                                              self.input_dim, size, features,
                                              noise_scale=self._r)
        V = dev.path_weights(Om, b, W, E)
        return _paths.PosteriorPaths(Om, b, W, V,
                                     lambda X: dev.paths_eval(Om, b, W, V, X),
                                     self._paths_token, device=dev)

    def max_value_entropy(self, X, ystar, floor=None):
        """Max-value entropy search acquisition (Wang & Jegelka 2017) at the rows of ``X``,
        ``(N, 1)``: with ``mu, v = predict_noiseless(X)``, ``sigma = sqrt(max(v, 1e-15))``,
        ``y_k = max(ystar[k], floor)`` and ``gamma_k = (y_k - mu) / sigma``, the mean over
        ``k`` of ``gamma phi(gamma) / (2 Phi(gamma)) - ln Phi(gamma)`` -- the information a
        noiseless measurement at the row carries about the value of the maximum, ``ystar``
        being ``K <= 64`` draws of that maximum (``posterior_paths(...).paths(X).max(0)``).
        ``floor``: a value no maximum can lie below (the best posterior mean, say); None for
        none.  One device call behind the prediction (``sgp_mes_eval``), finite for every
        ``gamma``."""
        mean, var = self.predict_noiseless(X)
        dev = self._fitted()
        return dev.ctx.mes_eval(mean, var, ystar, -np.inf if floor is None else float(floor))

    def log_expected_improvement(self, X, best, xi=0.0):
        """The logarithm of the expected improvement over ``best`` at the rows of ``X``,
        ``(N, 1)``: with ``mu, v = predict_noiseless(X)``, ``sigma = sqrt(max(v, 1e-15))`` and
        ``z = (mu - best - xi) / sigma``, ``ln sigma + ln(phi(z) + z Phi(z))`` (LogEI, Ament et
        al. 2023) -- finite and ordered where the expected improvement itself underflows to 0.
        ``best`` finite, ``xi >= 0``.  One device call behind the prediction
        (``sgp_ei_eval``)."""
        mean, var = self.predict_noiseless(X)
        dev = self._fitted()
        return dev.ctx.ei_eval(mean.ravel(), var.ravel(), float(best),
                               float(xi)).reshape(-1, 1)

    def posterior_samples(self, X, size=10):
        """``posterior_samples_f`` plus observation noise: ``sqrt(noise_var)`` times a
        second draw ``np.random.randn(N, 1, size)``."""
        f = self.posterior_samples_f(X, size=size)
        return f + np.sqrt(self.noise_var) * np.random.randn(*f.shape)


kern = _types.SimpleNamespace(Kern=_Kern, RBF=RBF, Matern32=Matern32, Matern52=Matern52,
                              Prod=Prod)
models = _types.SimpleNamespace(GPRegression=GPRegression)
