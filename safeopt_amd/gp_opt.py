"""SafeOpt / SafeOptSwarm on top of the MI355X HIP path.

Class surface = ``/root/reference/safeopt/gp_opt.py`` (constructor signatures,
method names, attribute names incl. the ``liptschitz`` spelling, exception
types).  What differs is where the arithmetic runs:

* ``SafeOpt.inputs`` lives in HBM (row-sharded over the ranks of a
  communicator), together with ``Q``, ``S``, ``M``, ``G``; the NumPy
  attributes of the same names are host mirrors that are refreshed lazily
  when read.
* ``update_confidence_intervals`` + ``compute_safe_set`` are ONE fused HIP
  kernel (``posterior_sweep``) per call; ``compute_sets`` /
  ``get_new_query_point`` are a handful of HBM-bound passes whose only host
  visible results are scalars.
* the expander loop (``gp_opt.py:557-612``) keeps its sequential semantics
  (first expander in descending-width order wins) but tests
  ``SGP_TOPK`` = 16 candidates per device pass with a closed-form rank-1
  posterior update instead of two O(n^3) re-factorisations per candidate.

The host code below is orchestration only; it never touches an ``(N, .)``
array unless the user reads one of the mirrors.
"""
from __future__ import annotations

import collections
import logging
from functools import partial

import weakref

import numpy as np

from . import _hip
from . import pooling as _pooling
from .dist import (LocalComm, allgather_rows, check_same_incumbent, check_same_maxima,
                   check_same_paths, check_same_targets,
                   gather_shard_columns,
                   merge_argmax, merge_batch_records, merge_ise_records, merge_mes_records,
                   merge_path_records, merge_topk, pick_ise, shard_range)
from .swarm import SwarmOptimization, DeviceSwarmOptimization

__all__ = ['SafeOpt', 'SafeOptFleet', 'SafeOptSwarm']

_I64_MAX = np.iinfo(np.int64).max


def _one_per_gp(value, count):
    """``value`` as a 1-d array with one entry per GP: a list is taken as it
    is, anything else is repeated for every GP (``fmin``, ``lipschitz``)."""
    items = value if isinstance(value, list) else [value] * count
    return np.atleast_1d(np.asarray(items).squeeze())


def _prior_std(gps):
    """``sqrt(k(x, x))`` of every GP (stationary kernels: taken at the origin);
    this is what ``scaling='auto'`` means in the reference (gp_opt.py:80-83)."""
    origin = np.zeros((1, gps[0].input_dim))
    return np.sqrt(np.array([g.kern.Kdiag(origin)[0] for g in gps]))


def _with_context(x, context):
    """``x`` (m, d) with the context columns appended to every row."""
    context = np.atleast_2d(context)
    out = np.empty((x.shape[0], x.shape[1] + context.shape[1]), dtype=float)
    out[:, :x.shape[1]] = x
    out[:, x.shape[1]:] = context
    return out


class GaussianProcessOptimization(object):
    """What SafeOpt and SafeOptSwarm share: the GP handles, ``fmin``,
    ``beta(t)``, ``scaling``, ``threshold`` and the measurement log.

    Same constructor, attributes and methods as the base class of the
    reference (``gp_opt.py:30-278``): ``gps`` / ``gp``, ``fmin`` (one per GP),
    ``beta`` (always callable), ``scaling``, ``x`` / ``y`` / ``data`` / ``t``,
    ``add_new_data_point`` / ``remove_last_data_point``; ``remove_data_point`` forgets
    any measurement (not in the reference).

    Not in the reference either: a measurement may come with a NOISE SCALE (``noise_scale=``
    of ``add_new_data_point``: its noise variance is that many times the GP's), and with
    ``pool_repeats=True`` a measurement at an input a GP already holds is pooled into that
    row (``GPRegression.pool_data``) instead of appended: the log stays what it is, every
    measurement in order, the posterior is the same, and the GPs grow with the number of
    distinct inputs only.
    """

    #: the map from the log to the rows of the pooled GPs (``pool_repeats=True``), else None
    _pool = None
    #: noise scales of the log, (t, n_gps), or None: none was ever given, all ones
    _rho = None

    def __init__(self, gp, fmin, beta=2, num_contexts=0, threshold=0,
                 scaling='auto', pool_repeats=False):
        self.gps = gp if isinstance(gp, list) else [gp]
        if len(self.gps) > _hip.MAX_GPS:
            raise ValueError("at most %d GPs are supported" % _hip.MAX_GPS)
        self.gp = self.gps[0]                    # GP 0 = the objective
        n_gps = len(self.gps)

        self.fmin = _one_per_gp(fmin, n_gps)
        self.beta = beta if callable(beta) else (lambda t: beta)
        self.threshold = threshold
        self.num_contexts = num_contexts

        if isinstance(scaling, str) and scaling == 'auto':
            self.scaling = _prior_std(self.gps)
        else:
            self.scaling = np.asarray(scaling)
            if self.scaling.shape[0] != n_gps:
                raise ValueError("The number of scaling values should be "
                                 "equal to the number of GPs")

        # filled in by the subclasses that discretise the domain
        self._parameter_set = None
        self.bounds = None
        self.num_samples = 0

        # measurement log: every GP must start from the same inputs
        for other in self.gps[1:]:
            if not np.allclose(self.gp.X, other.X):
                raise NotImplementedError('The GPs have different '
                                          'measurements.')
        self._x = self.gp.X
        self._y = np.concatenate([g.Y for g in self.gps], axis=1)
        if any(getattr(g, '_r', None) is not None for g in self.gps):
            self._rho = np.stack([np.asarray(g.noise_scale, dtype=float) for g in self.gps],
                                 axis=1)
        if pool_repeats:
            # the GPs' initial data are taken as they are: one row per initial measurement
            self._pool = _pooling.PoolBook(self._x, np.ones(self._y.shape, dtype=bool))

    # -- measurement log ----------------------------------------------------------
    x = property(lambda self: self._x)
    y = property(lambda self: self._y)

    @property
    def data(self):
        """The measurements ``(x, y)`` seen so far."""
        return self._x, self._y

    @property
    def t(self):
        """Time step = number of measurements."""
        return self._x.shape[0]

    def plot(self, *args, **kwargs):
        raise NotImplementedError(
            "plotting is outside the accelerated path (SURVEY.md section 2, "
            "row 13); read opt.Q / opt.S / opt.M / opt.G and plot with "
            "matplotlib directly")

    def _add_context(self, x, context):
        return _with_context(x, context)

    def _add_data_point(self, gp, x, y, context=None, noise_scale=None):
        """Append ``(x, y)`` to one GP only (``self.x`` / ``self.y`` untouched).
        One more row than before: the handle turns this ``set_XY`` into a
        bordered update of the factor (``sgp_gp_append``).  ``noise_scale``: the scales of the
        new rows (None: ones); a GP that holds scales keeps them."""
        rows = x if context is None else _with_context(x, context)
        if noise_scale is None and getattr(gp, '_r', None) is None:
            gp.set_XY(np.vstack([gp.X, rows]), np.vstack([gp.Y, y]))
            return
        new = np.ones(np.shape(rows)[0]) if noise_scale is None else np.ravel(noise_scale)
        gp.set_XY(np.vstack([gp.X, rows]), np.vstack([gp.Y, y]),
                  noise_scale=np.concatenate([gp.noise_scale, new]))

    def _scales_per_gp(self, noise_scale, rows):
        """``noise_scale`` -- a scalar, one value per GP, or (rows, n_gps) -- as (rows,
        n_gps), or None."""
        if noise_scale is None:
            return None
        r = np.asarray(noise_scale, dtype=float)
        n_gps = len(self.gps)
        if r.ndim == 0:
            r = np.full((rows, n_gps), float(r))
        elif r.ndim == 1 and r.size == n_gps:
            r = np.tile(r, (rows, 1))
        elif r.shape != (rows, n_gps):
            raise ValueError("noise_scale: a scalar or one value per GP (%d), got shape %r"
                             % (n_gps, r.shape))
        if not (np.all(np.isfinite(r)) and np.all(r > 0)):
            raise ValueError("noise scales must be finite and positive, got %r" % (r,))
        return r

    def _log(self, x, y, rho):
        """The log grows by the rows ``(x, y)`` with the noise scales ``rho`` (or None)."""
        if rho is not None or self._rho is not None:
            old = self._rho if self._rho is not None else np.ones(self._y.shape)
            new = rho if rho is not None else np.ones(y.shape)
            self._rho = np.concatenate((old, new), axis=0)
        self._x = np.concatenate((self._x, x), axis=0)
        self._y = np.concatenate((self._y, y), axis=0)

    def add_new_data_point(self, x, y, context=None, noise_scale=None):
        """Log a measurement and hand it to the GPs; a ``nan`` in column ``i``
        of ``y`` means GP ``i`` did not observe it.  ``noise_scale``: the noise variance of
        this measurement is that many times the GP's ``noise_var`` (a scalar, or one value
        per GP; None: 1).  With ``pool_repeats`` a measurement at an input the GP holds is
        pooled into that row."""
        x, y = np.atleast_2d(x), np.atleast_2d(y)
        rho = self._scales_per_gp(noise_scale, x.shape[0])
        if self.num_contexts:
            x = _with_context(x, context)
        if self._pool is not None:
            x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
            for k in range(x.shape[0]):
                for g, act in enumerate(self._pool.add(x[k], ~np.isnan(y[k]))):
                    if act is None:
                        continue
                    p = 1.0 if rho is None else rho[k, g]
                    if act[0] == 'pool':
                        self.gps[g].pool_data(act[1], y[k, g], p)
                    else:
                        self._add_data_point(self.gps[g], x[k:k + 1], y[k:k + 1, [g]],
                                             noise_scale=None if rho is None else [p])
            self._log(x, y, rho)
            return
        for i, gp in enumerate(self.gps):
            seen = ~np.isnan(y[:, i])
            if seen.any():
                if rho is None:
                    self._add_data_point(gp, x[seen, :], y[seen, [i]])
                else:
                    self._add_data_point(gp, x[seen, :], y[seen, [i]], noise_scale=rho[seen, i])
        self._log(x, y, rho)

    def _add_data_points(self, gp, rows, y, noise_scale=None):
        """Append the rows ``(rows, y)`` to one GP only: block appends of the factor
        (``GPRegression.append_XY``), a refit for a handle without them."""
        if noise_scale is not None:
            gp.append_XY(rows, y, noise_scale=noise_scale)
        elif hasattr(gp, 'append_XY'):
            gp.append_XY(rows, y)
        else:
            gp.set_XY(np.vstack([gp.X, rows]), np.vstack([gp.Y, y]))

    def add_new_data_points(self, X, Y, context=None, noise_scale=None):
        """Log ``b`` measurements at once -- the way back from ``optimize_batch`` -- and hand
        them to the GPs: ``X`` (b, d_parameters), ``Y`` (b, n_gps), a ``nan`` in ``Y[r, g]``
        meaning GP ``g`` did not observe row ``r`` (it then appends its own rows only).  The
        log ends up as after ``b`` calls of ``add_new_data_point``; every GP takes its rows
        by block appends of up to 16 rows (one O(b n^2) update each instead of ``b``), and
        the next ``optimize()`` of a ``SafeOpt`` corrects the resident posterior in ONE
        closed-form pass over the grid instead of sweeping it again.  ``noise_scale``: a
        scalar, one value per GP, or ``(b, n_gps)``.  With ``pool_repeats`` the rows whose
        input a GP holds (an earlier row of the batch included) are pooled one by one, the
        rest is block-appended."""
        X = np.atleast_2d(np.asarray(X, dtype=float))
        Y = np.atleast_2d(np.asarray(Y, dtype=float))
        if X.shape[0] != Y.shape[0] or Y.shape[1] != len(self.gps):
            raise ValueError("X (b, d) and Y (b, %d) expected, got %r and %r"
                             % (len(self.gps), X.shape, Y.shape))
        rho = self._scales_per_gp(noise_scale, X.shape[0])
        if self.num_contexts:
            X = _with_context(X, context)
        if self._pool is not None:
            # the batch's new inputs first (one block per GP), then the repeats row by row:
            # a repeat of a row of the same batch finds it in the GP
            acts = [self._pool.add(X[k], ~np.isnan(Y[k])) for k in range(X.shape[0])]
            for g, gp in enumerate(self.gps):
                new = [k for k, a in enumerate(acts) if a[g] is not None and a[g][0] == 'append']
                if new:
                    self._add_data_points(gp, X[new, :], Y[new][:, [g]],
                                          noise_scale=None if rho is None else rho[new, g])
                for k, a in enumerate(acts):
                    if a[g] is not None and a[g][0] == 'pool':
                        gp.pool_data(a[g][1], Y[k, g], 1.0 if rho is None else rho[k, g])
            self._log(X, Y, rho)
            return
        for i, gp in enumerate(self.gps):
            seen = ~np.isnan(Y[:, i])
            if seen.any():
                self._add_data_points(gp, X[seen, :], Y[seen][:, [i]],
                                      noise_scale=None if rho is None else rho[seen, i])
        self._log(X, Y, rho)

    def _remove_last_data_point(self, gp):
        """Drop the newest row of one GP (a one-row ``sgp_gp_pop``)."""
        if getattr(gp, '_r', None) is None:
            gp.set_XY(gp.X[:-1, :], gp.Y[:-1, :])
        else:
            gp.set_XY(gp.X[:-1, :], gp.Y[:-1, :], noise_scale=gp.noise_scale[:-1])

    def _unlog(self, index):
        self._x = np.delete(self._x, index, axis=0)
        self._y = np.delete(self._y, index, axis=0)
        if self._rho is not None:
            self._rho = np.delete(self._rho, index, axis=0)

    def _unpool(self, index):
        """``pool_repeats``: measurement ``index`` leaves the GPs -- taken back out of a row
        that keeps other measurements (``unpool_data``, with its value and scale from the
        log), the row removed otherwise."""
        where = self._pool.locate(index)
        for g, row in enumerate(where):
            if row is not None and self._pool.count[g][row] == 1 and self._pool.rows(g) < 2:
                raise ValueError("GP %d would be left without data" % g)
        for g, act in enumerate(self._pool.remove(index)):
            if act is None:
                continue
            if act[0] == 'unpool':
                self.gps[g].unpool_data(act[1], self._y[index, g],
                                        1.0 if self._rho is None else self._rho[index, g])
            else:
                self.gps[g].remove_data(act[1])

    def remove_last_data_point(self):
        """Undo the last ``add_new_data_point``: every GP that observed the
        newest measurement forgets it, then the log is shortened."""
        if self._pool is not None:
            self._unpool(self.t - 1)
            self._unlog(self.t - 1)
            return
        for gp, value in zip(self.gps, self._y[-1]):
            if not np.isnan(value):
                self._remove_last_data_point(gp)
        self._x, self._y = self._x[:-1, :], self._y[:-1, :]
        if self._rho is not None:
            self._rho = self._rho[:-1, :]

    def remove_data_point(self, index):
        """Forget measurement ``index`` of the log (``0 <= index < t``), whichever it is: a
        faulty reading, the oldest one of a sliding window.  Every GP that observed it drops
        it -- its row there is the number of measurements in front of ``index`` that the GP
        observed -- by an O(n^2) downdate of its factor (``GPRegression.remove_data``), and
        the next ``optimize()`` of a ``SafeOpt`` corrects the resident posterior in closed
        form instead of sweeping the grid again.  ``IndexError`` for an index outside the
        log, ``ValueError`` when a GP would be left without data; nothing has changed then.
        On N ranks nothing is different: the GPs are replicated, every rank makes the same
        call, and the correction of the posterior is local to the rows of a rank."""
        if isinstance(index, bool) or index != int(index) or not 0 <= index < self.t:
            raise IndexError("measurement %r of %d" % (index, self.t))
        index = int(index)
        if self._pool is not None:
            self._unpool(index)
            self._unlog(index)
            return
        seen = ~np.isnan(self._y[index])
        rows = [int(np.count_nonzero(~np.isnan(self._y[:index, i])))
                for i in range(len(self.gps))]
        for i, gp in enumerate(self.gps):
            if seen[i] and gp.X.shape[0] < 2:
                raise ValueError("GP %d would be left without data" % i)
        for i, gp in enumerate(self.gps):
            if seen[i]:
                gp.remove_data(rows[i])
        self._unlog(index)

    def loo_residuals(self):
        """Standardised leave-one-out residuals of the log, ``(t, n_gps)``: column ``g`` holds
        GP ``g``'s ``z = (y - mean_-i) / sqrt(var_-i)`` of every measurement it observed
        (``GPRegression.loo_residuals``, O(n^2) per GP from its resident factor), ``nan``
        where it did not.  Changes nothing in the optimiser.  With ``pool_repeats`` a
        measurement ``j`` (noise scale ``rho_j``) of a pooled row ``i`` (scale ``r_i``) is
        judged against the prediction that leaves the whole row out: ``z = (y_j - mean_-i) /
        sqrt(var_-i - s r_i + s rho_j)`` with ``s = noise_var + 1e-8`` -- the single reading,
        not the row's mean."""
        out = np.full(self._y.shape, np.nan)
        if self._pool is not None:
            for g, gp in enumerate(self.gps):
                mean, var = gp.loo()
                s, r = gp.noise_var + 1e-8, np.asarray(gp.noise_scale)
                for j in range(self.t):
                    row = self._pool.where[j][g]
                    if row is not None:
                        rho = 1.0 if self._rho is None else self._rho[j, g]
                        out[j, g] = ((self._y[j, g] - mean[row, 0])
                                     / np.sqrt(var[row, 0] - s * r[row] + s * rho))
            return out
        for g, gp in enumerate(self.gps):
            seen = ~np.isnan(self._y[:, g])
            out[seen, g] = gp.loo_residuals()[:, 0]
        return out

    def suspect_data_points(self, threshold=3.0):
        """Indices of the measurements that the other measurements do not explain:
        ``max_g |z| > threshold`` over the GPs' leave-one-out residuals, the largest first
        (ties by index).  Each can be passed straight to ``remove_data_point``.  Changes
        nothing in the optimiser."""
        z = np.abs(np.asarray(self.loo_residuals(), dtype=float))
        z = z.reshape(z.shape[0], -1)
        worst = np.max(np.where(np.isnan(z), -np.inf, z), axis=1) if z.size else np.zeros(0)
        order = np.lexsort((np.arange(worst.size), -worst))
        return [int(i) for i in order if worst[i] > threshold]


#: Hook of the CPU test-suite (tests/_oracle_backend.py): a callable ``(gps, rows of
#: this rank, global offset) -> backend`` that stands in for ``_HipGridBackend`` so the
#: sharded host logic can run without a GPU.  None in the product.
_BACKEND_FACTORY = None


class _WriteBackView(np.ndarray):
    """View of the host mirror of ``Q`` (or of ``S`` / ``M`` / ``G``) that remembers
    element-wise writes: the reference mutates these arrays in place
    (``gp_opt.py:374-390, 475-476, 481, 505-506, 511, 615``) and user code may do the same
    (``opt.Q[:, 0] = ...``, ``opt.S[:] = ...``); the optimiser uploads the mirror before
    the next device pass that reads it.  (Writes that bypass ``__setitem__`` --
    ``np.add(..., out=opt.Q)`` -- are not seen: assign ``opt.Q = array`` for those.)"""

    _owner = None
    _field = 'Q'

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, '_owner', None)
        self._field = getattr(obj, '_field', 'Q')

    def __setitem__(self, key, value):
        owner = self._owner() if self._owner is not None else None
        field = self._field
        # only writes that land IN the mirror count: a copy of opt.Q, or an array
        # computed from it, inherits this class but not the memory
        if owner is not None and np.may_share_memory(self, getattr(owner, '_' + field)):
            # the mirror may lag behind the device (a sweep since this view was
            # taken): bring it up to date first -- in the reference the array is live
            owner._mirror(field, getattr(_hip, field))
            np.ndarray.__setitem__(self, key, value)
            if field == 'Q':
                owner._q_written = True
            else:
                owner._masks_written.add(field)
        else:
            np.ndarray.__setitem__(self, key, value)


#: what the front half of ``compute_sets`` found (``SafeOpt._front_*``): counts of
#: candidates / unsafe rows over the whole grid, the first candidate in visiting order
#: (width, global index, its row, means, intervals), the probe flags + arg-max when they
#: came with it (``fused``), and the number of candidates tied with it (None: unknown)
_Front = collections.namedtuple(
    '_Front', 'n_cand n_unsafe w_c idx_c x_c mu_c q_c fused n_tied')

#: what one big pass of the expander loop found (``SafeOpt._pass_*``): candidates tested
#: (0 with a finite cut: counted by the histogram, not listed), the key and global row of the
#: first expander in visiting order (row -1: none), the cut in front of the next pass (-inf:
#: nothing left, the end of the loop), the step's arg-max (-1: unknown)
_Pass = collections.namedtuple('_Pass', 'tested key row left amax')


class _HipGridBackend(object):
    """Rank-local device state of a ``SafeOpt``: the shard of ``inputs`` in
    HBM plus the GP handles.  (Tests drive the same phase interface with a
    NumPy stand-in to exercise the sharded host logic without a GPU.)"""

    def __init__(self, gps, inputs_shard, global_offset, ctx=None, axes=None):
        # the grid must live in the context of its GPs (stream ordering, device
        # pointers) and of the communicator (in-stream collectives)
        gp_ctx = getattr(gps[0], '_ctx', None)
        self.ctx = ctx or gp_ctx or _hip.Context.default()
        if gp_ctx is not None and gp_ctx is not self.ctx:
            raise ValueError("the GPs live on HIP device %d but the communicator"
                             " / grid context is device %d"
                             % (gp_ctx.device, self.ctx.device))
        self.gps = gps
        self.grid = _hip.DeviceGrid(self.ctx, inputs_shard, len(gps),
                                    global_offset)
        #: the rows are a tensor grid (what linearly_spaced_combinations builds): RBF
        #: kernels are swept through per-axis factor tables
        self.tensor_grid = self.grid.set_axes(axes)
        self.lo = int(global_offset)
        self.hi = self.lo + self.grid.N
        # which data version of every GP the resident mean/var reflect
        self._seen = [None] * len(gps)
        self._rank1_streak = 0
        #: after one new observation update the resident posterior in closed
        #: form (O(n) per row) instead of re-running the O(n^2) sweep; a full
        #: sweep is forced every `refresh_every` updates to bound the drift
        self.incremental = True
        self.refresh_every = 16

    def _dev(self):
        return [g._fitted() for g in self.gps]

    def _tags(self, devs):
        # (serial number of the device GP, its data version): serials are never
        # reused, unlike id(), so a re-created handle cannot alias an old tag
        return [(dv.serial, dv.version) for dv in devs]

    def posterior_is_current(self):
        """Do the resident mean / var describe the GPs as they are now?"""
        return self._seen == self._tags(self._dev())

    def refresh_posterior(self):
        """Resident mean / var of every GP from a fresh sweep, ``Q`` and ``S``
        untouched (after ``opt.Q = ...`` or a data change without an interval
        update: the GP expander test reads mean / var, gp_opt.py:585-602)."""
        devs = self._dev()
        self.grid.posterior(devs)
        self._seen = self._tags(devs)
        self._rank1_streak = 0

    def owns(self, gidx):
        return self.lo <= gidx < self.hi

    def set_context(self, c):
        self.grid.set_context(c)
        self._seen = [None] * len(self.gps)      # rows changed: full sweep

    def confidence(self, beta, fmin, defer=False):
        devs = self._dev()
        tags = self._tags(devs)
        which = [0] * len(devs)
        rank1 = self.incremental
        kinds = set()                            # of the stale GPs' changes
        rows = 1                                 # rows the refresh absorbs (the drift budget)
        for i, dv in enumerate(devs):
            if self._seen[i] == tags[i]:
                continue                                  # up to date
            removed = getattr(dv, 'removed', False)
            block = getattr(dv, 'block', 0)
            reweighed = getattr(dv, 'reweighed', False)
            if (rank1 and (dv.appended or removed or block or reweighed)
                    and self._seen[i] is not None
                    and self._seen[i] == (dv.serial, dv.version - 1)):
                # one append / one removal / one block / one reweigh behind
                which[i] = 1
                kinds.add('block' if block else ('remove' if removed else
                                                 ('reweigh' if reweighed else 'append')))
                rows = max(rows, block)
            else:
                rank1 = False
        # (kinds mixed: a sweep; the streak counts absorbed rows, a block of b counts b)
        rank1 = (rank1 and len(kinds) == 1
                 and self._rank1_streak + rows <= self.refresh_every)
        self._seen = [None] * len(devs)          # unknown until the call is through
        if rank1 and any(which):
            refresh = getattr(self.grid, {'append': 'rank1_update', 'remove': 'rank1_remove',
                                          'reweigh': 'rank1_reweigh',
                                          'block': 'rankb_update'}[kinds.pop()])
            out = refresh(devs, which, beta, fmin, defer)
            self._rank1_streak += rows
        else:
            out = self.grid.confidence(devs, beta, fmin, defer)
            self._rank1_streak = 0
        self._seen = tags
        return out

    def upload_Q(self, Q, fmin):
        self._seen = [None] * len(self.gps)      # mean/var no longer match Q
        return self.grid.upload_Q(Q, fmin)

    def upload_mask(self, what, mask):
        self.grid.upload_mask(what, mask)

    def maximizers(self, max_l):
        return self.grid.maximizers(max_l)

    def candidates(self, max_var, scaling, thr_beta, full_sets):
        return self.grid.candidates(max_var, scaling, thr_beta, full_sets)

    def topk(self, mode, cut_w, cut_idx, k):
        return self.grid.topk(mode, cut_w, cut_idx, k)

    def gather_rows(self, gidx):
        return self.grid.gather_rows(gidx)

    def expander_check(self, beta, fmin, xc, mu_c, u_c, near_frac=0.0):
        return self.grid.expander_check(self._dev(), beta, fmin, xc, mu_c, u_c,
                                        near_frac)

    def lipschitz_check(self, fmin, lipschitz, xc, u_c):
        return self.grid.lipschitz_check(fmin, lipschitz, xc, u_c)

    def expander_batch(self, beta, fmin, mode, cut_w, cut_idx, k):
        return self.grid.expander_batch(self._dev(), beta, fmin, mode, cut_w, cut_idx, k)

    def expander_pass(self, beta, fmin, mode, cut_w, cut_idx, key_lo, key_hi, want,
                      scaling=None):
        return self.grid.expander_pass(self._dev(), beta, fmin, mode, cut_w, cut_idx,
                                       key_lo, key_hi, want, scaling)

    def lipschitz_pass(self, fmin, lipschitz, mode, cut_w, cut_idx, key_lo, key_hi, want,
                       scaling=None):
        return self.grid.lipschitz_pass(fmin, lipschitz, mode, cut_w, cut_idx, key_lo, key_hi,
                                        want, scaling)

    def pass_lipschitz_test(self, fmin, lipschitz, xc, u_c):
        return self.grid.pass_lipschitz_test(fmin, lipschitz, xc, u_c)

    def pass_hist(self, mode, cut_w, cut_idx, key_lo, key_hi):
        return self.grid.pass_hist(mode, cut_w, cut_idx, key_lo, key_hi)

    def pass_list(self, mode, cut_w, cut_idx, thr, cap):
        return self.grid.pass_list(mode, cut_w, cut_idx, thr, cap)

    def pass_test(self, beta, fmin, xc, resid):
        return self.grid.pass_test(self._dev(), beta, fmin, xc, resid)

    def small_grid(self):
        """At most 16384 rows and 48 observations per GP: every candidate can be tested at
        once (``sgp_grid_expanders_small``)."""
        return (self.grid.N <= 16384 and not getattr(self.ctx, 'sweep_forced', False)
                and all(g._fitted().n <= 48 for g in self.gps))

    def expanders_small(self, beta, fmin, gidx):
        return self.grid.expanders_small(self._dev(), beta, fmin, gidx)

    def expanders_small_all(self, beta, fmin, cap=4096):
        return self.grid.expanders_small_all(self._dev(), beta, fmin, cap)

    def mark_expanders(self, gidx):
        self.grid.mark_expanders(gidx)

    def unmark_expanders(self, gidx):
        self.grid.unmark_expanders(gidx)

    def candidate_widths(self):
        """This shard's candidate mask and ``max_i(u_i - l_i)`` per row."""
        return self.grid.download(_hip.CAND), self.grid.download(_hip.WIDTH)

    # fused passes (one stream sync each)
    def sets_front(self, max_l, max_var, scaling, thr_beta):
        return self.grid.sets_front(max_l, max_var, scaling, thr_beta)

    def sets_front_comm(self, scaling, thr_beta):
        return self.grid.sets_front_comm(scaling, thr_beta)

    def sets_fused(self, beta, fmin, max_l, scaling, thr_beta, near_frac):
        return self.grid.sets_fused(self._dev(), beta, fmin, max_l, scaling,
                                    thr_beta, near_frac)

    def sets_fused_comm(self, beta, fmin, scaling, thr_beta, near_frac):
        return self.grid.sets_fused_comm(self._dev(), beta, fmin, scaling,
                                         thr_beta, near_frac)

    #: budget of the one-launch step, in per-thread instructions of its posterior phase
    #: (~16 cycles each with two waves per SIMD): above it the nine launches of the
    #: large-grid path (~90 us whatever the grid) are the faster way
    SMALL_STEP_BUDGET = 5000

    def small_step_devs(self):
        """The fitted device GPs when a whole step of this grid is better taken in ONE
        launch (``sgp_grid_step_small``: at most 16384 rows, GPs with at most 48
        observations -- and few enough of both that one workgroup is through in ~30 us:
        the 1000-point grid with 20 observations of the reference's examples), else None."""
        N = self.grid.N
        if N > 16384 or getattr(self.ctx, 'sweep_forced', False):
            return None
        devs = [g._fitted() for g in self.gps]
        cost = 0
        for dv in devs:
            n = dv.n
            if n > 48:
                return None
            cost += n * (30 + n // 2)
        if -(-N // 512) * cost > self.SMALL_STEP_BUDGET:     # (512 threads: step_small.hip)
            return None
        return devs

    def step_small(self, devs, beta, fmin, scaling, thr_beta):
        self._seen = [None] * len(devs)          # unknown until the call is through
        out = self.grid.step_small(devs, beta, fmin, scaling, thr_beta)
        self._seen = self._tags(devs)            # (a full sweep: the posterior is current)
        self._rank1_streak = 0
        return out

    def sets_back(self, beta, fmin, xc, mu_c, u_c, near_frac, gidx_c, scaling,
                  mark):
        return self.grid.sets_back(self._dev(), beta, fmin, xc, mu_c, u_c,
                                   near_frac, gidx_c, scaling, mark)

    def argmax(self, mode, scaling):
        return self.grid.argmax(mode, scaling)

    def download(self, what):
        return self.grid.download(what)

    def batch(self, inputs, row0, size, mode, beta, scaling, want_var=False, comm=None):
        """The rows of a batch by hallucinated observations behind the pick ``row0`` of the
        real step (``SafeOpt.optimize_batch`` has the definition): private clones of the GPs,
        and per further pick one append of the pick before to every clone -- with ``y = 0``:
        only the variance is read -- and one ``sgp_grid_batch_next``.  ``inputs``: the rows
        of the WHOLE grid on the host (global row -> x).  Returns ``(rows, downdates,
        var_h)``: the global rows picked, how many of them the hallucinated variances
        ``var_h`` ``(G, N)`` account for (None without ``want_var``).  The user's GPs and the
        resident posterior, intervals and sets are only read; the clones are released on
        every way out.

        ``comm`` with ``world > 1`` (every rank makes the call): the grid is this rank's
        shard, every rank clones its own GPs and appends the same rows, and a pick is the
        best record ``{value, global row, stop}`` of all ranks -- ``_pick_over_ranks``: one
        collective per pick.  A rank whose append fails still takes part, with ``stop``:
        all ranks end the batch together.  ``var_h`` is gathered over the ranks in global
        row order."""
        world = 1 if comm is None else comm.world
        devs = self._dev()
        if not self.posterior_is_current():
            # (intervals assigned by hand, or data added since the last sweep: the downdates
            # start from the posterior of the GPs as they are)
            self.refresh_posterior()
        rows, downdates, clones = [int(row0)], 0, []
        try:
            for b in range(1, size):
                if not clones:
                    for dv in devs:
                        clones.append(dv.clone())
                x = np.asarray(inputs[rows[-1]], dtype=float)
                ok = all([c.append(x, 0.0) for c in clones])
                if not ok:
                    logging.getLogger(__name__).info(
                        "optimize_batch: pick %d (row %d) is determined to rounding by the "
                        "picks before it (non-positive pivot of the bordered append): the "
                        "batch ends with %d points", b - 1, rows[-1], len(rows))
                    if world == 1:
                        break
                if world == 1:
                    _v, i = self.grid.batch_next(clones, downdates == 0, mode, beta, scaling,
                                                 rows)
                else:
                    i, stop = self._pick_over_ranks(comm, clones, not ok, downdates == 0, mode,
                                                    beta, scaling, rows)
                    if stop:
                        downdates += int(ok)         # (this rank's var_h took the downdate)
                        break
                downdates += 1
                if i < 0:
                    break
                rows.append(int(i))
            var_h = None
            if want_var:
                var_h = self.grid.download(_hip.VAR_H if downdates else _hip.VAR)
                if world > 1:
                    var_h = gather_shard_columns(comm, var_h, inputs.shape[0])
        finally:
            for c in clones:
                c.destroy()
        return np.asarray(rows, dtype=np.int64), downdates, var_h

    def _pick_over_ranks(self, comm, clones, stop, first, mode, beta, scaling, rows):
        """One pick of a sharded batch, ``(global row, stop_any)``, the same on every rank.
        With an in-stream communicator ``sgp_grid_batch_next_comm``: the records are gathered
        and merged in the grid's stream, one device round trip.  Otherwise the shard's pick
        (``sgp_grid_batch_next``, none for a rank that stops), one ``allgather`` of the
        records and ``dist.merge_batch_records``: the same bits."""
        if getattr(comm, 'in_stream', False):
            _v, i, stop_any = self.grid.batch_next_comm(clones, first, mode, beta, scaling,
                                                        rows, stop=stop)
            return i, stop_any
        v, i = (-np.inf, -1) if stop else self.grid.batch_next(clones, first, mode, beta,
                                                               scaling, rows)
        rec = comm.allgather(np.array([v, float(i), float(stop)]))       # (rows < 2^53)
        _v, i, stop_any = merge_batch_records(rec)
        return i, stop_any

    def paths(self, pp, mask, values, comm=False):
        """Sample paths ``pp`` (of one of this backend's GPs) over the resident rows; ``comm``:
        the arg-max merged over the ranks in the grid's stream (``sgp_grid_paths_comm``)."""
        return self.grid.paths(pp.device, pp.Omega, pp.phase, pp.W, pp.V, mask=mask,
                               values=values, comm=comm)

    def mes(self, ystar, rows, floor, alpha=False, comm=False):
        """Max-value entropy search over the resident posterior of the objective
        (``DeviceGrid.mes``); the posterior is swept first when it is not that of the GPs as
        they are.  ``comm``: floor and arg-max merged over the ranks in the grid's stream
        (``sgp_grid_mes_comm``)."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        return self.grid.mes(ystar, rows=rows, floor=floor, alpha=alpha, comm=comm)

    def ei(self, kind, rows, tau, xi, fmin, alpha=False, comm=False):
        """Log expected improvement / log probability of improvement over the resident
        posterior (``DeviceGrid.ei``); the posterior is swept first when it is not that of
        the GPs as they are.  ``comm``: incumbent and arg-max merged over the ranks in the
        grid's stream (``sgp_grid_ei_comm``)."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        return self.grid.ei(kind=kind, rows=rows, tau=tau, xi=xi, fmin=fmin, alpha=alpha,
                            comm=comm)

    def ise_state(self):
        """What the host-side candidate selection of ``SafeOpt.ise_point`` reads, in one
        download each: the resident variances ``(G, N)``, the safe set ``(N,)`` and the
        GPs' measurement noise ``s_g = noise_var_g + 1e-8``; the posterior is swept first
        when it is not that of the GPs as they are."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        s = np.array([float(g.noise_var) + 1e-8 for g in self.gps])
        return (np.array(self.grid.download(_hip.VAR)),
                np.array(self.grid.download(_hip.S), dtype=bool), s)

    def ise(self, fmin, cand, about, pairs=False):
        """Information-theoretic safe exploration over the resident posterior
        (``DeviceGrid.ise``): ``(alpha (K,), target (K,), value, global row, pairs or None)``;
        the posterior is swept first when it is not that of the GPs as they are."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        al, tg, v, i, pr, _ = self.grid.ise(self._dev(), fmin, cand, about=about, pairs=pairs)
        return al, tg, v, i, pr

    def ise_at(self, fmin, cand, xc, vx, about, comm=False):
        """``ise`` with the candidates by value -- global rows of the WHOLE grid, their
        coordinates ``(K, d)`` and variances ``(G, K)`` -- over this shard's rows
        (``DeviceGrid.ise_at``): ``(alpha (K,), target (K,), value, global row)``.  ``comm``:
        merged over the ranks in the grid's stream (``sgp_grid_ise_comm``), a collective."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        return self.grid.ise_at(self._dev(), fmin, cand, xc, vx, about=about, comm=comm)

    # candidate selection of ise_point where the variances are (SafeOpt._ise_select)
    def ise_keys(self, fmin):
        """``(count, min key, max key)`` of this shard's safe rows; the posterior is swept
        first when it is not that of the GPs as they are."""
        if not self.posterior_is_current():
            self.refresh_posterior()
        return self.grid.ise_keys(self._dev(), fmin)

    def ise_hist(self, fmin, key_lo, key_hi):
        return self.grid.ise_hist(self._dev(), fmin, key_lo, key_hi)

    def ise_list(self, fmin, thr, cap):
        return self.grid.ise_list(self._dev(), fmin, thr, cap)

    def ise_noise(self):
        """``s_g = noise_var_g + 1e-8`` of the GPs, ``(G,)``."""
        return np.array([float(g.noise_var) + 1e-8 for g in self.gps])

    def ise_safe(self, gidx):
        """Which of the global rows ``gidx`` OF THIS SHARD are in ``S`` as it stands on the
        device."""
        S = np.array(self.grid.download(_hip.S), dtype=bool)
        return S[np.asarray(gidx, dtype=np.int64) - self.lo]


def ise_candidates(var, S, s, active, K):
    """The candidate rows of ``SafeOpt.ise_point``: the ``min(K, |S|)`` rows of ``S`` with the
    largest ``sum_{g active} log1p(var_g / s_g) / 2`` (added in the order of ``g``), the lower
    row first among equals.  ``var`` ``(G, N)``, ``S`` ``(N,)`` bool, ``s`` ``(G,)``, ``active``
    ``(G,)`` bool."""
    ids = np.flatnonzero(S)
    key = np.zeros(ids.size)
    for g in np.flatnonzero(active):
        key = key + 0.5 * np.log1p(var[g, ids] / s[g])
    K = int(K)
    if K < ids.size:
        # (only the rows at or above the K-th largest key can be picked: sort those)
        keep = key >= np.partition(key, ids.size - K)[ids.size - K]
        ids, key = ids[keep], key[keep]
    order = np.lexsort((ids, -key))[:K]
    return ids[order].astype(np.int64)


#: Bound on |device key - NumPy key| of an ``ise_point`` candidate, in units of ``max(1, largest
#: key)``, the rounding of the histogram's bin edges included: 64 ulp.  A term ``log1p(var / s) /
#: 2`` has the same quotient on both sides, a ``log1p`` within 2 ulp (device) and 1 ulp (host) of
#: the truth and an exact halving; the in-order sum over at most ``SGP_MAX_GPS`` = 8 such terms
#: adds half an ulp of the running sum per addition on either side -- below 3 + 8 ulp of the
#: key together, and the two roundings of ``(key - lo) * scale`` at a bin edge are 2 more.
#: tests/test_gpu_ise_select.py measures the key error and holds it below a quarter of this.
ISE_KEY_EPS = 2.0 ** -46
ISE_BINS = 4096


def ise_list_cap(K):
    """Rows the device selection of ``ise_point`` may list for ``K`` candidates before the host
    selection takes over (masses of equal keys)."""
    return 4 * int(K) + 4096


def ise_threshold(hist, want, lo, hi, nbins=ISE_BINS):
    """``(thr, listed)``: the key from which the candidates are listed and how many the
    histogram ``hist`` (``nbins`` bins over ``[lo, hi]``, summed over the ranks) counts there.
    ``b`` is the highest bin at which the count from the top reaches ``want``; the list starts
    at the lower edge of bin ``b - 1`` (``-inf`` for ``b <= 1``: everything).  With a bin wider
    than ``2 eps``, ``eps`` bounding |device key - host key|: at least ``want`` rows have a
    device key in the bins from ``b`` up, so a host key ``>= edge_b - eps``; the ``want``-th
    largest HOST key is therefore ``>= edge_b - eps``, every row at or above it -- its ties
    included -- has a device key ``>= edge_b - 2 eps >= edge_(b-1)`` and is listed."""
    from_top = np.cumsum(np.asarray(hist, dtype=np.float64)[::-1])
    b = nbins - 1 - int(np.argmax(from_top >= want))
    if b <= 1:
        return -np.inf, int(from_top[-1])
    return lo + (hi - lo) * (float(b - 1) / nbins), int(from_top[nbins - b])


def ise_order(gidx, var, s, active, K):
    """The exact ordering behind a device selection: positions, in pick order, of the
    ``min(K, m)`` listed rows (``gidx (m,)`` ascending, ``var (m, G)`` their resident variances)
    that ``ise_candidates`` takes -- NumPy keys, largest first, the lower row first among
    equals."""
    assert np.all(np.diff(gidx) > 0)
    return ise_candidates(np.ascontiguousarray(var.T), np.ones(gidx.size, dtype=bool), s, active,
                          K)


class SafeOpt(GaussianProcessOptimization):
    """Safe Bayesian optimisation over a discretised parameter set.

    Parameters
    ----------
    gp : GP handle or list of GP handles (``safeopt_amd.gpy``)
        First GP = objective, the others = safety constraints.
    parameter_set : 2d-array
        Candidate parameters, one per row (every rank passes the full set;
        each rank keeps its contiguous row block on its GPU).
    fmin : float or list of floats
        Safety thresholds (``-inf`` disables the constraint of a GP).
    lipschitz : float or list of floats, optional
    beta : float or callable ``beta(t)``
    num_contexts : int
    threshold : float or list of floats
    scaling : list of floats or ``'auto'``
    comm : communicator, optional
        ``safeopt_amd.dist.RcclComm`` for multi-GPU runs (default: 1 GPU).

    Examples
    --------
    >>> from safeopt_amd import SafeOpt, linearly_spaced_combinations
    >>> import safeopt_amd.gpy as GPy          # doctest: +SKIP
    >>> gp = GPy.models.GPRegression(np.array([[0.]]), np.array([[1.]]),
    ...                              noise_var=0.01**2)      # doctest: +SKIP
    >>> ps = linearly_spaced_combinations([[-1., 1.]], 100)
    >>> opt = SafeOpt(gp, ps, fmin=[0.])                      # doctest: +SKIP
    >>> x = opt.optimize()                                    # doctest: +SKIP
    >>> opt.add_new_data_point(x, np.array([[1.]]))           # doctest: +SKIP
    """

    def __init__(self, gp, parameter_set, fmin, lipschitz=None, beta=2,
                 num_contexts=0, threshold=0, scaling='auto', comm=None,
                 pool_repeats=False):
        super(SafeOpt, self).__init__(gp, fmin=fmin, beta=beta,
                                      num_contexts=num_contexts,
                                      threshold=threshold, scaling=scaling,
                                      pool_repeats=pool_repeats)
        # candidate rows = parameters (+ zeroed context columns that the context
        # setter fills); `parameter_set` stays a view of the parameter columns
        params = np.asarray(parameter_set)
        if self.num_contexts:
            self.inputs = np.hstack(
                (params, np.zeros((params.shape[0], self.num_contexts),
                                  dtype=params.dtype)))
            self.parameter_set = self.inputs[:, :params.shape[1]]
        else:
            self.inputs = self.parameter_set = params

        # attribute name as spelled by the reference (gp_opt.py:366)
        self.liptschitz = (None if lipschitz is None
                           else _one_per_gp(lipschitz, len(self.gps)))
        self._use_lipschitz = lipschitz is not None

        # host mirrors of the resident arrays, with the reference's dtypes and
        # shapes (gp_opt.py:374-390); refreshed from HBM only when read
        N = self.inputs.shape[0]
        self._Q = np.empty((N, 2 * len(self.gps)), dtype=float)
        self._S, self._M, self._G = (np.zeros(N, dtype=bool) for _ in range(3))
        self._stale = dict(Q=False, S=False, M=False, G=False)
        self._s_user = False       # the device's S was assigned by user code (opt.S[...] = ...)
        self._masks_written = set()
        self._q_written = False

        # this rank's contiguous block of rows, resident on its GPU
        self._comm = comm if comm is not None else LocalComm()
        if N < self._comm.world:
            # every rank owns at least one row (a shard without rows has no resident
            # state to launch on; raised on ALL ranks, before any collective)
            raise ValueError("parameter_set has %d rows for %d ranks" % (N, self._comm.world))
        self._shard = shard_range(N, self._comm.rank, self._comm.world)
        lo, hi = self._shard
        if _BACKEND_FACTORY is not None:          # CPU tests: NumPy stand-in
            self._backend = _BACKEND_FACTORY(self.gps, self.inputs[lo:hi], lo)
        else:
            self._backend = _HipGridBackend(self.gps, self.inputs[lo:hi], lo,
                                            ctx=getattr(self._comm, 'ctx', None),
                                            axes=_hip.tensor_grid_axes(self.inputs))
        # every rank must sweep with the same arithmetic (the N-rank run equals the one-rank
        # run bit for bit): a parameter set that is a tensor grid on some shards only -- the
        # device check is per shard -- is a tensor grid on none
        if self._comm.world > 1 and hasattr(self._backend, 'tensor_grid'):
            bad = self._comm.allreduce_max(
                np.array([0.0 if self._backend.tensor_grid else 1.0]))[0] > 0
            if bad and self._backend.tensor_grid:
                self._backend.grid.clear_axes()
                self._backend.tensor_grid = False
        self._any_safe = False
        self._max_l = -np.inf
        self._ci_fresh = False
        self._argmax_cache = None
        #: small grids with few observations take the whole step in one launch
        #: (``sgp_grid_step_small``); False keeps them on the large-grid path
        self.small_step = True
        self._thr_beta_key = self._thr_beta = None

    # -- host mirrors ---------------------------------------------------------
    def _mirror(self, name, what):
        if self._stale[name]:
            arr = getattr(self, '_' + name)
            part = self._backend.download(what)
            world = self._comm.world
            if world > 1:
                part = allgather_rows(self._comm, np.asarray(part, dtype=arr.dtype), [
                    hi - lo for lo, hi in (shard_range(arr.shape[0], r, world)
                                           for r in range(world))])
            np.copyto(arr, part)
            self._stale[name] = False
        # (the properties hand out write-back views of this array)
        return getattr(self, '_' + name)

    @property
    def Q(self):
        """Confidence intervals ``[l_0, u_0, l_1, u_1, ...]`` per row.  Writable:
        element-wise writes are uploaded before the next pass that reads them."""
        return self._view('Q', _hip.Q)

    def _view(self, name, what):
        view = self._mirror(name, what).view(_WriteBackView)
        view._owner = weakref.ref(self)
        view._field = name
        return view

    def _flush_Q(self):
        """Upload ``Q`` if user code wrote into the mirror since the last pass."""
        if self._q_written:
            self._q_written = False
            self.Q = self._Q.copy()

    @Q.setter
    def Q(self, value):
        """Assigning ``opt.Q`` uploads the intervals and recomputes ``S``."""
        value = np.asarray(value, dtype=float).reshape(self._Q.shape)
        lo, hi = self._shard
        m, a = self._backend.upload_Q(value[lo:hi], self.fmin)
        red = self._comm.allreduce_max(np.array([m, float(a)]))
        self._max_l, self._any_safe = red[0], bool(red[1] > 0)
        np.copyto(self._Q, value)
        self._q_written = False
        self._stale.update(Q=False, S=True)
        self._ci_fresh = True
        self._argmax_cache = None

    @property
    def S(self):
        """Safe set mask.  Writable like in the reference (``opt.S[:] = ...``): the next
        ``get_new_query_point`` reads the edited mask; ``compute_sets`` recomputes it from
        the intervals, as the reference's ``compute_safe_set`` does (gp_opt.py:478-481)."""
        return self._view('S', _hip.S)

    @property
    def M(self):
        """Potential maximisers mask (writable; ``compute_sets`` recomputes it)."""
        return self._view('M', _hip.M)

    @property
    def G(self):
        """Expanders mask (writable; ``compute_sets`` recomputes it)."""
        return self._view('G', _hip.G)

    def _flush_masks(self, for_sets=False):
        """Element-wise writes into ``opt.S / M / G`` since the last pass reach the device.
        ``for_sets``: ``compute_sets`` is about to overwrite M and G and recomputes S from
        the intervals (gp_opt.py:478-481, 505-615): an edited S is dropped, not uploaded."""
        written, self._masks_written = self._masks_written, set()
        if for_sets and (self._s_user or 'S' in written):
            # (an S that user code assigned -- now or before an earlier arg-max -- is
            # recomputed from the intervals, like compute_safe_set does in the reference)
            self._s_user = False
            self._argmax_cache = None
            self.Q = self._mirror('Q', _hip.Q).copy()
            return
        if not written:
            return
        self._argmax_cache = None
        if for_sets:
            return
        lo, hi = self._shard
        for name in sorted(written):
            self._backend.upload_mask(getattr(_hip, name), getattr(self, '_' + name)[lo:hi])
        if 'S' in written:
            self._any_safe = bool(self._S.any())
            self._s_user = True

    # -- reference properties ---------------------------------------------------
    @property
    def use_lipschitz(self):
        """True: expanders are certified with the Lipschitz constant, False:
        with the GP confidence intervals."""
        return self._use_lipschitz

    @use_lipschitz.setter
    def use_lipschitz(self, value):
        if value and self.liptschitz is None:
            raise ValueError('Lipschitz constant not defined')
        self._use_lipschitz = value

    @property
    def parameter_set(self):
        """Discrete parameter samples (without context columns)."""
        return self._parameter_set

    @parameter_set.setter
    def parameter_set(self, parameter_set):
        cols = parameter_set.T
        self._parameter_set = parameter_set
        self.bounds = [(c.min(), c.max()) for c in cols]
        self.num_samples = [np.unique(c).size for c in cols]

    def _context_columns(self):
        return self.inputs[0, self.inputs.shape[1] - self.num_contexts:]

    @property
    def context_fixed_inputs(self):
        """``[(column, value), ...]`` of the inputs the current context fixes
        (counted down from the last GP input, as the reference's plots expect)."""
        if self.num_contexts > 0:
            last = self.gp.input_dim - 1
            return [(last - k, v) for k, v in enumerate(self._context_columns())]

    @property
    def context(self):
        """Current context variables."""
        if self.num_contexts:
            return self._context_columns()

    @context.setter
    def context(self, context):
        if not self.num_contexts:
            return
        if context is None:
            raise ValueError('Need to provide value for context.')
        self.inputs[:, self.inputs.shape[1] - self.num_contexts:] = context
        self._backend.set_context(np.asarray(self._context_columns(), dtype=float))
        self._ci_fresh = False

    # -- the hot path -------------------------------------------------------------
    def update_confidence_intervals(self, context=None, _defer=False):
        """Posterior sweep of every GP over all candidates -> ``Q`` (and ``S``).

        One fused kernel per rank; the only values that come back are
        ``max(l_0[S])`` and ``any(S)``.  (``_defer``: internal to
        :meth:`optimize` -- the sweep is only enqueued and the two scalars
        arrive with the set passes, one device round trip for the whole step.)
        """
        beta = self.beta(self.t)
        self.context = context
        if _defer:
            m, a = self._backend.confidence(beta, self.fmin, defer=True)
        else:
            m, a = self._backend.confidence(beta, self.fmin)
        if m is None:
            self._max_l, self._any_safe = None, None      # known after the sets
        else:
            red = self._comm.allreduce_max(np.array([m, float(a)]))
            self._max_l, self._any_safe = red[0], bool(red[1] > 0)
        self._stale.update(Q=True, S=True)
        self._q_written = False          # (the sweep overwrites the intervals)
        self._s_user = False
        self._ci_fresh = True
        self._argmax_cache = None

    def compute_safe_set(self):
        """``S = all(l_i > fmin_i)``; fused into the sweep, nothing to redo."""
        self._flush_Q()
        self._flush_masks(for_sets=True)
        if not self._ci_fresh:
            self.update_confidence_intervals(context=self.context)

    def _sum_over_ranks(self, values):
        v = np.asarray(values, dtype=np.float64)
        return self._comm.allgather(v).sum(axis=0)

    def compute_sets(self, full_sets=False):
        """Maximisers ``M`` and expanders ``G`` from the current intervals.

        ``full_sets=True`` evaluates every safe point as an expander candidate
        (plotting mode of the reference).

        The common case -- GP certificates, not ``full_sets`` -- runs as a FRONT half
        (maximisers, candidate mask, the first candidate in visiting order) and the
        certification of that candidate; which entry points carry the front half depends
        on where the step runs (one method each):

        ==========================  =====================================================
        one rank                    ``_front_one_rank_fused``: both halves in one device
                                    round trip (``sgp_grid_sets_fused``)
        one rank, no GP active      ``_front_one_rank``
        N ranks, in-stream comm     ``_front_n_ranks_in_stream``: one round trip, merges on
                                    the device behind the collectives
        N ranks otherwise           ``_front_n_ranks_host``: packed host collectives
        ==========================  =====================================================
        """
        beta = self.beta(self.t)
        self.compute_safe_set()
        be = self._backend
        G = len(self.gps)
        # the GP expander test updates the RESIDENT posterior in closed form
        # (the reference re-predicts from the GP, gp_opt.py:585-602): bring it
        # up to date if the intervals were assigned by hand or the data changed
        if (not self.use_lipschitz and hasattr(be, 'posterior_is_current')
                and not be.posterior_is_current()):
            be.refresh_posterior()
        thr_beta = np.broadcast_to(
            np.asarray(self.threshold, dtype=float) * beta, (G,)).copy()

        self._argmax_cache = None
        if self._max_l is not None and not self._any_safe:
            # M = G = False everywhere
            be.maximizers(np.inf)
            be.candidates(np.inf, self.scaling, thr_beta, False)
            self._stale.update(M=True, G=True)
            return

        active = self.fmin != -np.inf
        world = self._comm.world
        if full_sets or self.use_lipschitz or not hasattr(be, 'sets_front'):
            return self._general_sets(beta, active, thr_beta, full_sets)
        if world == 1 and np.any(active) and hasattr(be, 'sets_fused'):
            front = self._front_one_rank_fused(beta, thr_beta)
        elif world == 1:
            front = self._front_one_rank(thr_beta)
        elif (self._max_l is None and np.any(active) and hasattr(be, 'sets_fused_comm')):
            front = self._front_n_ranks_in_stream(beta, thr_beta)
        else:
            front = self._front_n_ranks_host(thr_beta)
        if front is not None:                 # (None: no safe row, M = G = False)
            self._certify_first_candidate(beta, active, front)

    # -- the front half of compute_sets, one method per place the step runs ----------
    @staticmethod
    def _front_of(out5, x_c, mu_c, q_c, fused):
        return _Front(out5[1], out5[2], float(out5[3]), int(out5[4]), x_c, mu_c, q_c,
                      fused, int(out5[5]) if len(out5) > 5 else None)

    def _deferred_max_l(self, max_l):
        """``max l0[S]`` arrives with the front half after a deferred confidence pass;
        False when no row is safe (the passes ran with ``-inf``: ``M = G = False``)."""
        self._max_l, self._any_safe = max_l, bool(max_l > -np.inf)
        if not self._any_safe:
            self._stale.update(M=True, G=True)
        return self._any_safe

    def _front_one_rank_fused(self, beta, thr_beta):
        """One rank: both halves in one device round trip."""
        (out5, x_c, mu_c, q_c, f_flags, f_val, f_idx,
         max_l) = self._backend.sets_fused(beta, self.fmin, self._max_l, self.scaling,
                                           thr_beta, 0.5)
        if self._max_l is None and not self._deferred_max_l(max_l):
            return None
        return self._front_of(out5, x_c, mu_c, q_c, (f_flags, f_val, f_idx))

    def _front_one_rank(self, thr_beta):
        """One rank without an active GP certificate: the front half alone."""
        out5, x_c, mu_c, q_c = self._backend.sets_front(self._max_l, None, self.scaling,
                                                        thr_beta)
        return self._front_of(out5, x_c, mu_c, q_c, None)

    def _front_n_ranks_in_stream(self, beta, thr_beta):
        """N ranks behind a deferred confidence pass, communicator in stream: the whole
        certified step in one device round trip -- the first-candidate merge, the probe
        flags and the arg-max merge run on the device behind the collectives, every rank
        reads back the same (global) numbers (gp_opt.py:511-513, 542-557, 611-612, 642-644)."""
        (out5, x_c, mu_c, q_c, f_flags, f_val, f_idx,
         max_l) = self._backend.sets_fused_comm(beta, self.fmin, self.scaling, thr_beta, 0.5)
        if not self._deferred_max_l(max_l):
            return None
        return self._front_of(out5, x_c, mu_c, q_c, (f_flags, f_val, f_idx))

    def _front_n_ranks_host(self, thr_beta):
        """N ranks, collectives on the host side of the step: every rank's first candidate
        with its rows goes through one packed all-gather and is merged in NumPy."""
        be = self._backend
        d, G = self.inputs.shape[1], len(self.gps)
        if self._max_l is None:
            # deferred confidence pass: max l0 and the maximiser width
            # are all-reduced in stream, one round trip for this half
            out5, x_l, mu_l, q_l, max_l = be.sets_front_comm(self.scaling, thr_beta)
            if not self._deferred_max_l(max_l):
                return None
        else:
            width = self._comm.allreduce_max(np.array([be.maximizers(self._max_l)]))[0]
            out5, x_l, mu_l, q_l = be.sets_front(self._max_l, width / self.scaling[0],
                                                 self.scaling, thr_beta)
        tied_l = out5[5] if len(out5) > 5 else np.nan
        pk = self._comm.allgather(np.concatenate([out5[1:5], [tied_l], x_l, mu_l, q_l]))
        n_cand, n_unsafe = pk[:, 0].sum(), pk[:, 1].sum()
        w_b, i_b = merge_topk(pk[:, 2], pk[:, 3].astype(np.int64), 1)
        idx_c = int(i_b[0]) if i_b.size else -1
        w_c = float(w_b[0]) if i_b.size else -np.inf
        r = int(np.flatnonzero(pk[:, 3].astype(np.int64) == idx_c)[0]) if idx_c >= 0 else 0
        x_c, mu_c, q_c = pk[r, 5:5 + d], pk[r, 5 + d:5 + d + G], pk[r, 5 + d + G:]
        # candidates of ALL shards tied with the first one: a shard whose
        # own first candidate is narrower holds none of that width
        holds = (pk[:, 3] >= 0) & (pk[:, 2] == w_c)
        tied = pk[holds, 4].sum()
        return _Front(n_cand, n_unsafe, w_c, idx_c, x_c, mu_c, q_c, None,
                      None if np.isnan(tied) else int(tied))

    def _certify_first_candidate(self, beta, active, front, exact=False):
        """Second half, shared by every variant: is the first candidate an expander
        (gp_opt.py:579-612)?  ``front.fused``: the probe flags and the arg-max came with the
        front half (already global); otherwise ``sets_back`` runs them now.  ``exact``: the
        flags are those of the scan over ALL unsafe rows, not of the probe."""
        be = self._backend
        G = len(self.gps)
        world = self._comm.world
        n_cand, n_unsafe, w_c, idx_c, x_c, mu_c, q_c, fused, n_tied = front
        self._stale.update(M=True, G=True)
        if n_cand == 0 or n_unsafe == 0 or not np.any(active) or idx_c < 0:
            if fused is not None:       # G untouched: the arg-max over M holds
                self._argmax_cache = (fused[1], int(fused[2]))
            return
        if fused is not None:
            flags, val, idx = fused
        else:
            flags, val, idx = be.sets_back(beta, self.fmin, x_c, mu_c, q_c[1::2], 0.5,
                                           idx_c, self.scaling, world == 1)
        # N ranks without the fused step: flags and arg-max are merged here, and a certified
        # candidate is marked here (otherwise the device has marked it)
        host = world > 1 and fused is None
        if host:
            pk = self._comm.allgather(np.concatenate(
                [flags.astype(np.float64), [val, float(idx)]]))
            flags = pk[:, :G].max(axis=0)
        if np.all(flags[active] != 0):
            if host:
                # arg-max over M on every rank + the certified expander
                v_c = np.max((q_c[1::2] - q_c[::2]) / self.scaling)
                val, idx = merge_argmax(
                    np.append(pk[:, G], v_c),
                    np.append(pk[:, G + 1].astype(np.int64), idx_c))
            self._argmax_cache = (val, int(idx))
            self._first_expander(beta, active, w_c, idx_c, n_tied, mark=host)
            return
        self._visit_candidates(beta, active, False, w_c, idx_c, None if exact else front)

    def _general_sets(self, beta, active, thr_beta, full_sets):
        """Step by step (``full_sets``, Lipschitz certificates, backends without the fused
        passes): maximisers, candidate mask, then the expander loop from its start."""
        be = self._backend
        width = self._comm.allreduce_max(
            np.array([be.maximizers(self._max_l)]))[0]
        max_var = width / self.scaling[0]
        n_cand, n_unsafe = self._sum_over_ranks(
            be.candidates(max_var, self.scaling, thr_beta, full_sets))
        self._stale.update(M=True, G=True)

        if n_cand == 0 or n_unsafe == 0 or not np.any(active):
            # no candidate, or nothing unsafe to certify (any([]) is False),
            # or no safety constraint at all: G stays empty
            return
        self._visit_candidates(beta, active, full_sets, np.inf,
                               -1 if full_sets else _I64_MAX)

    def _visit_candidates(self, beta, active, full_sets, cut_w, cut_idx, first=None):
        """Expander loop of gp_opt.py:557-612 from the cut onwards; the one place that picks
        the loop.  ``first``: the candidate at the cut, which the probe did not certify and the
        exact scan has not tested.  The first matching rule decides:

        =  ==================================  ============================================
        1  ``first``, one rank, big passes,    big passes from ``(w_c, idx_c + 1)``: its
           finite width                        exact test rides in the first one
        2  ``first``                           its exact test; a hit ends the loop
        3  one rank, GP, ``small_step``,       ``_visit_all_candidates``
           ``small_grid()``
        4  big passes, ``full_sets`` or (one   big passes from the cut (``full_sets``:
           rank, finite cut)                   over every safe row)
        5  otherwise                           ``_visit_in_batches``, handing over to big
                                               passes after a batch of SGP_TOPK (one rank,
                                               Lipschitz: any batch) without an expander
        =  ==================================  ============================================

        Big passes: ``big_passes`` and ``expander_pass`` / ``lipschitz_pass`` on one rank,
        ``pass_test`` / ``pass_lipschitz_test`` on N ranks.  Batches: ``expander_batch`` on one
        rank with GP certificates, ``topk`` otherwise."""
        be, one, gp = self._backend, self._comm.world == 1, not self.use_lipschitz
        need = (('expander_pass' if gp else 'lipschitz_pass') if one
                else ('pass_test' if gp else 'pass_lipschitz_test'))
        big = ((self._pass_one_rank if one else self._pass_n_ranks)
               if self.big_passes and hasattr(be, need) else None)
        if first is not None:
            if one and big is not None and np.isfinite(cut_w):
                # a candidate that lifts no row close to it rarely lifts a far one, and a pass
                # costs little more than its scan
                return self._visit_in_big_passes(beta, active, False, cut_w, cut_idx + 1, big)
            if self._expander_flags(beta, first.x_c[None, :], first.mu_c[None, :],
                                    first.q_c[None, 1::2], active, probe=False)[0]:
                return self._first_expander(beta, active, cut_w, cut_idx, first.n_tied)
        if (one and gp and self.small_step and hasattr(be, 'expanders_small')
                and be.small_grid()):
            return self._visit_all_candidates(beta, active, full_sets, cut_idx)
        if big is not None and (full_sets or one and np.isfinite(cut_w)):
            # (behind a first candidate that is no expander: a pass of 256 candidates costs less
            # than the 16 of sgp_grid_expander_batch, whose scan knows neither the block test
            # nor the posterior Cauchy-Schwarz bound)
            return self._visit_in_big_passes(beta, active, full_sets, cut_w, cut_idx, big)
        batch = (self._batch_one_rank if one and gp and hasattr(be, 'expander_batch')
                 else self._batch_topk)
        return self._visit_in_batches(beta, active, full_sets, cut_w, cut_idx, batch, big,
                                      1 if one and not gp else _hip.TOPK)

    def _first_expander(self, beta, active, w, row, n_tied=None, mark=True):
        """First expander ``row`` of width ``w`` found: its owner marks it (``mark``; False:
        the device has), exact ties are settled.  Returns the row that ends up in ``G``."""
        if mark and self._backend.owns(row):
            self._backend.mark_expanders(np.array([row], dtype=np.int64))
        return self._settle_ties(beta, active, w, row, n_tied)

    def _visit_in_batches(self, beta, active, full_sets, cut_w, cut_idx, batch, big, big_after):
        """The loop K candidates in visiting order at a time (``batch``); the first hit ends it
        (``full_sets``: every hit is marked).  The first expander is very often the very first
        candidate: without a cut the first batch is that one alone, later ones SGP_TOPK.  A full
        batch of at least ``big_after`` candidates without a hit hands over to ``big``."""
        mode = 1 if full_sets else 0
        K = _hip.TOPK if (full_sets or cut_idx != _I64_MAX) else 1
        while True:
            w_b, i_b, is_exp, own = batch(beta, active, mode, cut_w, cut_idx, K)
            if i_b.size == 0:
                return
            if full_sets:
                self._backend.mark_expanders(i_b[is_exp & own])
            elif is_exp.any():
                first = int(np.argmax(is_exp))
                return self._first_expander(beta, active, float(w_b[first]), int(i_b[first]))
            if i_b.size < K:
                return
            cut_w, cut_idx = float(w_b[-1]), int(i_b[-1])
            if big is not None and K >= big_after:
                return self._visit_in_big_passes(beta, active, False, cut_w, cut_idx, big)
            K = _hip.TOPK

    def _batch_one_rank(self, beta, active, mode, cut_w, cut_idx, K):
        """Widths, rows, expander flags and ownership of the next K candidates: one rank, GP
        certificates, ONE device round trip (``sgp_grid_expander_batch``)."""
        w_b, i_b, fl = self._backend.expander_batch(beta, self.fmin, mode, cut_w, cut_idx, K)
        return w_b, i_b, np.all(fl[:, active] != 0, axis=1), True

    def _batch_topk(self, beta, active, mode, cut_w, cut_idx, K):
        """``_batch_one_rank`` step by step: every rank's next K candidates, merged; their rows
        from their owners; the test (the probe first, unless ``full_sets``)."""
        w_b, i_b = self._backend.topk(mode, cut_w, cut_idx, K)
        if self._comm.world > 1:
            wp = np.full(K, -np.inf)
            ip = np.full(K, -1, dtype=np.int64)
            wp[:w_b.size] = w_b
            ip[:i_b.size] = i_b
            w_b, i_b = merge_topk(self._comm.allgather(wp), self._comm.allgather(ip), K,
                                  by_index=mode == 1)
        if i_b.size == 0:
            return w_b, i_b, None, None
        xc, mu_c, u_c, own = self._candidate_rows(i_b)
        return w_b, i_b, self._expander_flags(beta, xc, mu_c, u_c, active, probe=mode == 0), own

    def _candidate_rows(self, gidx):
        """Rows, means and upper bounds of the global rows ``gidx`` on every rank: the owners
        fetch theirs, one all-gather sums them.  Also returns which of them this rank owns."""
        be, d, G = self._backend, self.inputs.shape[1], len(self.gps)
        own = np.array([be.owns(int(i)) for i in gidx])
        packed = np.zeros((gidx.size, d + 2 * G))
        if own.any():
            x_o, mean_o, _var_o, Q_o = be.gather_rows(gidx[own])
            packed[own, :d], packed[own, d:d + G], packed[own, d + G:] = x_o, mean_o, Q_o[:, 1::2]
        if self._comm.world > 1:
            packed = self._comm.allgather(packed).sum(axis=0)
        return packed[:, :d], packed[:, d:d + G], packed[:, d + G:], own

    #: candidates per big pass (the last entry repeats); None: by the number of observations
    #: (``_pass_size``)
    pass_sizes = None
    #: False: the expander loop of a large grid stays at SGP_TOPK candidates per round trip
    big_passes = True

    def _pass_size(self, k):
        """Candidates of pass k.  A pass costs a scan of the unsafe rows whatever its size
        (0.1-0.2 ms at 1e6 rows) plus the candidates' operands, 4 n^2 flop each: the first pass
        takes what keeps the operands at about 1e9 flop -- 8192 candidates up to n = 250, 1024
        at n = 640, 256 from n = 1000 on, so that an expander among the first candidates stays
        cheap to find --, the following ones 8 times as many each, up to 8192."""
        if self.pass_sizes is not None:
            return self.pass_sizes[min(k, len(self.pass_sizes) - 1)]
        if self.use_lipschitz:
            return 8192                 # (no operands: the distance test alone)
        n = max(int(gp.X.shape[0]) for gp in self.gps)
        first = 256
        while first < 8192 and 2 * first * n * n <= 5e8:
            first *= 2
        return min(8192, first * 8 ** min(k, 2))

    def _visit_in_big_passes(self, beta, active, full_sets, cut_w, cut_idx, step):
        """The expander loop of gp_opt.py:557-612 behind the cut where it goes far -- no
        expander among the first candidates (a converged run has none at all), or ``full_sets``
        (:553-555: every safe row is visited).  A pass (``step``: ``_pass_one_rank`` /
        ``_pass_n_ranks``) takes the next few hundred to few thousand candidates in visiting
        order (``pass_sizes``; chosen by a histogram of the keys, not a sort) and tests ALL of
        them in one scan of the unsafe rows: the first expander in visiting order is the widest
        hit of the first pass that has one -- every candidate in front of it has been tested --
        and exact ties among equal widths are settled as always.

        The loop ends when nothing is left behind the cut: ``left == -inf`` (the pass took
        everything, or its histogram was empty).  A pass that tested NOTHING although its
        histogram counted candidates is not the end: the histogram bins by a product, the list
        compares with the bin's lower edge, and a key an ulp below the edge is counted in the
        picked bin but not listed.  Such a pass reports its threshold as ``left``; with the cut
        and the top of the range moved there its keys fall into the top bin of the next pass,
        whose threshold lies at least a bin's width below them."""
        if full_sets:
            lo, hi, mode = -(float(self.inputs.shape[0]) + 1.0), 1.0, 1   # keys: minus the row
        else:
            lo, hi, mode = 0.0, float(cut_w), 0                            # keys: the widths
        for k in range(1 << 30):
            p = step(beta, active, mode, cut_w, cut_idx, lo, hi, self._pass_size(k))
            if p.row >= 0 and not full_sets:
                return self._first_expander(beta, active, p.key, p.row)
            if p.left == -np.inf:
                if p.amax >= 0 and p.tested > 0:
                    self._argmax_cache = (None, p.amax)
                return
            cut_w, cut_idx = p.left, -1
            if not full_sets or p.tested == 0:
                hi = p.left

    def _pass_one_rank(self, beta, active, mode, cut_w, cut_idx, lo, hi, want):
        """One big pass on one rank, one device round trip (``sgp_grid_expander_pass`` /
        ``sgp_grid_lipschitz_pass``; ``full_sets``: the device marks the hits).  The step's
        arg-max comes with a pass that ends the loop without an expander."""
        sc = None if mode else self.scaling
        if self.use_lipschitz:
            tested, hits, key, row, left, amax = self._backend.lipschitz_pass(
                self.fmin, self.liptschitz, mode, cut_w, cut_idx, lo, hi, want, sc)
        else:
            tested, hits, key, row, left, amax = self._backend.expander_pass(
                beta, self.fmin, mode, cut_w, cut_idx, lo, hi, want, sc)
        return _Pass(tested, key, row if hits else -1, left, amax)

    def _pass_n_ranks(self, beta, active, mode, cut_w, cut_idx, lo, hi, want, nbins=4096):
        """One big pass on a row-sharded grid.  The ranks sum their histograms of the keys
        behind the cut and pick ONE threshold (every rank computes the same one from the same
        sum); every rank lists its candidates above it and the lists are gathered -- the same
        candidates in the same order everywhere; every rank tests ALL of them against its own
        unsafe rows (the operands of the test are recomputed on every rank: a few MFLOP per
        candidate against the scan) and the flags are or-ed over the ranks (gp_opt.py:602:
        ``np.any`` over all unsafe rows).  Three small collectives per pass instead of three
        per 16 candidates.  ``full_sets``: the owners mark every hit."""
        be, comm = self._backend, self._comm
        d, G = self.inputs.shape[1], len(self.gps)
        hist = comm.allgather(be.pass_hist(mode, cut_w, cut_idx, lo, hi).astype(np.float64))
        from_top = np.cumsum(hist.sum(axis=0)[::-1])
        if from_top[-1] == 0:
            return _Pass(0, None, -1, -np.inf, -1)
        # the highest bin at which the count from the top reaches `want` (k_pass_pick)
        b = nbins - 1 - int(np.argmax(from_top >= want)) if from_top[-1] >= want else 0
        thr = -np.inf if b == 0 else lo + (hi - lo) * (float(b) / nbins)
        # (rounding at a bin edge can move a few candidates across it: room for the
        # bin below as well)
        cap = int(from_top[min(nbins - 1, nbins - b)] if b > 0 else from_top[-1]) + 64
        # (Lipschitz certificates: the candidates' upper bounds themselves, mode | 2)
        gi, key, xc, resid = be.pass_list(mode | (2 if self.use_lipschitz else 0), cut_w,
                                          cut_idx, thr, cap)
        part = np.empty((gi.size, 2 + d + G))
        part[:, 0], part[:, 1] = gi, key                        # (row indices < 2^53)
        part[:, 2:2 + d], part[:, 2 + d:] = xc, resid
        rows = allgather_rows(comm, part, count_dtype=np.float64)
        if rows.shape[0] == 0:
            # counted, not listed (keys an ulp below the edge of the picked bin): an empty
            # pass, not the end -- the loop goes on from the threshold
            return _Pass(0, None, -1, thr, -1)
        if self.use_lipschitz:
            flags = be.pass_lipschitz_test(self.fmin, self.liptschitz, rows[:, 2:2 + d],
                                           rows[:, 2 + d:])
        else:
            flags = be.pass_test(beta, self.fmin, rows[:, 2:2 + d], rows[:, 2 + d:])
        flags = comm.allreduce_max(flags.astype(np.float64)) > 0
        hits = np.all(flags[:, active], axis=1)
        gidx = rows[:, 0].astype(np.int64)
        if mode == 1:
            mine = [int(i) for i in gidx[hits] if be.owns(int(i))]
            for a in range(0, len(mine), 4096):
                be.mark_expanders(np.asarray(mine[a:a + 4096], dtype=np.int64))
        elif hits.any():
            hk, hg = rows[hits, 1], gidx[hits]
            first = np.lexsort((hg, hk))[-1]             # widest, then the larger row
            return _Pass(rows.shape[0], float(hk[first]), int(hg[first]), thr, -1)
        return _Pass(rows.shape[0], None, -1, thr, -1)

    def _visit_all_candidates(self, beta, active, full_sets, cut_idx, chunk=1024):
        """The expander loop of a SMALL grid on one rank: every candidate is tested at once
        (two launches, one round trip per ``chunk`` candidates) and the flags are walked in
        the reference's own visiting order -- ``argsort()[::-1]`` of the candidate widths
        (gp_opt.py:542-552), exact ties included, so nothing is left to settle.  ``cut_idx``:
        the first candidate of the device's order when it is already known to be no expander
        (it is skipped wherever the reference's order puts it)."""
        be = self._backend
        if not full_sets and hasattr(be, 'expanders_small_all'):
            # one round trip: the device lists the candidates in row order and tests ALL of
            # them; rows, widths and flags come back together (up to 4096 candidates)
            got = be.expanders_small_all(beta, self.fmin)
            if got is not None:
                rows, w_rows, flags = got
                order = w_rows.argsort()[::-1]         # (the reference's width[rows].argsort()[::-1])
                if 0 <= cut_idx < _I64_MAX:
                    order = order[rows[order] != cut_idx]
                is_exp = np.all(flags[order][:, active] != 0, axis=1)
                if is_exp.any():
                    be.mark_expanders(rows[order[int(np.argmax(is_exp))]][None])
                    self._argmax_cache = None
                return
        cand, width = be.candidate_widths()
        rows = np.flatnonzero(np.asarray(cand, dtype=bool))
        if full_sets:
            order = rows                                   # natural order, no early exit
        else:
            order = rows[np.asarray(width)[rows].argsort()[::-1]]
            if 0 <= cut_idx < _I64_MAX:
                order = order[order != cut_idx]
        for a in range(0, order.size, chunk):
            part = order[a:a + chunk]
            flags = be.expanders_small(beta, self.fmin, part)
            is_exp = np.all(flags[:, active] != 0, axis=1)
            if full_sets:
                be.mark_expanders(part[is_exp])
            elif is_exp.any():
                be.mark_expanders(part[int(np.argmax(is_exp))][None])
                self._argmax_cache = None
                return

    def _settle_ties(self, beta, active, w_star, idx_star, n_tied=None):
        """Exact ties in the visiting order of the expander loop.

        The device visits candidates by (width descending, index descending) and
        has just found its first expander ``idx_star`` of width ``w_star``.  The
        reference visits them in the order of ``widths.argsort()[::-1]``
        (gp_opt.py:542-552), which is the same except among candidates whose
        widths are EQUAL bit for bit -- NumPy's (unstable) sort decides there.
        Only when such a tie exists: take the candidate widths to the host, run
        the very same ``argsort()[::-1]`` on the very same values, and walk the
        tied group in that order -- members above ``idx_star`` were already
        rejected on the device, ``idx_star`` is an expander, the others are tested
        now; the first expander in THAT order is the one the reference marks.
        Returns the global index that ends up in ``G``.
        """
        be = self._backend
        if not hasattr(be, 'candidate_widths'):
            return idx_star
        if n_tied is None:
            # is the next candidate in the device's order tied with this one?
            w_loc, i_loc = be.topk(0, w_star, idx_star, 1)
            wp = np.full(1, -np.inf)
            wp[:w_loc.size] = w_loc[:1]
            n_tied = 2 if np.max(self._comm.allgather(wp)) == w_star else 1
        if n_tied <= 1:
            return idx_star
        # the candidate rows of the whole grid and their widths, in row order: what the
        # reference's ``width[rows]`` is.  N ranks exchange the CANDIDATES only (12 bytes
        # each), not the masks and widths of all rows (9 N bytes per shard)
        cand_loc, w_loc = be.candidate_widths()
        rows_loc = np.flatnonzero(np.asarray(cand_loc, dtype=bool))
        wc_loc = np.asarray(w_loc, dtype=float)[rows_loc]
        rows_loc = rows_loc + self._shard[0]
        if self._comm.world > 1:
            part = np.empty((rows_loc.size, 2))
            part[:, 0], part[:, 1] = rows_loc, wc_loc              # (idx < 2^53)
            part = allgather_rows(self._comm, part)
            rows, wrows = part[:, 0].astype(np.int64), part[:, 1]
        else:
            rows, wrows = rows_loc, wc_loc
        order = wrows.argsort()[::-1]              # the reference's own expression
        winner = idx_star
        for k in order:
            idx = int(rows[k])
            if wrows[k] != w_star or idx > idx_star:
                continue                           # other width / rejected before
            if idx == idx_star:
                break
            xc, mu_c, u_c, _own = self._candidate_rows(np.array([idx], dtype=np.int64))
            if self._expander_flags(beta, xc, mu_c, u_c, active, probe=False)[0]:
                winner = idx
                break
        if winner != idx_star:
            if be.owns(idx_star):
                be.unmark_expanders(np.array([idx_star], dtype=np.int64))
            if be.owns(winner):
                be.mark_expanders(np.array([winner], dtype=np.int64))
            self._argmax_cache = None
        return winner

    def _expander_flags(self, beta, xc, mu_c, u_c, active, probe):
        """Which of the candidates are expanders (all ranks agree).

        ``probe``: first scan only the rows strongly correlated with the
        candidate; a hit there already certifies it (``any`` over a subset).
        Only when the FIRST candidate in visiting order is not certified that
        way is the exact scan over all unsafe rows run.
        """
        be = self._backend

        def run(**kw):
            if self.use_lipschitz:
                f = be.lipschitz_check(self.fmin, self.liptschitz, xc, u_c)
            else:
                f = be.expander_check(beta, self.fmin, xc, mu_c, u_c, **kw)
            f = self._comm.allreduce_max(f.astype(np.float64)) > 0
            return np.all(f[:, active], axis=1)

        if probe and not self.use_lipschitz:
            hit = run(near_frac=0.5)
            if hit[0]:
                return hit
        return run()

    def get_new_query_point(self, ucb=False):
        """Next parameters to evaluate (first index wins among equals)."""
        self._flush_Q()
        self._flush_masks()
        if not self._any_safe:
            raise EnvironmentError('There are no safe points to evaluate.')
        mode = _hip.ARGMAX_UCB if ucb else _hip.ARGMAX_MG_WIDTH
        cached = getattr(self, '_argmax_cache', None)
        if not ucb and cached is not None:
            idx = cached[1]          # arg-max already done with the sets
        else:
            idx = self._global_argmax(mode)[1]
        x = self.inputs[idx, :]
        if self.num_contexts:
            return x[:-self.num_contexts]
        return x

    def _global_argmax(self, mode):
        v, i = self._backend.argmax(mode, self.scaling)
        if self._comm.world > 1:
            v, i = merge_argmax(self._comm.allgather(np.array([v])),
                                self._comm.allgather(np.array([i],
                                                              dtype=np.int64)))
        return v, int(i)

    def optimize(self, context=None, ucb=False):
        """One SafeOpt step: intervals -> sets -> next query point."""
        # common case on one GPU: sweep, set passes, probe of the first
        # candidate and arg-max are enqueued back to back, one read-back
        # (N ranks: the same deferral with the two scalar all-reduces in stream)
        one_trip = (not ucb and not self.use_lipschitz
                    and hasattr(self._backend, 'sets_fused')
                    and bool(np.any(self.fmin != -np.inf))
                    and (self._comm.world == 1
                         or getattr(self._comm, 'in_stream', False)))
        if (one_trip and self._comm.world == 1 and self.small_step
                and hasattr(self._backend, 'step_small')):
            devs = self._backend.small_step_devs()
            if devs is not None:
                # a small grid (the reference's own regime): the whole step is one launch
                self._small_step(context, devs)
                return self.get_new_query_point()
        self.update_confidence_intervals(context=context, _defer=one_trip)
        if ucb:
            self.compute_safe_set()
        else:
            self.compute_sets()
        return self.get_new_query_point(ucb=ucb)

    def _small_step_devs(self):
        """The fitted device GPs when ``optimize()`` (``ucb=False``) takes the one-launch
        step of a small grid, else None: the condition at the top of ``optimize``, which
        spells it out itself to keep a call off its 30-microsecond path (``SafeOptFleet``
        asks here which members ride its launch)."""
        if (not self.use_lipschitz and hasattr(self._backend, 'sets_fused')
                and bool(np.any(self.fmin != -np.inf))
                and self._comm.world == 1 and self.small_step
                and hasattr(self._backend, 'step_small')):
            return self._backend.small_step_devs()
        return None

    def _small_step(self, context, devs):
        """``update_confidence_intervals`` + ``compute_sets`` of a small grid in one launch
        and one read-back (``sgp_grid_step_small``: grids of at most 16384 rows, GPs with at
        most 48 observations -- gp_opt.py:651-675 as the reference's examples run it)."""
        beta = self._small_step_begin(context)
        self._small_step_end(beta, self._backend.step_small(devs, beta, self.fmin, self.scaling,
                                                            self._thr_beta))

    def _small_step_begin(self, context):
        """The host side of the one-launch step in front of the launch (shared with
        ``SafeOptFleet``, which launches many members at once); returns ``beta``."""
        beta = self.beta(self.t)
        if self.num_contexts:
            self.context = context
        thr = self.threshold
        key = (beta, thr if isinstance(thr, (int, float)) else tuple(np.ravel(thr)))
        if self._thr_beta_key != key:        # (constant for a constant beta: built once)
            self._thr_beta = np.broadcast_to(
                np.asarray(self.threshold, dtype=float) * beta, (len(self.gps),)).copy()
            self._thr_beta_key = key
        # element-wise edits of opt.S / M / G since the last pass are dropped, not uploaded:
        # the launch recomputes all three sets (gp_opt.py:478-481, 505-615), exactly as
        # _flush_masks(for_sets=True) does in front of compute_sets on the large-grid path
        self._masks_written = set()
        return beta

    def _small_step_end(self, beta, out):
        """... and behind it: ``out`` is what the backend's ``step_small`` returns."""
        out5, x_c, mu_c, q_c, flags, val, idx, max_l = out
        self._stale.update(Q=True, S=True)
        self._q_written = False          # (the sweep overwrites the intervals)
        self._s_user = False
        self._ci_fresh = True
        self._argmax_cache = None
        if self._deferred_max_l(max_l):
            self._certify_first_candidate(beta, self.fmin != -np.inf,
                                          self._front_of(out5, x_c, mu_c, q_c,
                                                         (flags, val, idx)), exact=True)

    def optimize_batch(self, size=8, context=None, ucb=False, return_state=False):
        """``k <= size`` query points from SafeOpt's own rule for experiments that run in
        parallel, spread out because every pick accounts for the ones before it: the GP-BUCB
        construction (Desautels et al. 2014) on SafeOpt.  The posterior variance depends on
        where one measures, not on what one measures, so a pending pick is "hallucinated"
        into the model: the means stay, the widths shrink around it.

        1. ``x_0 = self.optimize(context=context, ucb=ucb)``, the unchanged step: row 0 of
           the result is what ``optimize()`` returns, and the optimiser's state afterwards
           is the state after ``optimize()``.
        2. With ``mean_i``, ``var_i`` the resident posterior of GP ``i``,
           ``beta = self.beta(self.t)`` and ``var^0 = var``: for ``b = 1 .. size - 1`` and
           EVERY GP ``i`` (``add_new_data_point`` feeds all of them),
           ``var^b_i(x) = max(var^{b-1}_i(x) - c_i(x)^2 / s2_i, 1e-15)``, where ``c_i(x)`` is
           the posterior covariance of GP ``i`` between row ``x`` and ``x_{b-1}`` given the
           real data and the hallucinated inputs ``x_0 .. x_{b-2}``, and
           ``s2_i = c_i(x_{b-1}) + noise_i + 1e-8``.  Hallucinated intervals:
           ``l = mean - beta sqrt(var^b)``, ``u = mean + beta sqrt(var^b)``.
        3. ``x_b`` = the row that maximises, among the rows not picked before in this call
           (picks are distinct rows by construction; the lowest row wins among equal values):
           ``max_i (u_i - l_i) / scaling_i`` over the rows of ``M | G`` (``ucb=False``), or
           ``u_0`` over the rows of ``S`` (``ucb=True``).
        4. The batch ends early, with ``k < size`` rows, when no eligible row is left, or when
           the bordered append of a hallucinated point meets a non-positive pivot (the point
           is determined to rounding already; logged at ``logging.INFO``, not an error).

        Safety is untouched: ``S``, ``M``, ``G`` and every bound compared with ``fmin`` are
        those of the real data; hallucinated widths only rank rows inside sets the real data
        certified.  Nothing real changes: ``Q / S / M / G``, the resident posterior and the
        GPs are the bits ``optimize()`` left (the points are appended to private device
        copies of the GPs), so ``add_new_data_point`` + ``optimize()`` afterwards give what
        they give after a plain ``optimize()``.  An ``opt.Q`` edited by hand influences step 1
        and the sets only: the hallucinated intervals are built from the posterior of the GPs.

        Returns ``X (k, d_parameters)``, context columns stripped as ``optimize()`` strips
        them; with ``return_state=True`` ``(X, rows (k,) int64, var_h (G, N))``: the global
        rows picked and the hallucinated variances after the last downdate (tests, plots).
        ``size`` above ``SGP_MAX_BATCH`` (64) raises ``ValueError``.

        N ranks (SPMD, as ``optimize()``: the same data and the same call on every rank):
        every rank clones its own device GPs, appends the same picks to them and downdates
        the variances of its shard; a pick is the best row of all shards -- one collective of
        one record ``{value, global row, stop}`` per rank and pick: gathered and merged in
        the grid's stream with an in-stream communicator (``sgp_grid_batch_next_comm``, one
        device round trip per pick), else by one ``allgather`` and
        ``dist.merge_batch_records``.  Both give the bits of the one-rank run, on every rank:
        ``X``, ``rows`` (global) and ``var_h`` (gathered, ``(G, N)`` in global row order).
        The batch ends early on every rank at once: no eligible row on any shard, or a
        non-positive pivot on any rank (``stop``; that rank still takes part in the
        collective).  A communicator of several ranks without a device context
        (``comm.ctx``) cannot run the clones' appends next to its grid: there
        ``optimize_batch`` runs on one rank only and raises ``NotImplementedError`` before
        anything runs."""
        size = int(size)
        if size < 1 or size > _hip.MAX_BATCH:
            raise ValueError("size must be in 1 .. SGP_MAX_BATCH = %d, got %d"
                             % (_hip.MAX_BATCH, size))
        world = self._comm.world
        if world > 1 and getattr(self._comm, 'ctx', None) is None:
            raise NotImplementedError(
                "optimize_batch runs on one rank unless the communicator carries a device "
                "context (this communicator of %d ranks has no ctx)" % world)
        if not hasattr(self._backend, 'batch'):
            raise NotImplementedError("this grid backend hallucinates no observations")
        x0 = self.optimize(context=context, ucb=ucb)
        mode = _hip.ARGMAX_UCB if ucb else _hip.ARGMAX_MG_WIDTH
        cached = self._argmax_cache
        # (the row of x_0: the arg-max optimize() took -- its cache, or the same pass again,
        # merged over the ranks)
        row0 = cached[1] if (not ucb and cached is not None) else self._global_argmax(mode)[1]
        rows, _downdates, var_h = self._backend.batch(
            self.inputs, row0, size, mode, self.beta(self.t), self.scaling,
            want_var=return_state, **({'comm': self._comm} if world > 1 else {}))
        X = self.inputs[rows, :self.inputs.shape[1] - self.num_contexts]
        X[0] = x0
        return (X, rows, var_h) if return_state else X

    def thompson_points(self, size=8, features=1024, within='safe', return_values=False):
        """``size`` Thompson picks: sample paths of the objective GP (``gps[0]``,
        ``GPRegression.posterior_paths(size, features)``) evaluated over the whole resident
        grid, and per path the row that maximises it inside the current safe set ``S`` -- a
        batch of distinct-by-chance safe query points for experiments that run in parallel.

        Returns ``(x (size, d_parameters), values (size,))``: the maximisers, context columns
        stripped as ``optimize()`` strips them, and the paths' values there; with
        ``return_values=True`` also the ``(N, size)`` array of all path values.
        ``within='all'`` ignores ``S``: the arg-max over every row -- NOT a safe pick, for
        diagnostics and unconstrained problems only.  Raises ``RuntimeError`` when no row is
        safe.  Changes no state of the optimiser -- except that in-place edits
        of ``opt.Q`` / ``opt.S`` still pending are flushed to the device first, as before a
        set pass (an edited ``Q`` is uploaded and ``S`` recomputed from it); the random
        numbers come from NumPy's global generator.

        N ranks (SPMD, as ``optimize()``: the same seed and the same call on every rank):
        every rank draws the same paths -- the draws of one rank, so NumPy's generator ends
        where the one-rank run leaves it; one ``allreduce_max`` of a digest verifies it and
        raises ``ValueError`` on every rank otherwise -- and evaluates them over its shard.
        The per-path maxima are merged over the ranks, the lowest global row among equal
        values: in the grid's stream with an in-stream communicator
        (``sgp_grid_paths_comm``, one device round trip), else by one all-gather of the
        ranks' records and ``dist.merge_path_records``; both give the bits of the one-rank
        run, on every rank.  ``return_values=True`` gathers the ``(N, size)`` array in
        global row order on every rank.  "No row is safe" raises on every rank, after the
        collective."""
        if within not in ('safe', 'all'):
            raise ValueError("within must be 'safe' or 'all', got %r" % (within,))
        comm = self._comm
        world = comm.world
        if world > 1 and not all(callable(getattr(comm, f, None))
                                 for f in ('allreduce_max', 'allgather')):
            raise NotImplementedError(
                "thompson_points on more than one rank merges the ranks' picks through the "
                "communicator's allreduce_max and allgather: this communicator of %d ranks "
                "implements neither" % world)
        if not hasattr(self._backend, 'paths'):
            raise NotImplementedError("this grid backend evaluates no sample paths")
        self._flush_Q()
        self._flush_masks()
        safe = within == 'safe'
        # (N ranks: raised behind the collective, where every rank is sure to arrive)
        if world == 1 and safe and self._any_safe is not None and not self._any_safe:
            raise RuntimeError('There are no safe points to sample in.')
        pp = self.gp.posterior_paths(size=size, features=features)
        if world == 1:
            values, best, idx = self._backend.paths(pp, safe, return_values)
        else:
            check_same_paths(comm, pp)
            if getattr(comm, 'in_stream', False):
                values, best, idx = self._backend.paths(pp, safe, return_values, comm=True)
            else:
                values, bv, bi = self._backend.paths(pp, safe, return_values)
                rec = np.empty((2, bv.shape[0]))
                rec[0], rec[1] = bv, bi                           # (rows < 2^53)
                rec = comm.allgather(rec)
                best, idx = merge_path_records(rec[:, 0], rec[:, 1].astype(np.int64))
            if return_values:
                N = self.inputs.shape[0]
                values = allgather_rows(comm, values, [
                    hi - lo for lo, hi in (shard_range(N, r, world) for r in range(world))])
        if np.any(idx < 0):
            raise RuntimeError('There are no safe points to sample in.')
        x = self.inputs[idx, :self.inputs.shape[1] - self.num_contexts]
        return (x, best, values) if return_values else (x, best)

    def mes_point(self, paths=16, features=1024, within='safe', floor='mean',
                  return_values=False):
        """The safe row whose measurement tells most about the VALUE of the safe optimum:
        max-value entropy search (Wang & Jegelka 2017) inside the safe set.

        ``paths`` sample paths of the objective GP (``gps[0]``, ``posterior_paths(paths,
        features)``) give ``paths`` draws ``ystar`` of the maximum over ``S`` (their maxima
        over the resident grid, as ``thompson_points`` takes them); with ``mu``, ``v`` the
        resident posterior of the objective, ``sigma = sqrt(max(v, 1e-15))``,
        ``y_k = max(ystar_k, floor)`` and ``gamma_k = (y_k - mu) / sigma``,

            ``alpha(x) = mean_k [gamma_k phi(gamma_k) / (2 Phi(gamma_k)) - ln Phi(gamma_k)]``,

        and the pick is the row of ``S`` with the largest ``alpha`` (the lowest row among
        equals).  One pass over the resident rows on the device, finite for every ``gamma``.
        It needs no Lipschitz constant and no width rule, and it stops sampling the
        incumbent, which UCB and Thompson picks do not.

        ``floor='mean'`` (default): the largest posterior mean over ``S``.  A path maximum
        slightly below the mean -- the paths' prior term is approximate, and the maximum is
        taken over ``S`` only -- would make ``gamma`` negative where the mean is high, and the
        pick would collapse onto the incumbent with the smallest ``sigma``; with the floor
        ``gamma >= 0`` on every candidate.  ``floor=None``: none; a float: that value.

        ``within='safe'``: candidates ``S``.  ``'MG'``: candidates ``M | G`` as they stand --
        call it after ``optimize()`` / ``compute_sets()``, which compute them; maxima and
        floor are still those of ``S``.  ``'all'``: no mask for maxima, floor and candidates
        -- NOT a safe pick, for diagnostics and unconstrained problems only.

        Returns ``(x, alpha)``: the row, context columns stripped as ``optimize()`` strips
        them, and its ``alpha``; with ``return_values=True`` ``(x, alpha, values (N,),
        ystar (paths,))``: ``alpha`` of every row and the maxima used.  Raises
        ``RuntimeError`` when no row qualifies.  Changes no state of the optimiser or its
        GPs -- except that pending in-place edits of ``opt.Q`` / ``opt.S`` are flushed first,
        as before a set pass, and that the resident posterior is swept again if data came
        in since the last interval update; the random numbers come from NumPy's global
        generator.

        N ranks (SPMD, as ``thompson_points``: the same seed and the same call on every
        rank, verified by its digest check): maxima, floor and pick are those of all
        shards -- merged in the grid's stream with an in-stream communicator
        (``sgp_grid_paths_comm``, ``sgp_grid_mes_comm``), else through ``allreduce_max`` of
        the floor (one extra pass over the shard with one maximum finds the shard's), one
        ``allgather`` of the ranks' records and ``dist.merge_mes_records``; both give the
        bits of the one-rank run, on every rank.  ``values`` is gathered in global row
        order.  "No row qualifies" raises on every rank, behind the collective."""
        if within not in ('safe', 'MG', 'all'):
            raise ValueError("within must be 'safe', 'MG' or 'all', got %r" % (within,))
        paths = int(paths)
        if paths < 1 or paths > _hip.MAX_MES:
            raise ValueError("paths must be in 1 .. SGP_MAX_MES = %d, got %d"
                             % (_hip.MAX_MES, paths))
        if isinstance(floor, str):
            if floor != 'mean':
                raise ValueError("floor must be 'mean', None or a float, got %r" % (floor,))
        elif floor is not None:
            floor = float(floor)
            if np.isnan(floor):
                raise ValueError("floor is NaN")
        comm = self._comm
        world = comm.world
        if world > 1 and not all(callable(getattr(comm, f, None))
                                 for f in ('allreduce_max', 'allgather')):
            raise NotImplementedError(
                "mes_point on more than one rank merges the ranks' picks through the "
                "communicator's allreduce_max and allgather: this communicator of %d ranks "
                "implements neither" % world)
        if not (hasattr(self._backend, 'paths') and hasattr(self._backend, 'mes')):
            raise NotImplementedError("this grid backend runs no max-value entropy search")
        self._flush_Q()
        self._flush_masks()
        safe = within != 'all'
        rows = {'safe': _hip.MES_S, 'MG': _hip.MES_MG, 'all': _hip.MES_ALL}[within]
        # (N ranks: raised behind the collective, where every rank is sure to arrive)
        if world == 1 and safe and self._any_safe is not None and not self._any_safe:
            raise RuntimeError('There are no safe points to sample in.')
        pp = self.gp.posterior_paths(size=paths, features=features)
        in_stream = world > 1 and getattr(comm, 'in_stream', False)
        if world == 1:
            _, ystar, at = self._backend.paths(pp, safe, False)
        else:
            check_same_paths(comm, pp)
            if in_stream:
                _, ystar, at = self._backend.paths(pp, safe, False, comm=True)
            else:
                _, bv, bi = self._backend.paths(pp, safe, False)
                rec = np.empty((2, bv.shape[0]))
                rec[0], rec[1] = bv, bi                           # (rows < 2^53)
                rec = comm.allgather(rec)
                ystar, at = merge_path_records(rec[:, 0], rec[:, 1].astype(np.int64))
        if np.any(at < 0):
            raise RuntimeError('There are no safe points to sample in.')
        if world == 1 or in_stream:
            values, alpha, idx, _floor = self._backend.mes(ystar, rows, floor, return_values,
                                                           comm=world > 1)
        else:
            if floor == 'mean':
                # the shard's floor from a pass with one maximum, then the ranks' largest
                floor = self._backend.mes(ystar[:1], rows, 'mean')[3]
                floor = float(comm.allreduce_max(np.array([floor]))[0])
            values, v, i, _floor = self._backend.mes(ystar, rows, floor, return_values)
            alpha, idx = merge_mes_records(comm.allgather(np.array([v, float(i)])))
        if world > 1 and return_values:
            N = self.inputs.shape[0]
            values = allgather_rows(comm, values, [
                hi - lo for lo, hi in (shard_range(N, r, world) for r in range(world))])
        if idx < 0:
            raise RuntimeError('There are no safe points to sample in.')
        x = self.inputs[idx, :self.inputs.shape[1] - self.num_contexts]
        return (x, alpha, values, ystar) if return_values else (x, alpha)

    def ei_point(self, incumbent='mean', xi=0.0, within='safe', kind='ei', feasibility=False,
                 return_values=False):
        """The safe row with the largest expected improvement over the incumbent, evaluated
        as a logarithm (LogEI: Ament et al. 2023).

        With ``mu_g``, ``v_g`` the resident posterior of GP ``g`` (the objective is GP 0),
        ``sigma_g = sqrt(max(v_g, 1e-15))``, the incumbent ``tau`` and
        ``z = (mu_0 - tau - xi) / sigma_0``,

            ``kind='ei'``: ``alpha(x) = ln sigma_0 + ln(phi(z) + z Phi(z))``  (= ln EI),
            ``kind='pi'``: ``alpha(x) = ln Phi(z)``  (= ln of the probability of improvement),

        and the pick is the row of ``S`` with the largest ``alpha`` (the lowest row among
        equals).  One pass over the resident rows on the device.  On a converged run --
        ``sigma`` tiny, the incumbent far above most safe rows -- EI itself underflows to 0 on
        almost every row and its arg-max is "the lowest row among equals"; ``alpha`` stays
        finite and ordered there.

        ``incumbent='mean'`` (default): the largest posterior mean over ``S``; ``'data'``:
        the largest measured objective value, ``max(opt.y[:, 0])``; a finite float: that
        value.  ``xi >= 0``: the margin an improvement has to exceed.

        ``feasibility=True``: every GP with a finite ``fmin`` adds ``ln Phi((mu_g - fmin_g) /
        sigma_g)``, the log probability that its constraint holds (EIC: Gelbart et al. 2014,
        Gardner et al. 2014).

        ``within='safe'``: candidates ``S``.  ``'MG'``: candidates ``M | G`` as they stand --
        call it after ``optimize()`` / ``compute_sets()``, which compute them; the incumbent
        of ``'mean'`` is still that of ``S``.  ``'all'``: no mask for incumbent and candidates
        -- NOT a safe pick; with ``feasibility=True`` it is the EIC baseline the safe-BO
        papers compare against, for diagnostics and unconstrained problems only.

        Returns ``(x, alpha)``: the row, context columns stripped as ``optimize()`` strips
        them, and its ``alpha``; with ``return_values=True`` ``(x, alpha, values (N,),
        tau)``: ``alpha`` of every row and the incumbent used.  Raises ``RuntimeError`` when
        no row qualifies.  Changes no state of the optimiser or its GPs -- except that
        pending in-place edits of ``opt.Q`` / ``opt.S`` are flushed first, as before a set
        pass, and that the resident posterior is swept again if data came in since the last
        interval update.  Draws no random numbers.

        N ranks (SPMD: the same call on every rank): incumbent and pick are those of all
        shards -- merged in the grid's stream with an in-stream communicator
        (``sgp_grid_ei_comm``), else through ``allreduce_max`` of the shard's incumbent (one
        extra pass over the shard finds it), one ``allgather`` of the ranks' records and
        ``dist.merge_mes_records``; both give the bits of the one-rank run, on every rank.
        ``values`` is gathered in global row order.  "No row qualifies" raises on every rank,
        behind the collective."""
        if within not in ('safe', 'MG', 'all'):
            raise ValueError("within must be 'safe', 'MG' or 'all', got %r" % (within,))
        if kind not in ('ei', 'pi'):
            raise ValueError("kind must be 'ei' or 'pi', got %r" % (kind,))
        xi = float(xi)
        if not (np.isfinite(xi) and xi >= 0.0):
            raise ValueError("xi must be finite and >= 0, got %r" % (xi,))
        if isinstance(incumbent, str):
            if incumbent not in ('mean', 'data'):
                raise ValueError("incumbent must be 'mean', 'data' or a float, got %r"
                                 % (incumbent,))
            tau = 'mean'
            if incumbent == 'data':
                seen = self.y[:, 0][~np.isnan(self.y[:, 0])]
                if seen.size == 0:
                    raise ValueError("incumbent='data': the objective has no measurement")
                tau = float(seen.max())
        else:
            tau = float(incumbent)
        if tau != 'mean' and not np.isfinite(tau):
            raise ValueError("the incumbent must be finite, got %r" % (tau,))
        comm = self._comm
        world = comm.world
        if world > 1 and not all(callable(getattr(comm, f, None))
                                 for f in ('allreduce_max', 'allgather')):
            raise NotImplementedError(
                "ei_point on more than one rank merges the ranks' picks through the "
                "communicator's allreduce_max and allgather: this communicator of %d ranks "
                "implements neither" % world)
        if not hasattr(self._backend, 'ei'):
            raise NotImplementedError("this grid backend runs no expected improvement")
        self._flush_Q()
        self._flush_masks()
        safe = within != 'all'
        rows = {'safe': _hip.MES_S, 'MG': _hip.MES_MG, 'all': _hip.MES_ALL}[within]
        code = _hip.EI_EI if kind == 'ei' else _hip.EI_PI
        fmin = np.asarray(self.fmin, dtype=float).reshape(-1) if feasibility else None
        # (N ranks: raised behind the collective, where every rank is sure to arrive)
        if world == 1 and safe and self._any_safe is not None and not self._any_safe:
            raise RuntimeError('There are no safe points to sample in.')
        be = self._backend
        if world == 1 or getattr(comm, 'in_stream', False):
            values, alpha, idx, tau = be.ei(code, rows, tau, xi, fmin, return_values,
                                            comm=world > 1)
        else:
            if tau == 'mean':
                # the shard's incumbent from a pass of its own, then the ranks' largest
                tau = be.ei(code, rows, 'mean', xi, fmin)[3]
                tau = float(comm.allreduce_max(np.array([tau]))[0])
            if tau == -np.inf:                       # no rank has a safe row
                lo, hi = shard_range(self.inputs.shape[0], comm.rank, world)
                values = np.full(hi - lo, -np.inf) if return_values else None
                v, i = -np.inf, -1
            else:
                values, v, i, _tau = be.ei(code, rows, tau, xi, fmin, return_values)
            alpha, idx = merge_mes_records(comm.allgather(np.array([v, float(i)])))
        if world > 1 and return_values:
            N = self.inputs.shape[0]
            values = allgather_rows(comm, values, [
                hi - lo for lo, hi in (shard_range(N, r, world) for r in range(world))])
        if idx < 0:
            raise RuntimeError('There are no safe points to sample in.')
        x = self.inputs[idx, :self.inputs.shape[1] - self.num_contexts]
        return (x, alpha, values, tau) if return_values else (x, alpha)

    def _ise(self, candidates, about):
        """The body of ``ise_point``: ``(rows, values, targets, alpha, global row)``, the
        last two ``-inf`` / ``-1`` when no row qualifies as ``z``."""
        if about not in ('unsafe', 'all'):
            raise ValueError("about must be 'unsafe' or 'all', got %r" % (about,))
        self._ise_guard()
        be, comm = self._backend, self._comm
        world = comm.world
        fmin = np.asarray(self.fmin, dtype=float).reshape(-1)
        active = np.isfinite(fmin)
        if not active.any():
            raise ValueError("no GP has a finite fmin: there is no safety indicator to learn")
        by_count = np.ndim(candidates) == 0
        if by_count:
            K = int(candidates)
            if K < 1 or K > _hip.MAX_ISE or K != candidates:
                raise ValueError("candidates must be in 1 .. SGP_MAX_ISE = %d, got %r"
                                 % (_hip.MAX_ISE, candidates))
        else:
            rows = np.asarray(candidates)
            if (rows.ndim != 1 or rows.size < 1 or rows.size > _hip.MAX_ISE
                    or not np.issubdtype(rows.dtype, np.integer)):
                raise ValueError("candidates must be a count or a 1-D index array of 1 .. "
                                 "SGP_MAX_ISE = %d rows" % _hip.MAX_ISE)
            rows = rows.astype(np.int64)
            if rows.min() < 0 or rows.max() >= self.inputs.shape[0]:
                raise ValueError("candidate rows outside 0 .. %d" % (self.inputs.shape[0] - 1))
        self._flush_Q()
        self._flush_masks()
        code = _hip.ISE_UNSAFE if about == 'unsafe' else _hip.ISE_ALL
        on_device = all(hasattr(be, f) for f in ('ise_keys', 'ise_hist', 'ise_list'))
        self._ise_path = 'host'
        if world == 1:
            picked = self._ise_select(K, fmin, active) if by_count and on_device else None
            if picked is not None:
                rows = picked[0]
            else:
                var, S, s = be.ise_state()
                if not S.any():
                    raise RuntimeError('There are no safe points to sample in.')
                if by_count:
                    rows = ise_candidates(var, S, s, active, K)
                elif not np.all(S[rows]):
                    raise ValueError("candidate rows outside the safe set: %r"
                                     % (rows[~S[rows]][:8].tolist(),))
            values, targets, alpha, idx = be.ise(fmin, rows, code)[:4]
            return rows, values, targets, alpha, idx
        # ---- N ranks: the same candidates, by value, on every rank
        if by_count:
            picked = self._ise_select(K, fmin, active)
            rows, xc, vx = picked if picked is not None else self._ise_select_host(K, active)
        else:
            xc, vx = self._ise_rows_by_value(rows, fmin)
        if getattr(comm, 'in_stream', False):
            values, targets, alpha, idx = be.ise_at(fmin, rows, xc, vx, code, comm=True)
        else:
            al, tg = be.ise_at(fmin, rows, xc, vx, code)[:2]
            rec = comm.allgather(np.stack([al, tg.astype(np.float64)]))   # (rows < 2^53)
            values, targets = merge_ise_records(rec[:, 0], rec[:, 1].astype(np.int64))
            alpha, idx = pick_ise(values, targets, rows)
        return rows, values, targets, alpha, idx

    def _ise_guard(self):
        """What ``ise_point`` / ``info_point`` need of communicator and backend, before
        anything runs."""
        comm, be = self._comm, self._backend
        if comm.world > 1 and not all(callable(getattr(comm, f, None))
                                      for f in ('allreduce_max', 'allgather')):
            raise NotImplementedError(
                "ise_point runs on one rank with this communicator: on its %d ranks the "
                "candidates and the ranks' picks are agreed on through allreduce_max and "
                "allgather, and it implements neither" % comm.world)
        if not (hasattr(be, 'ise') and hasattr(be, 'ise_state')):
            raise NotImplementedError(
                "this grid backend runs no information-theoretic safe exploration")
        if comm.world > 1 and not all(hasattr(be, f) for f in ('ise_at', 'ise_keys', 'ise_hist',
                                                               'ise_list', 'ise_safe')):
            raise NotImplementedError(
                "this grid backend runs information-theoretic safe exploration on one rank "
                "only (this communicator has %d)" % comm.world)

    def _ise_safe_count(self, fmin):
        """``(|S|, smallest key, largest key)`` over all ranks, the same on every rank."""
        comm = self._comm
        n, lo, hi = self._backend.ise_keys(fmin)
        if comm.world > 1:
            red = comm.allreduce_max(np.array([-lo, hi]))
            lo, hi = -float(red[0]), float(red[1])
            n = int(comm.allgather(np.array([float(n)])).sum())
        return n, lo, hi

    def _ise_select(self, K, fmin, active):
        """The candidates of ``ise_point(candidates=K)``, chosen where the variances are:
        ``(rows (min(K, |S|),), x (.., d), var (G, ..))`` -- what ``ise_candidates`` returns on
        the downloaded state, on every rank -- or ``None`` when the host selection has to take
        over (``self._ise_path`` says why).  The device only ever picks a SUPERSET
        (``ise_threshold``): the ranks agree on count and range of the keys
        (``sgp_grid_ise_keys``), sum their histograms (``sgp_grid_ise_hist``), take ONE
        threshold, list the rows above it (``sgp_grid_ise_list``) and gather the lists; the
        host orders the few listed rows exactly, from the NumPy keys of their variances
        (``ise_order``).  ``RuntimeError`` on every rank when no row is safe."""
        be, comm = self._backend, self._comm
        world = comm.world
        n, lo, hi = self._ise_safe_count(fmin)
        if n == 0:
            raise RuntimeError('There are no safe points to sample in.')
        eps = ISE_KEY_EPS * max(1.0, hi)
        if not hi - lo >= ISE_BINS * 2.0 * eps:
            self._ise_path = 'host: degenerate key range'
            return None
        hist = be.ise_hist(fmin, lo, hi).astype(np.float64)
        if world > 1:
            hist = comm.allgather(hist).sum(axis=0)
        thr, listed = ise_threshold(hist, min(K, n), lo, hi)
        if listed > ise_list_cap(K):
            self._ise_path = 'host: list above the cap'
            return None
        # (rounding at the edge can move a few rows across it: room for them, as in
        # _pass_n_ranks; a count above the room is seen and handed to the host)
        room = listed + 64
        count, gi, _key, x, var = be.ise_list(fmin, thr, room)
        if world > 1:
            counts = comm.allgather(np.array([float(count)]))[:, 0]
            if counts.max() > room:
                self._ise_path = 'host: list above the cap'
                return None
            part = np.empty((gi.size, 1 + x.shape[1] + var.shape[1]))
            part[:, 0], part[:, 1:1 + x.shape[1]] = gi, x               # (rows < 2^53)
            part[:, 1 + x.shape[1]:] = var
            part = allgather_rows(comm, part, counts=counts)
            d = x.shape[1]
            gi, x, var = part[:, 0].astype(np.int64), part[:, 1:1 + d], part[:, 1 + d:]
            count = gi.size
        if count > room or count < min(K, n):
            self._ise_path = 'host: list above the cap' if count > room else 'host: short list'
            return None
        at = ise_order(gi, var, be.ise_noise(), active, K)
        self._ise_path = 'device'
        return gi[at], np.ascontiguousarray(x[at]), np.ascontiguousarray(var[at].T)

    def _ise_select_host(self, K, active):
        """``_ise_select``'s result by the host selection on N ranks: the shards' variances
        and ``S`` gathered, ``ise_candidates`` on every rank."""
        be, comm = self._backend, self._comm
        N = self.inputs.shape[0]
        var, S, s = be.ise_state()
        var = gather_shard_columns(comm, var, N)
        S = gather_shard_columns(comm, S[None, :].astype(np.float64), N)[0] > 0
        rows = ise_candidates(var, S, s, active, K)
        x = self._ise_rows_by_value(rows, None)[0]
        return rows, x, np.ascontiguousarray(var[:, rows])

    def _ise_rows_by_value(self, rows, fmin):
        """Coordinates ``(K, d)`` and variances ``(G, K)`` of the global rows ``rows`` on every
        rank: the owners fetch them (``gather_rows``), one ``allgather``.  With ``fmin`` the
        rows must lie in ``S``: the owners look, and every rank raises the same
        ``RuntimeError`` (no row is safe at all) or ``ValueError``."""
        be, comm = self._backend, self._comm
        world, N = comm.world, self.inputs.shape[0]
        if fmin is not None and self._ise_safe_count(fmin)[0] == 0:
            raise RuntimeError('There are no safe points to sample in.')
        d, G = self.inputs.shape[1], len(self.gps)
        lo, hi = self._shard
        mine = (rows >= lo) & (rows < hi)
        part = np.zeros((rows.size, d + G + 1))
        if mine.any():
            x, _mean, var, _q = be.gather_rows(rows[mine])
            part[mine, :d], part[mine, d:d + G] = x, var
            part[mine, -1] = 1.0 if fmin is None else be.ise_safe(rows[mine])
        allp = comm.allgather(part)
        starts = np.array([shard_range(N, r, world)[0] for r in range(world)])
        owner = np.searchsorted(starts, rows, side='right') - 1
        rec = allp[owner, np.arange(rows.size)]
        bad = rec[:, -1] == 0
        if bad.any():
            raise ValueError("candidate rows outside the safe set: %r"
                             % (rows[bad][:8].tolist(),))
        return np.ascontiguousarray(rec[:, :d]), np.ascontiguousarray(rec[:, d:d + G].T)

    def ise_point(self, candidates=256, about='unsafe', return_values=False):
        """The safe row whose measurement tells most about whether some OTHER row is safe:
        information-theoretic safe exploration (Bottero, Luis, Vinogradska, Berkenkamp,
        Peters 2022) over the resident grid -- the expansion counterpart of ``mes_point``,
        without a Lipschitz constant and without a width rule.

        A GP ``g`` is active when ``fmin_g`` is finite.  For a candidate ``x`` in ``S`` and a
        row ``z``, with ``mu = mean_g(z) - fmin_g``, the resident variances ``vz``, ``vx``
        (clipped at 1e-15), the posterior covariance ``c = c_g(z, x)``, ``s = noise_var_g +
        1e-8`` and ``c1 = 1 / (pi ln 2)``,

            ``t = c1 mu^2 / vz,  r2 = min(c^2 / (vx vz), 1),  e = r2 vx / (s + vx + (2 c1 - 1)
            r2 vx)``,
            ``I_g = -ln2 exp(-t) expm1(log1p(-min(2 c1 e, 1)) / 2 - t (1 - 2 c1) e)``

        approximates the mutual information, in nats, between the measurement at ``x`` and
        the indicator ``[f_g(z) >= fmin_g]``.  The GPs are measured together, so
        ``pair(x, z) = sum_g I_g`` (in the order of ``g``), ``alpha(x) = max_z pair(x, z)``
        and the pick is the candidate with the largest ``alpha``, the lowest row among
        equals.  ``z`` ranges over the rows outside ``S`` (``about='unsafe'``, the rows the
        expander test scans) or over every row (``about='all'``, the paper's domain).  The
        covariances are formed on the device, row tile by row tile, and never stored
        (``sgp_grid_ise``).

        ``candidates``: an int ``K`` -- the ``min(K, |S|)`` rows of ``S`` with the largest
        ``sum_{g active} log1p(var_g / s_g) / 2``, the lower row first among equals: the
        data-processing bound on what a measurement there can tell about anything.  The
        selection runs where the variances are: three passes over the resident ``var`` and
        ``S`` (count and range of the keys, a 4096-bin histogram, the rows above one
        threshold) list a superset of a few hundred rows, and the host orders those exactly
        -- the rows are the ones ``ise_candidates`` takes from the downloaded state, in its
        order; a degenerate key range or a mass of equal keys at the threshold falls back to
        that download.  Or a 1-D integer array of rows, every one of them in ``S`` (else
        ``ValueError``).  At most ``SGP_MAX_ISE`` = 4096 either way.

        Returns ``(x, alpha)``: the row, context columns stripped as ``optimize()`` strips
        them, and its ``alpha``; with ``return_values=True`` ``(x, alpha, rows (K,), values
        (K,), targets (K,))``: the candidates, their ``alpha`` and the rows ``z`` that attain
        them.  Raises ``RuntimeError`` when ``S`` is empty or no row qualifies as ``z``,
        ``ValueError`` when no GP has a finite ``fmin``.  Changes no state of the optimiser
        or its GPs -- except that pending in-place edits of ``opt.Q`` / ``opt.S`` are flushed
        first and the resident posterior is swept again if data came in since the last
        interval update, as for ``mes_point``.  Draws no random numbers.

        N ranks (SPMD: the same call on every rank): the ranks agree on count and range of
        the keys (``allreduce_max``, ``allgather``), sum their histograms, take ONE threshold
        and gather their lists, which carry the rows' coordinates and variances; for an index
        array the owners fetch both and check ``S``.  Every rank then evaluates ALL
        candidates, by value, against its own rows (``sgp_grid_ise_at``), and the ranks'
        ``alpha | target`` blocks are merged -- in the grid's stream with an in-stream
        communicator (``sgp_grid_ise_comm``), else through one ``allgather`` and
        ``dist.merge_ise_records``.  A pair depends on the candidate and the row alone, so
        every rank returns the bits of the one-rank run; every error above is raised on every
        rank, from agreed values.  A communicator of several ranks without ``allreduce_max``
        / ``allgather`` gets ``NotImplementedError`` before anything runs."""
        rows, values, targets, alpha, idx = self._ise(candidates, about)
        if idx < 0:
            raise RuntimeError("no row qualifies as z: every row is in the safe set "
                               "(about='all' takes every row)")
        x = self.inputs[idx, :self.inputs.shape[1] - self.num_contexts]
        return (x, alpha, rows, values, targets) if return_values else (x, alpha)

    def info_point(self, paths=16, features=1024, candidates=256, about='unsafe'):
        """ISE-BO (Bottero et al. 2023): the ``mes_point`` pick (what a measurement tells
        about the VALUE of the safe optimum) or the ``ise_point`` pick (what it tells about
        the SAFETY of another row), whichever acquisition is larger -- both are mutual
        informations in nats.  Returns ``(x, alpha, which)``, ``which`` in ``{'mes',
        'ise'}``; MES wins a tie, and is returned when no row qualifies for ISE.
        ``paths`` / ``features`` as for ``mes_point`` (candidates ``S``, floor ``'mean'``),
        ``candidates`` / ``about`` as for ``ise_point``.  N ranks: the two N-rank picks, the
        same on every rank (seed NumPy's generator alike, as for ``mes_point``)."""
        self._ise_guard()
        xm, am = self.mes_point(paths=paths, features=features)
        _rows, _values, _targets, ai, idx = self._ise(candidates, about)
        if idx >= 0 and ai > am:
            return self.inputs[idx, :self.inputs.shape[1] - self.num_contexts], ai, 'ise'
        return xm, am, 'mes'

    def get_maximum(self, context=None):
        """Best lower bound inside the safe set: ``(x, l)`` or ``None``."""
        self.update_confidence_intervals(context=context)
        self.compute_safe_set()
        if not self._any_safe:
            return None
        v, idx = self._global_argmax(_hip.ARGMAX_LCB)
        return (self.inputs[idx, :-self.num_contexts or None], v)


def _step_into_band(value_at, lo=0.94, hi=0.95, v_max=1000., tol=1e-5):
    """Bisection for a DECREASING ``value_at``: the midpoint ``v`` of the bracket
    ``[a, b]`` (``value_at(a) >= hi > value_at(b)``) at which the value first lies
    strictly inside ``(lo, hi)`` or the bracket is shorter than ``tol``."""
    a, b = 0., v_max
    while True:
        v = 0.5 * (a + b)
        c = value_at(v)
        if c >= hi:
            a = v
        else:
            b = v
        if lo < c < hi or b - a < tol:
            return v


def thompson_pick(best_positions, best_values, safe):
    """The pick of one Thompson swarm: the personal best with the largest value among
    those that are ``safe``, the lowest index among equal values -- ``(x, index)``.
    ``RuntimeError`` when none is safe."""
    best_values = np.asarray(best_values, dtype=float)
    safe = np.asarray(safe, dtype=bool)
    rows = np.flatnonzero(safe)
    if rows.size == 0:
        raise RuntimeError('There are no safe points to sample in.')
    i = int(rows[int(np.argmax(best_values[rows]))])      # (argmax: first among equals)
    return np.array(np.asarray(best_positions)[i], dtype=float), i


def swarm_batch_choice(sd_maxi, sd_exp, scaling, fmin, threshold, ucb=False):
    """Step 3 of ``SafeOptSwarm.optimize_batch``: which swarm's candidate becomes the next
    pick -- ``optimize()``'s rule on the HALLUCINATED standard deviations.  ``sd_maxi`` /
    ``sd_exp``: ``(G,)`` standard deviations of every GP at the maximizers' / expanders'
    candidate, or ``None`` for a swarm that yielded none.  The maximiser's value is
    ``sd_maxi[0] / scaling[0]``, the expander's ``max_g sd_exp[g] / scaling[g]`` over the GPs
    with a finite ``fmin`` and ``sd_exp[g] >= threshold`` (0 when none counts); the maximiser
    wins only when strictly larger, and always with ``ucb``.  Returns ``'maximizers'``,
    ``'expanders'`` or ``None`` (no candidate: the batch ends)."""
    scaling = np.asarray(scaling, dtype=float)
    if ucb or sd_exp is None:
        return None if sd_maxi is None else 'maximizers'
    if sd_maxi is None:
        return 'expanders'
    sd_exp = np.asarray(sd_exp, dtype=float)
    counts = (sd_exp >= threshold) & (np.asarray(fmin, dtype=float) != -np.inf)
    v_exp = np.max(np.where(counts, sd_exp, 0.) / scaling)
    v_maxi = float(np.asarray(sd_maxi, dtype=float)[0]) / scaling[0]
    return 'maximizers' if v_maxi > v_exp else 'expanders'


def swarm_batch_loop(x0, sd0, size, devs, next_pick):
    """Steps 2 and 4 of ``SafeOptSwarm.optimize_batch`` behind the real pick ``x0`` (``sd0``:
    the real standard deviations there): private clones of the device GPs ``devs``, and per
    further pick one append of the pick before to every clone -- with ``y = 0``: only the
    variance is read -- and one ``next_pick(clones) -> (x, sd_h (G,))`` or ``None``.  Ends
    early at a non-positive pivot of an append (logged at ``logging.INFO``) or when there is
    no candidate; the clones are released on every way out.  Returns ``(X (k, d), sd_h (k,
    G))``."""
    X, sds, clones = [np.array(x0, dtype=float)], [np.array(sd0, dtype=float)], []
    try:
        for b in range(1, size):
            if not clones:
                for dv in devs:
                    clones.append(dv.clone())
            if not all([c.append(X[-1], 0.0) for c in clones]):
                logging.getLogger(__name__).info(
                    "optimize_batch: pick %d is determined to rounding by the picks before "
                    "it (non-positive pivot of the bordered append): the batch ends with %d "
                    "points", b - 1, len(X))
                break
            got = next_pick(clones)
            if got is None:
                break
            X.append(np.array(got[0], dtype=float))
            sds.append(np.array(got[1], dtype=float))
    finally:
        for c in clones:
            c.destroy()
    return np.vstack(X), np.vstack(sds)


class NoIseTarget(RuntimeError):
    """``ise_targets`` has no target left: every one is certified safe.  The one outcome of
    ``SafeOptSwarm.ise_point`` that ``info_point`` answers with the MES pick."""


def _ise_about(about):
    if about not in ('unsafe', 'all'):
        raise ValueError("about must be 'unsafe' or 'all', got %r" % (about,))


def ise_target_rows(targets, d):
    """The ``targets`` argument of ``SafeOptSwarm.ise_point``, checked before anything is drawn:
    an int ``T`` in ``1 .. SGP_MAX_ISE`` (returned as it is) or an array of ``T`` finite rows
    ``(T, d)`` (returned as a float copy); ``ValueError`` otherwise."""
    if isinstance(targets, (int, np.integer)) and not isinstance(targets, bool):
        if targets < 1 or targets > _hip.MAX_ISE:
            raise ValueError("targets must be in 1 .. SGP_MAX_ISE = %d, got %d"
                             % (_hip.MAX_ISE, targets))
        return int(targets)
    rows = np.array(targets, dtype=float)
    if rows.ndim != 2 or rows.shape[1] != d or not 1 <= rows.shape[0] <= _hip.MAX_ISE:
        raise ValueError("targets must be an int or (T, d) rows with d = %d and T in 1 .. "
                         "SGP_MAX_ISE = %d, got shape %r" % (d, _hip.MAX_ISE, rows.shape))
    if not np.all(np.isfinite(rows)):
        raise ValueError("a target is not finite")
    return rows


def ise_targets(targets, bounds, about, fmin, beta, posterior):
    """The targets of ``SafeOptSwarm.ise_point`` and their posterior: ``(rows (T', d), zmean
    (G, T'), zvar (G, T'))``.  ``targets``: an int ``T`` -- ONE ``np.random.rand(T, d)`` scaled
    into ``bounds`` (``d`` pairs ``(low, high)``) -- or ``(T, d)`` rows, nothing drawn.
    ``posterior(rows) -> (zmean, zvar)``, the noiseless posterior of every GP, is called once.
    ``about='unsafe'`` drops the rows that are certified safe -- ``mean_g - beta sd_g >=
    fmin_g`` for every GP with a finite ``fmin_g`` --, ``'all'`` keeps every row.  No row
    left: ``NoIseTarget``, a ``RuntimeError``.  A pure function of its arguments and NumPy's
    generator."""
    _ise_about(about)
    bounds = np.asarray(bounds, dtype=float)
    if isinstance(targets, (int, np.integer)):
        low, high = bounds[:, 0], bounds[:, 1]
        rows = low + np.random.rand(int(targets), bounds.shape[0]) * (high - low)
    else:
        rows = np.array(targets, dtype=float)
    zmean, zvar = posterior(rows)
    zmean, zvar = np.asarray(zmean, dtype=float), np.asarray(zvar, dtype=float)
    if about == 'unsafe':
        fmin = np.asarray(fmin, dtype=float)
        active = np.isfinite(fmin)
        lower = zmean[active] - beta * np.sqrt(zvar[active])
        keep = ~np.all(lower >= fmin[active, None], axis=0)
        rows, zmean, zvar = rows[keep], zmean[:, keep], zvar[:, keep]
    if rows.shape[0] == 0:
        raise NoIseTarget("no target is left: every one is certified safe (about='all' "
                          "keeps every target)")
    return (np.ascontiguousarray(rows), np.ascontiguousarray(zmean),
            np.ascontiguousarray(zvar))


class SafeOptFleet(object):
    """Many small ``SafeOpt`` problems stepped together: the members whose ``optimize()``
    would take the one-launch step of a small grid (``sgp_grid_step_small``) take it side by
    side, one workgroup each, in one call (``sgp_grid_step_small_many``) instead of one
    launch and one wait after another.

    >>> fleet = SafeOptFleet(opts)                       # doctest: +SKIP
    >>> X = fleet.optimize()                             # doctest: +SKIP
    >>> for o, x in zip(opts, X):                        # doctest: +SKIP
    ...     o.add_new_data_point(x, measure(x))

    ``fleet.optimize(contexts)`` returns what ``[o.optimize(context=c) for o, c in zip(opts,
    contexts)]`` returns and leaves every member in the state its own ``optimize()`` leaves
    it, bit for bit: the members stay ordinary ``SafeOpt`` objects.  A member that does not
    qualify for the one-launch step (``small_step = False``, Lipschitz certificates, more
    than 48 observations, a grid over the step's budget, a backend without the step) runs its
    own ``optimize()`` behind the launch; one whose first candidate the launch did not
    certify continues alone, as it does behind its own launch.

    The members are independent problems on one device context: an empty list, a member
    that is no ``SafeOpt``, a member on several ranks, one member twice, a GP under two
    members and members on different contexts are refused.  ``ucb`` steps never take the
    one-launch step and are not offered.
    """

    def __init__(self, opts):
        opts = list(opts)
        if not opts:
            raise ValueError("a fleet needs at least one SafeOpt member")
        seen_gp = {}
        for b, o in enumerate(opts):
            if not isinstance(o, SafeOpt):
                raise TypeError("member %d is a %s, not a SafeOpt" % (b, type(o).__name__))
            if o._comm.world > 1:
                raise ValueError("member %d runs on %d ranks: a fleet steps one-rank "
                                 "optimisers" % (b, o._comm.world))
            if any(o is e for e in opts[:b]):
                raise ValueError("member %d is member %d again"
                                 % (b, next(i for i, e in enumerate(opts) if e is o)))
            for g in o.gps:
                if seen_gp.setdefault(id(g), b) != b:
                    raise ValueError("members %d and %d share a GP" % (seen_gp[id(g)], b))
            if getattr(o._backend, 'ctx', None) is not getattr(opts[0]._backend, 'ctx', None):
                raise ValueError("member %d lives in another device context than member 0" % b)
        self.opts = opts
        self._ctx = getattr(opts[0]._backend, 'ctx', None)
        self._plan = self._plan_key = None

    def __len__(self):
        return len(self.opts)

    def optimize(self, contexts=None, return_exceptions=False):
        """One step of every member; the list of their query points.  ``contexts``: one
        context per member (None: none).  A member may raise -- ``EnvironmentError`` when
        none of its rows is safe, say: with ``return_exceptions`` the exception stands in
        its place in the list, otherwise the first one in member order is raised -- in both
        cases after ALL members have been stepped."""
        opts = self.opts
        B = len(opts)
        if contexts is None:
            contexts = [None] * B
        elif len(contexts) != B:
            raise ValueError("%d contexts for %d members" % (len(contexts), B))
        out = [None] * B
        ride, alone = [], []
        for b, o in enumerate(opts):
            try:
                devs = o._small_step_devs() if self._ctx is not None else None
                if devs is None:
                    alone.append(b)
                else:
                    ride.append((b, o, devs, o._small_step_begin(contexts[b])))
            except Exception as e:       # (the member's own step would have raised it)
                out[b] = e
        if ride:
            key = tuple(r[0] for r in ride)
            if self._plan_key != key:
                self._plan = _hip.FleetPlan(self._ctx, [r[1]._backend.grid for r in ride])
                self._plan_key = key
            plan = self._plan
            pbeta = plan.beta
            for j, (b, o, devs, beta) in enumerate(ride):
                o._backend._seen = [None] * len(devs)     # unknown until the call is through
                plan.set_gps(j, devs)
                pbeta[j] = beta
                fm, sc, tb = plan.rows[j]
                fm[:], sc[:], tb[:] = o.fmin, o.scaling, o._thr_beta
            self._ctx.step_small_many(plan)
            value, gidx, max_l = plan.value.tolist(), plan.gidx.tolist(), plan.max_l.tolist()
            for j, (b, o, devs, beta) in enumerate(ride):
                be = o._backend
                be._seen = be._tags(devs)                # (a full sweep: the posterior is current)
                be._rank1_streak = 0
                try:
                    o._small_step_end(beta, plan.result(j, value[j], gidx[j], max_l[j]))
                    out[b] = o.get_new_query_point()
                except Exception as e:
                    out[b] = e
        for b in alone:
            try:
                out[b] = opts[b].optimize(context=contexts[b])
            except Exception as e:
                out[b] = e
        if not return_exceptions:
            for x in out:
                if isinstance(x, Exception):
                    raise x
        return out


class SafeOptSwarm(GaussianProcessOptimization):
    """SafeOpt for higher dimensions with adaptive swarm discretisation.

    Same constructor and behaviour as ``gp_opt.py:715-1192`` of the reference
    (no Lipschitz constant, no contexts).  The particle fitness -- the GP
    posterior of every GP at all particles plus the penalty / interest shaping
    -- is one fused HIP kernel per swarm iteration; the swarm bookkeeping and
    its NumPy global RNG stay on the host so runs are reproducible against the
    reference.

    ``comm`` (as for :class:`SafeOpt`; SPMD: same data, seeds and calls on every
    rank): every swarm run is split over the ranks by particle
    (``sgp_swarm_run_shard``), the global best merged on the device after every
    iteration; growth of the safe set, its recheck and the point predictions stay
    replicated, so every rank holds the same ``S`` and returns the same point as
    one rank would.  ``pso='host'`` runs on one rank only.
    """

    def __init__(self, gp, fmin, bounds, beta=2, scaling='auto', threshold=0,
                 swarm_size=20, pso='device', comm=None, pool_repeats=False):
        if pso not in ('device', 'device-rng', 'host'):
            raise ValueError("pso must be 'device', 'device-rng' or 'host'")
        self._comm = comm if comm is not None else LocalComm()
        world = self._comm.world
        if world > 1:
            # checked on every rank before any collective
            if pso == 'host':
                raise ValueError("pso='host' runs on one rank; %d ranks need pso='device' "
                                 "or 'device-rng'" % world)
            if swarm_size < world:
                raise ValueError("swarm_size %d for %d ranks" % (swarm_size, world))
            ctx = getattr(self._comm, 'ctx', None)
            if ctx is None:
                raise ValueError("the communicator has no device context: the swarm's "
                                 "global best is merged in its stream")
            for g in (gp if isinstance(gp, list) else [gp]):
                g_ctx = getattr(g, '_ctx', None)
                if g_ctx is not None and g_ctx is not ctx:
                    raise ValueError("the GPs live on HIP device %d but the communicator"
                                     " context is device %d" % (g_ctx.device, ctx.device))
        GaussianProcessOptimization.__init__(self, gp, fmin=fmin, beta=beta, num_contexts=0,
                                             threshold=threshold, scaling=scaling,
                                             pool_repeats=pool_repeats)
        # the safe set starts as the observed inputs; one (min, max) pair may
        # stand for every dimension
        safe_points = np.asarray(self.gps[0].X)
        self.S, self.greedy_point = safe_points, safe_points[0, :]
        self.swarm_size, self.max_iters = swarm_size, 100
        self.bounds = bounds if isinstance(bounds, list) else [bounds] * safe_points.shape[1]
        self.best_lower_bound = -np.inf
        self.optimal_velocities = self.optimize_particle_velocity()

        # pso='device' (default): whole swarm runs on the GPU with NumPy's
        # random stream (bit-identical to the host loop); 'device-rng': GPU
        # generator, no per-run random upload; 'host': the reference's loop
        # with one fitness call per iteration.
        if pso == 'host':
            self.swarms = {
                swarm_type: SwarmOptimization(
                    swarm_size, self.optimal_velocities,
                    partial(self._compute_particle_fitness, swarm_type),
                    bounds=self.bounds)
                for swarm_type in ['greedy', 'maximizers', 'expanders']}
        else:
            self.swarms = {
                swarm_type: DeviceSwarmOptimization(
                    swarm_size, self.optimal_velocities, self, swarm_type,
                    bounds=self.bounds,
                    rng='numpy' if pso == 'device' else 'device', comm=self._comm)
                for swarm_type in ['greedy', 'maximizers', 'expanders']}

    def optimize_particle_velocity(self):
        """Step length per input dimension at which a particle's prior correlation
        with its starting point has fallen into (0.94, 0.95), the smallest over the
        GPs, divided by sqrt(d) (``gp_opt.py:818-872``).  Stationary kernels only:
        the correlation is probed from the origin."""
        d = self.gp.input_dim
        origin = np.zeros((1, d))

        def correlation(gp, scale, axis):
            probe = np.zeros((1, d))

            def at(v):
                probe[0, axis] = v
                return float(np.squeeze(gp.kern.K(origin, probe))) / scale ** 2
            return at

        per_gp = [[_step_into_band(correlation(gp, self.scaling[i], j)) for j in range(d)]
                  for i, gp in enumerate(self.gps)]
        return np.min(np.asarray(per_gp, dtype=float), axis=0) / np.sqrt(d)

    def _compute_penalty(self, slack):
        """Penalty of a constraint violation (``gp_opt.py:874-899``): zero for a
        satisfied constraint, the (negative) slack times 2 / 5 / 10 on the bands
        (-0.001, 0), (-1, -0.1], ..., and ``-300 slack^2`` below -1 (a slack of
        exactly -1 keeps its own value).  Host helper; the device applies the same
        rule inside the fitness kernels (``csrc/fitness.h``)."""
        s = np.atleast_1d(np.asarray(slack, dtype=float))
        return np.select([s >= 0, s > -0.001, s > -0.1, s > -1, s == -1],
                         [np.zeros_like(s), 2 * s, 5 * s, 10 * s, s], default=-300 * (s * s))

    def _compute_particle_fitness(self, swarm_type, particles):
        """Fitness and safety of ``particles`` for one swarm type:
        ``'greedy' | 'maximizers' | 'expanders' | 'safe_set'``."""
        if swarm_type not in _hip.SWARM_TYPES:
            raise AssertionError("Invalid swarm type")
        return self._swarm_fitness(swarm_type, particles)

    def _swarm_fitness(self, swarm_type, particles, **variant):
        """What the fitness callbacks share: the current ``beta``, the fitted device GPs and
        this optimiser's ``fmin`` / ``scaling`` / best lower bound; ``variant``: ``path=``,
        ``clones=``, ``mes=``, ``ise=`` or ``ei=`` (the last two with ``want=``) of
        ``_hip._swarm_fitness``."""
        beta = self.beta(self.t)
        devs = [g._fitted() for g in self.gps]
        return _hip._swarm_fitness(devs[0].ctx, devs, swarm_type, np.atleast_2d(particles),
                                   (beta, self.fmin, self.scaling, self.best_lower_bound),
                                   **variant)

    def _compute_path_fitness(self, path, particles):
        """Fitness and safety of ``particles`` for a Thompson swarm on the sample path
        ``path = (Omega, phase, w, v)`` of the objective GP: ``values = f(x) / scaling[0] +``
        the maximizers' penalty, ``safe`` the maximizers' safety flag
        (``sgp_swarm_fitness_path``).  The fitness callback of the host loop."""
        return self._swarm_fitness(None, particles, path=path)

    def _compute_hall_fitness(self, swarm_type, clones, particles):
        """Fitness and safety of ``particles`` for a hallucinated ``'maximizers'`` or
        ``'expanders'`` swarm: the width term from the variance of ``clones`` (the device GPs'
        clones with the pending picks appended), everything else -- bounds, interest, penalty,
        ``safe`` -- from the real GPs (``sgp_swarm_fitness_hall``).  The fitness callback of
        the host loop."""
        return self._swarm_fitness(swarm_type, particles, clones=clones)

    def _compute_mes_fitness(self, mes, particles):
        """Fitness and safety of ``particles`` for a max-value entropy search swarm with
        ``mes = (ystar, floor)``: ``values = alpha + `` the maximizers' penalty, ``alpha`` the
        acquisition of ``gp.max_value_entropy`` on the posterior of the objective GP, ``safe``
        the maximizers' safety flag (``sgp_swarm_fitness_mes``).  The fitness callback of the
        host loop."""
        return self._swarm_fitness(None, particles, mes=mes)

    def _compute_ise_fitness(self, ise, particles, want=None):
        """Fitness and safety of ``particles`` for an information-theoretic safe exploration
        swarm with ``ise = (targets, zmean, zvar)``: ``values = alpha + `` the maximizers'
        penalty, ``alpha[p] = max_t pair(p, t)`` over the targets, ``safe`` the maximizers'
        safety flag (``sgp_swarm_fitness_ise``).  The fitness callback of the host loop;
        ``want``: ``(values, safe, out)`` with the arrays named in it (``_hip._swarm_fitness``)."""
        res = self._swarm_fitness(None, particles, ise=ise, want=want or ())
        return res if want else res[:2]

    def _compute_ei_fitness(self, ei, particles, want=None):
        """Fitness and safety of ``particles`` for an expected-improvement swarm with ``ei =
        (kind, tau, xi, feasibility, free)``: ``values = alpha + `` the maximizers' penalty,
        ``alpha`` the logarithm of ``Context.ei_eval`` on the posterior of the GPs, ``safe``
        the maximizers' safety flag -- with ``free`` ``values = alpha`` and every particle
        safe (``sgp_swarm_fitness_ei``).  The fitness callback of the host loop; ``want``:
        ``(values, safe, out)`` with the arrays named in it, 'alpha' (P) and 'post' (G, 2, P)
        (``_hip._swarm_fitness``)."""
        return self._swarm_fitness(None, particles, ei=ei, want=want or ())

    def _side_swarm_pick(self, swarm, configure, fitness, iters, empty_ok=False,
                         unchecked=False):
        """One side swarm of ``optimize_batch`` / ``thompson_points`` and its pick ``(x,
        index)``: ``swarm_size`` draws of ``S`` as start positions (one ``randint``), then the
        device swarm ``swarm`` after ``configure(swarm)`` -- or, ``swarm is None``
        (``pso='host'``), a reference loop over the callback ``fitness`` -- runs ``iters``
        iterations; the pick is ``thompson_pick`` among the personal bests that are safe under
        one real ``'safe_set'`` fitness call.  None is safe: ``RuntimeError``, or ``None``
        with ``empty_ok``.  ``unchecked`` (``ei_point(within='bounds')`` alone): no
        ``'safe_set'`` call, the pick is ``thompson_pick`` among ALL personal bests -- not a
        safe pick."""
        picks = np.random.randint(self.S.shape[0], size=self.swarm_size)
        if swarm is None:
            swarm = SwarmOptimization(self.swarm_size, self.optimal_velocities, fitness,
                                      bounds=self.bounds)
        else:
            configure(swarm)
        swarm.init_swarm(self.S[picks, :])
        swarm.run_swarm(iters)
        if unchecked:
            return thompson_pick(swarm.best_positions, swarm.best_values,
                                 np.ones(len(swarm.best_values), dtype=bool))
        _, safe = self._compute_particle_fitness('safe_set', swarm.best_positions)
        if empty_ok and not np.any(safe):
            return None
        return thompson_pick(swarm.best_positions, swarm.best_values, safe)

    def optimize_batch(self, size=8, ucb=False, max_iters=None, return_state=False):
        """``k <= size`` query points from SafeOptSwarm's own rule for experiments that run
        in parallel, without a grid: the GP-BUCB construction (Desautels et al. 2014) of
        ``SafeOpt.optimize_batch`` on the swarms.  A pending pick is "hallucinated" into
        private copies of the GPs: the means stay, the widths shrink around it.

        1. ``x_0 = self.optimize(ucb=ucb)``, the unchanged step: row 0 is what ``optimize()``
           returns, and the optimiser's state afterwards -- ``S``, ``greedy_point``,
           ``best_lower_bound``, ``t``, the three swarm objects, the GPs -- is the state
           after ``optimize()``.
        2. Every GP's device handle is cloned; for ``b = 1 .. size - 1`` the pick ``x_{b-1}``
           is appended to every clone and a hallucinated maximizers swarm and (unless
           ``ucb``) a hallucinated expanders swarm run: swarm objects of their own, each
           from ``swarm_size`` draws of ``S`` (no fixed points), ``max_iters`` (default
           ``self.max_iters``) iterations.  Their fitness is ``(values + total_pen) *
           interest`` with ``values = max_g sqrt(var_h_g) / scaling_g`` from the hallucinated
           variance ``var_h_g = max(var_g - down_g, 1e-15)`` and everything else -- lower and
           upper bounds, the interest, the penalty, the safety flag -- from the real
           posterior (``csrc/fitness.h``).  A swarm's candidate is the personal best with the
           largest value among those safe under one real ``'safe_set'`` fitness call, the
           lowest index among equals (``thompson_pick``'s rule); a swarm with no safe
           personal best yields none.
        3. Between the two candidates ``optimize()``'s rule decides, on the hallucinated
           standard deviations there (``swarm_batch_choice``); no candidate ends the batch.
        4. The batch also ends early, with ``k < size`` rows, when the bordered append of a
           pick meets a non-positive pivot (logged at ``logging.INFO``, not an error).  The
           clones are released on every way out.

        Safety is untouched: hallucinated widths only rank points inside what the real data
        certified; no bound compared with ``fmin`` is a hallucinated one.  Nothing real
        changes after step 1: ``S`` neither grows nor is rechecked in the hallucinated runs,
        so ``add_new_data_point`` + ``optimize()`` afterwards give what they give after a
        plain ``optimize()`` under the same seed.

        Returns ``X (k, d)``, ``1 <= k <= size``; with ``return_state=True`` ``(X, sd_h (k,
        G))``: the hallucinated standard deviation of every GP at every pick when it was
        picked (row 0: the real ones).  ``size`` outside ``1 .. SGP_MAX_BATCH`` (64) raises
        ``ValueError``.

        N ranks (SPMD, as ``optimize()``: the same data, seed and call on every rank): the
        hallucinated swarms are split over the ranks by particle like every other swarm
        (``sgp_swarm_run_hall_shard``: the global best merged on the device after every
        iteration, the personal bests gathered after a run); every rank clones its own
        device GPs and appends the same picks.  The start draws, the ``'safe_set'`` recheck
        of the gathered personal bests, ``swarm_batch_choice`` and the predictions on the
        clones stay replicated, so every rank returns the bits of the one-rank run and
        NumPy's generator ends where the one-rank run leaves it.  Several ranks whose
        communicator carries no device context (``comm.ctx``): ``optimize_batch`` runs on one
        rank only there and raises ``NotImplementedError`` before anything runs or is drawn.

        NumPy's global generator is consumed in this order:

        1. what ``optimize(ucb=ucb)`` draws;
        2. ``size > 1`` and ``pso='device-rng'`` only: one ``randint`` for the key of the
           maximizers swarm's device generator, then (unless ``ucb``) one for the expanders';
        3. per pick ``b``, for the maximizers swarm and then (unless ``ucb``) the expanders
           swarm: one ``randint(len(S), size=swarm_size)`` for the start positions, then
           what a swarm of that ``pso`` draws -- ``'host'``: ``rand(swarm_size, d)`` in
           ``init_swarm`` and ``rand(2 swarm_size, d)`` per iteration; ``'device'``: the same
           numbers as ``rand(swarm_size d)`` and ``rand(2 swarm_size d max_iters)``, one C
           call each; ``'device-rng'``: nothing.

        Out of scope: growing ``S`` from hallucinated runs; all picks or both swarms in one
        launch."""
        size = int(size)
        if size < 1 or size > _hip.MAX_BATCH:
            raise ValueError("size must be in 1 .. SGP_MAX_BATCH = %d, got %d"
                             % (_hip.MAX_BATCH, size))
        if self._comm.world > 1 and getattr(self._comm, 'ctx', None) is None:
            raise NotImplementedError(
                "optimize_batch runs on one rank unless the communicator carries a device "
                "context (this communicator of %d ranks has no ctx)" % self._comm.world)
        x0 = np.array(self.optimize(ucb=ucb), dtype=float)
        sd0 = np.sqrt([gp.predict_noiseless(x0[None, :])[1].item() for gp in self.gps])
        iters = int(max_iters or self.max_iters)
        types = ['maximizers'] if ucb else ['maximizers', 'expanders']
        swarms = {}                       # pso='host': a reference loop per run
        if size > 1 and isinstance(self.swarms['maximizers'], DeviceSwarmOptimization):
            swarms = {t: DeviceSwarmOptimization(
                self.swarm_size, self.optimal_velocities, self, t, bounds=self.bounds,
                rng=self.swarms['maximizers']._rng, comm=self._comm) for t in types}

        def candidate(swarm_type, clones):
            pick = self._side_swarm_pick(
                swarms.get(swarm_type), lambda run: run.set_clones(clones),
                partial(self._compute_hall_fitness, swarm_type, clones), iters, empty_ok=True)
            if pick is None:
                return None
            x = pick[0]
            return x, np.sqrt([c.predict(x[None, :])[1].item() for c in clones])

        def next_pick(clones):
            found = {t: candidate(t, clones) for t in types}
            which = swarm_batch_choice(
                None if found['maximizers'] is None else found['maximizers'][1],
                None if found.get('expanders') is None else found['expanders'][1],
                self.scaling, self.fmin, self.threshold, ucb=ucb)
            return None if which is None else found[which]

        X, sd_h = swarm_batch_loop(x0, sd0, size, [g._fitted() for g in self.gps], next_pick)
        return (X, sd_h) if return_state else X

    def thompson_points(self, size=8, features=1024, max_iters=None, return_paths=False):
        """``size`` Thompson picks without a grid: per posterior sample path of the
        objective GP (``gps[0]``, ``GPRegression.posterior_paths(size, features)``) one swarm
        climbs the path, held inside the safe region by the penalty and safety rule of the
        maximizers swarm -- a batch of safe query points for experiments that run in
        parallel, from three or four input dimensions up.

        The fitness of a particle is ``f_s(x) / scaling[0] + total_pen`` (``csrc/fitness.h``),
        evaluated on the device inside the swarm iteration; every swarm starts from
        ``swarm_size`` draws from the safe set ``S`` (no fixed points) and runs ``max_iters``
        (default ``self.max_iters``) iterations.  The pick of a path is the personal best
        with the largest value among those that are safe under the current posterior (one
        ``safe_set`` fitness call; ``init_swarm`` does not mask, and ``_recheck_safe_set`` may
        keep unsafe points), the lowest index among equals.

        Returns ``(x (size, d), values (size,))`` with ``values[s] = pp.paths(x[s][None])[0, 0,
        s]``; with ``return_paths=True`` also the ``PosteriorPaths`` ``pp``.  Raises
        ``RuntimeError`` when the safe set is empty or a swarm ends with no safe personal
        best, ``ValueError`` for more than ``SGP_MAX_PATHS`` paths.

        N ranks (``comm=``; SPMD, the same seed and call on every rank): every swarm is
        split over the ranks by particle as the other swarms are
        (``sgp_swarm_run_path_shard``: the path staged on every rank, the global best merged
        on the device after every iteration); every rank draws what one rank draws -- one
        ``allreduce_max`` of a digest verifies that the ranks hold the same paths,
        ``ValueError`` on every rank otherwise -- and the final ``safe_set`` fitness call and
        the pick run replicated on the gathered personal bests: the bits of the one-rank run
        on every rank.  The global best is merged in the stream of the communicator's device
        context; a communicator of several ranks without one is refused
        (``NotImplementedError``) before any draw.

        Changes no state of the optimiser beyond what ``_recheck_safe_set`` does at the start
        of every swarm run (it may drop points that are no longer safe): ``S`` does not grow,
        ``greedy_point``, ``best_lower_bound`` and the greedy / maximizers / expanders swarm
        objects are untouched.  NumPy's global generator is consumed in this order:

        1. ``pso='device-rng'`` only: one ``randint`` for the key of the device generator;
        2. the ``posterior_paths`` draw (``safeopt_amd/paths.py`` documents its order);
        3. per path: one ``randint(len(S), size=swarm_size)`` for the start positions, then
           what a swarm of that ``pso`` draws today -- ``'host'``: ``rand(swarm_size, d)`` in
           ``init_swarm`` and ``rand(2 swarm_size, d)`` per iteration; ``'device'``: the same
           numbers as ``rand(swarm_size d)`` and ``rand(2 swarm_size d max_iters)``, one C
           call each; ``'device-rng'``: nothing.

        Out of scope: running all ``size`` swarms as one launch with per-swarm global bests;
        paths of the constraint GPs (the constraints enter through their confidence
        bounds)."""
        size = int(size)
        if size > _hip.MAX_PATHS:
            raise ValueError("size = %d paths, at most SGP_MAX_PATHS = %d per call"
                             % (size, _hip.MAX_PATHS))
        world = self._comm.world
        if world > 1 and getattr(self._comm, 'ctx', None) is None:
            # (what the constructor asks of a communicator of several ranks)
            raise NotImplementedError(
                "the sharded Thompson swarm merges the global best in the stream of the "
                "communicator's device context: a merge over this host-only communicator of "
                "%d ranks is not implemented" % world)
        self._recheck_safe_set()
        iters = int(max_iters or self.max_iters)
        swarm = None                      # pso='host': a reference loop per path
        if isinstance(self.swarms['maximizers'], DeviceSwarmOptimization):
            swarm = DeviceSwarmOptimization(
                self.swarm_size, self.optimal_velocities, self, 'thompson',
                bounds=self.bounds, rng=self.swarms['maximizers']._rng, comm=self._comm)
        pp = self.gp.posterior_paths(size, features)
        if world > 1:
            check_same_paths(self._comm, pp)
        x = np.empty((size, self.gp.input_dim))
        for s in range(size):
            path = (pp.Omega, pp.phase, np.ascontiguousarray(pp.W[:, s]),
                    np.ascontiguousarray(pp.V[:, s]))
            x[s], _ = self._side_swarm_pick(
                swarm, lambda run: run.set_path(path),
                partial(self._compute_path_fitness, path), iters)
        values = np.array([pp.paths(x[s][None])[0, 0, s] for s in range(size)])
        return (x, values, pp) if return_paths else (x, values)

    def mes_point(self, paths=16, features=1024, floor='mean', ystar=None, max_iters=None,
                  return_state=False):
        """The safe point whose measurement tells most about the VALUE of the safe optimum,
        without a grid: max-value entropy search (Wang & Jegelka 2017; ``SafeOpt.mes_point``
        on a grid) by a swarm.  It needs no Lipschitz constant and no width rule.

        1. The refusals below come before anything is drawn or run.
        2. ``ystar=None``: ``x_t, values = self.thompson_points(size=paths, features=features,
           max_iters=max_iters)`` and ``ystar = values`` -- a path's value at its own safe
           pick is a lower bound of its maximum over the safe region.  ``ystar`` given (``1 ..
           SGP_MAX_MES`` finite maxima): no path is drawn; ``_recheck_safe_set()`` runs once.
        3. ``floor='mean'`` (default): the largest posterior mean of the objective GP over
           the rows of ``S`` and the Thompson picks (one ``predict_noiseless`` call) -- a
           maximum cannot lie below a value the mean already reaches, and without the floor
           such a ``ystar`` would make ``gamma`` negative and the pick collapse onto the point
           with the smallest ``sigma``.  ``None``: no floor; a float: that value.
        4. One swarm (``DeviceSwarmOptimization(..., 'mes')``; ``pso='host'``: the reference
           loop over ``_compute_mes_fitness``) starts from ``swarm_size`` draws from ``S`` and
           runs ``max_iters`` (default ``self.max_iters``) iterations.  The fitness of a
           particle is ``alpha(x) + total_pen``: with ``mu``, ``v`` the posterior of the
           objective, ``sigma = sqrt(max(v, 1e-15))``, ``y_k = max(ystar_k, floor)`` and
           ``gamma_k = (y_k - mu) / sigma``, ``alpha = mean_k [gamma_k phi(gamma_k) / (2
           Phi(gamma_k)) - ln Phi(gamma_k)]``, formed on the device inside the swarm
           iteration (``k_swarm_mes``, ``csrc/mes.hip``), under the penalty and safety rule
           of the maximizers swarm.  The pick is the personal best with the largest value
           among those that are safe under the current posterior (one ``safe_set`` fitness
           call), the lowest index among equals.
        5. Returns ``(x (d,), alpha)`` with ``alpha = gp.max_value_entropy(x[None], ystar,
           floor)[0, 0]``; with ``return_state=True`` ``(x, alpha, {'ystar', 'floor',
           'thompson_x'})`` (``thompson_x``: the Thompson picks, ``None`` with ``ystar`` given).

        Raises ``ValueError`` for ``paths`` (or ``len(ystar)``) outside ``1 .. SGP_MAX_MES``
        (64), a maximum that is not finite, a floor that is NaN or a string other than
        ``'mean'``; ``NotImplementedError`` for several ranks whose communicator carries no
        device context (``thompson_points``' refusal); ``RuntimeError`` when the safe set is
        empty or the swarm ends with no safe personal best.

        Changes no state of the optimiser beyond what ``_recheck_safe_set`` does (it may drop
        points that are no longer safe): ``S`` does not grow, ``greedy_point``,
        ``best_lower_bound`` and the greedy / maximizers / expanders swarm objects are
        untouched.  NumPy's global generator is consumed in this order:

        1. with ``ystar=None``, what ``thompson_points(size=paths, ...)`` draws, in its order;
        2. ``pso='device-rng'`` only: one ``randint`` for the key of the swarm's device
           generator;
        3. one swarm's worth, as step 3 of ``thompson_points``, once: one
           ``randint(len(S), size=swarm_size)`` for the start positions, then ``'host'``:
           ``rand(swarm_size, d)`` in ``init_swarm`` and ``rand(2 swarm_size, d)`` per
           iteration; ``'device'``: the same numbers as ``rand(swarm_size d)`` and ``rand(2
           swarm_size d max_iters)``; ``'device-rng'``: nothing.

        N ranks (``comm=``; SPMD, the same seed and call on every rank): the Thompson swarms
        are sharded as ``thompson_points`` shards them and the 'mes' swarm is split over the
        ranks by particle like every other swarm (``sgp_swarm_run_mes_shard``).  ``ystar``
        and ``floor`` are functions of replicated data: one ``allreduce_max`` of a digest
        verifies that the ranks hold the same, ``ValueError`` on every rank otherwise.  The
        ``safe_set`` call and the pick run replicated on the gathered personal bests: the
        bits of the one-rank run on every rank.

        Out of scope: greedy batches of MES picks through the hallucination clones,
        noisy-observation MES, running the Thompson swarms as one launch."""
        if ystar is None:
            paths = int(paths)
            if paths < 1 or paths > _hip.MAX_MES:
                raise ValueError("paths must be in 1 .. SGP_MAX_MES = %d, got %d"
                                 % (_hip.MAX_MES, paths))
        else:
            ystar = np.array(ystar, dtype=float).reshape(-1)
            if ystar.size < 1 or ystar.size > _hip.MAX_MES:
                raise ValueError("ystar must hold 1 .. SGP_MAX_MES = %d maxima, got %d"
                                 % (_hip.MAX_MES, ystar.size))
            if not np.all(np.isfinite(ystar)):
                raise ValueError("a maximum in ystar is not finite")
        if isinstance(floor, str):
            if floor != 'mean':
                raise ValueError("floor must be 'mean', None or a float, got %r" % (floor,))
        elif floor is not None:
            floor = float(floor)
            if np.isnan(floor):
                raise ValueError("floor is NaN")
        world = self._comm.world
        if world > 1 and getattr(self._comm, 'ctx', None) is None:
            raise NotImplementedError(
                "the sharded 'mes' swarm merges the global best in the stream of the "
                "communicator's device context: a merge over this host-only communicator of "
                "%d ranks is not implemented" % world)
        thompson_x = None
        if ystar is None:
            thompson_x, ystar = self.thompson_points(size=paths, features=features,
                                                     max_iters=max_iters)
        else:
            self._recheck_safe_set()
        if floor is None:
            floor = -np.inf
        elif floor == 'mean':
            rows = self.S if thompson_x is None else np.vstack((self.S, thompson_x))
            floor = float(np.max(self.gp.predict_noiseless(rows)[0]))
        if world > 1:
            check_same_maxima(self._comm, ystar, floor)
        iters = int(max_iters or self.max_iters)
        swarm = None                      # pso='host': a reference loop
        if isinstance(self.swarms['maximizers'], DeviceSwarmOptimization):
            swarm = DeviceSwarmOptimization(
                self.swarm_size, self.optimal_velocities, self, 'mes',
                bounds=self.bounds, rng=self.swarms['maximizers']._rng, comm=self._comm)
        x, _ = self._side_swarm_pick(
            swarm, lambda run: run.set_maxima(ystar, floor),
            partial(self._compute_mes_fitness, (ystar, floor)), iters)
        alpha = float(self.gp.max_value_entropy(x[None, :], ystar, floor)[0, 0])
        if return_state:
            return x, alpha, dict(ystar=ystar, floor=floor, thompson_x=thompson_x)
        return x, alpha

    def ei_point(self, incumbent='mean', xi=0.0, kind='ei', feasibility=False, within='safe',
                 max_iters=None, return_state=False):
        """The safe point with the largest expected improvement over the incumbent, evaluated
        as a logarithm (LogEI: Ament et al. 2023), without a grid: ``SafeOpt.ei_point`` by a
        swarm.  It needs no Lipschitz constant and no width rule.

        1. The refusals below come before anything is drawn or run.
        2. ``_recheck_safe_set()`` runs once.
        3. The incumbent ``tau``.  ``incumbent='mean'`` (default): the largest posterior mean
           of the objective GP over the rows of ``S`` (one ``predict_noiseless`` call; the
           same for ``within='bounds'``, there is no other set); ``'data'``: the largest
           measured objective value, ``max(opt.y[:, 0])`` over the entries that are not NaN; a
           finite float: that value.  ``xi >= 0``: the margin an improvement has to exceed.
        4. One swarm (``DeviceSwarmOptimization(..., 'ei')``; ``pso='host'``: the reference
           loop over ``_compute_ei_fitness``) starts from ``swarm_size`` draws from ``S`` and
           runs ``max_iters`` (default ``self.max_iters``) iterations.  With ``mu_g``, ``v_g``
           the posterior of GP ``g`` (the objective is GP 0), ``sigma_g = sqrt(max(v_g,
           1e-15))`` and ``z = (mu_0 - tau - xi) / sigma_0``,

               ``kind='ei'``: ``alpha(x) = ln sigma_0 + ln(phi(z) + z Phi(z))``  (= ln EI),
               ``kind='pi'``: ``alpha(x) = ln Phi(z)``  (= ln PI),

           and with ``feasibility=True`` every GP with a finite ``fmin`` adds ``ln Phi((mu_g -
           fmin_g) / sigma_g)`` (EIC: Gelbart et al. 2014, Gardner et al. 2014).  It is formed
           on the device inside the swarm iteration (``k_swarm_ei``, ``csrc/ei.hip``).  On a
           converged run EI itself underflows to 0 almost everywhere and a swarm on it has
           nothing to climb; ``alpha`` stays finite and ordered.
           ``within='safe'``: the fitness of a particle is ``alpha(x) + total_pen`` under the
           penalty and safety rule of the maximizers swarm, and the pick is the personal best
           with the largest value among those that are safe under the current posterior (one
           ``safe_set`` fitness call), the lowest index among equals.
           ``within='bounds'``: the fitness is ``alpha(x)`` alone, every particle counts as
           safe, and the pick is the personal best with the largest value, the lowest index
           among equals; no ``safe_set`` call.  This is NOT a safe pick: with
           ``feasibility=True`` it is the EIC baseline the safe-BO papers compare against, for
           diagnostics and unconstrained problems only.
        5. Returns ``(x (d,), alpha)`` with ``alpha = ctx.ei_eval`` on ``predict_noiseless`` of
           every GP at ``x`` -- the number the public per-point call gives; with
           ``return_state=True`` ``(x, alpha, {'tau', 'kind', 'xi', 'safe'})``, ``safe`` the
           ``safe_set`` flag of the pick (computed in that case for ``within='bounds'`` too).

        Raises ``ValueError`` for a ``within`` other than ``'safe'`` / ``'bounds'``, a ``kind``
        other than ``'ei'`` / ``'pi'``, an ``xi`` that is negative or not finite, an
        ``incumbent`` that is neither ``'mean'``, ``'data'`` nor a finite float, or
        ``'data'`` without a measurement of the objective; ``NotImplementedError`` for several
        ranks whose communicator carries no device context; ``RuntimeError`` when the safe
        set is empty or, ``within='safe'``, the swarm ends with no safe personal best.

        Changes no state of the optimiser beyond what ``_recheck_safe_set`` does (it may drop
        points that are no longer safe): ``S`` does not grow, ``greedy_point``,
        ``best_lower_bound`` and the greedy / maximizers / expanders swarm objects are
        untouched.  NumPy's global generator is consumed in the order of steps 2 - 3 of
        ``mes_point``'s list; no path is drawn:

        1. ``pso='device-rng'`` only: one ``randint`` for the key of the swarm's device
           generator;
        2. one swarm's worth: one ``randint(len(S), size=swarm_size)`` for the start
           positions, then ``'host'``: ``rand(swarm_size, d)`` in ``init_swarm`` and ``rand(2
           swarm_size, d)`` per iteration; ``'device'``: the same numbers as ``rand(swarm_size
           d)`` and ``rand(2 swarm_size d max_iters)``; ``'device-rng'``: nothing.

        N ranks (``comm=``; SPMD, the same seed and call on every rank): the incumbent is a
        function of replicated data; one ``allreduce_max`` of a digest of ``(kind, tau, xi,
        feasibility, free)`` verifies that the ranks hold the same, ``ValueError`` on every
        rank otherwise.  The swarm is split over the ranks by particle
        (``sgp_swarm_run_ei_shard``); the ``safe_set`` call and the pick run replicated on the
        gathered personal bests: the bits of the one-rank run on every rank.

        Out of scope: greedy batches of EI picks through the hallucination clones,
        noisy-incumbent EI, an ``'ei'`` leg in ``info_point``."""
        if within not in ('safe', 'bounds'):
            raise ValueError("within must be 'safe' or 'bounds', got %r" % (within,))
        if kind not in ('ei', 'pi'):
            raise ValueError("kind must be 'ei' or 'pi', got %r" % (kind,))
        xi = float(xi)
        if not (np.isfinite(xi) and xi >= 0.0):
            raise ValueError("xi must be finite and >= 0, got %r" % (xi,))
        if isinstance(incumbent, str):
            if incumbent not in ('mean', 'data'):
                raise ValueError("incumbent must be 'mean', 'data' or a float, got %r"
                                 % (incumbent,))
            tau = 'mean'
            if incumbent == 'data':
                seen = self.y[:, 0][~np.isnan(self.y[:, 0])]
                if seen.size == 0:
                    raise ValueError("incumbent='data': the objective has no measurement")
                tau = float(seen.max())
        else:
            tau = float(incumbent)
        if tau != 'mean' and not np.isfinite(tau):
            raise ValueError("the incumbent must be finite, got %r" % (tau,))
        world = self._comm.world
        if world > 1 and getattr(self._comm, 'ctx', None) is None:
            raise NotImplementedError(
                "the sharded 'ei' swarm merges the global best in the stream of the "
                "communicator's device context: a merge over this host-only communicator of "
                "%d ranks is not implemented" % world)
        self._recheck_safe_set()
        if tau == 'mean':
            tau = float(np.max(self.gp.predict_noiseless(self.S)[0]))
        free = within == 'bounds'
        ei = (kind, tau, xi, bool(feasibility), free)
        if world > 1:
            check_same_incumbent(self._comm, *ei)
        iters = int(max_iters or self.max_iters)
        swarm = None                      # pso='host': a reference loop
        if isinstance(self.swarms['maximizers'], DeviceSwarmOptimization):
            swarm = DeviceSwarmOptimization(
                self.swarm_size, self.optimal_velocities, self, 'ei',
                bounds=self.bounds, rng=self.swarms['maximizers']._rng, comm=self._comm)
        x, _ = self._side_swarm_pick(
            swarm, lambda run: run.set_incumbent(*ei),
            partial(self._compute_ei_fitness, ei), iters, unchecked=free)
        post = [gp.predict_noiseless(x[None, :]) for gp in self.gps]
        mean = np.stack([np.asarray(m, dtype=float).reshape(-1) for m, _ in post])
        var = np.stack([np.asarray(v, dtype=float).reshape(-1) for _, v in post])
        ctx = self.gp._fitted().ctx
        alpha = float(ctx.ei_eval(
            mean, var, tau, xi, _hip.EI_EI if kind == 'ei' else _hip.EI_PI,
            np.asarray(self.fmin, dtype=float).reshape(-1) if feasibility else None)[0])
        if return_state:
            _, safe = self._compute_particle_fitness('safe_set', x[None, :])
            return x, alpha, dict(tau=tau, kind=kind, xi=xi, safe=bool(safe[0]))
        return x, alpha

    def _ise_refusals(self, targets, about):
        """The argument refusals ``ise_point`` and ``info_point`` share, before anything is
        drawn or run; returns ``ise_target_rows``' form of ``targets``."""
        targets = ise_target_rows(targets, self.gp.input_dim)
        _ise_about(about)
        if not np.any(np.isfinite(self.fmin)):
            raise ValueError("no GP is active: every fmin is infinite")
        return targets

    def ise_point(self, targets=256, about='unsafe', max_iters=None, return_state=False):
        """The safe point whose measurement tells most about whether some OTHER point is safe,
        without a grid: information-theoretic safe exploration (Bottero, Luis, Vinogradska,
        Berkenkamp, Peters 2022; ``SafeOpt.ise_point`` on a grid) by a swarm.  It needs no
        Lipschitz constant and no width rule.

        1. The refusals below come before anything is drawn or run.
        2. ``_recheck_safe_set()`` runs once.
        3. Targets ``z_t``: an int ``T`` -- one ``np.random.rand(T, d)`` scaled into
           ``bounds`` -- or ``(T, d)`` rows, nothing drawn.  ``about='unsafe'`` (default) drops
           the targets that are certified safe (``mean_g - beta sd_g >= fmin_g`` for every GP
           with a finite ``fmin_g``, one ``predict_noiseless`` per GP); ``'all'`` keeps every
           one (``ise_targets``).
        4. One swarm (``DeviceSwarmOptimization(..., 'ise')``; ``pso='host'``: the reference
           loop over ``_compute_ise_fitness``) starts from ``swarm_size`` draws from ``S`` and
           runs ``max_iters`` (default ``self.max_iters``) iterations.  The fitness of a
           particle is ``alpha(x) + total_pen`` with ``alpha(x) = max_t sum_{g active} I_g(x;
           z_t)``, ``I_g`` the term of ``SafeOpt.ise_point`` from the posterior covariance of
           particle and target, formed on the device inside the swarm iteration
           (``k_swarm_ise``, ``csrc/swarm_ise.hip``), under the penalty and safety rule of
           the maximizers swarm.  The pick is the personal best with the largest value among
           those that are safe under the current posterior (one ``safe_set`` fitness call),
           the lowest index among equals.
        5. Returns ``(x (d,), alpha)``, ``alpha`` from one fitness call on ``x`` alone (a
           particle's bits do not depend on the swarm it sits in); with ``return_state=True``
           ``(x, alpha, {'targets' (T', d), 'target' (d,): the z attained, 'zmean', 'zvar' (G,
           T')})``.

        Raises ``ValueError`` for ``targets`` outside ``1 .. SGP_MAX_ISE`` (4096) or an array
        that is not ``(T, d)`` or not finite, an ``about`` other than ``'unsafe'`` / ``'all'``,
        a ``max_iters`` below 1, or when no ``fmin`` is finite; ``NotImplementedError`` for several ranks whose
        communicator carries no device context; ``RuntimeError`` when the safe set is empty
        or the swarm ends with no safe personal best, its subclass ``NoIseTarget`` when no
        target is left.

        Changes no state of the optimiser beyond what ``_recheck_safe_set`` does.  NumPy's
        global generator is consumed in this order:

        1. with an int ``targets``, one ``rand(T, d)``;
        2. ``pso='device-rng'`` only: one ``randint`` for the key of the swarm's device
           generator;
        3. one swarm's worth, as step 3 of ``mes_point``.

        N ranks (``comm=``; SPMD, the same seed and call on every rank): the targets are a
        function of replicated data and the shared seed; one ``allreduce_max`` of a digest
        verifies that the ranks hold the same, ``ValueError`` on every rank otherwise.  The
        swarm is split over the ranks by particle (``sgp_swarm_run_ise_shard``); the
        ``safe_set`` call and the pick run replicated on the gathered personal bests: the
        bits of the one-rank run on every rank.

        Out of scope: optimising ``z`` jointly with ``x`` (the paper's continuous variant),
        target proposals concentrated at the boundary of ``S``, batches of ISE picks."""
        targets = self._ise_refusals(targets, about)
        iters = self.max_iters if max_iters is None else int(max_iters)
        if iters < 1:
            raise ValueError("max_iters must be at least 1, got %r" % (max_iters,))
        world = self._comm.world
        if world > 1 and getattr(self._comm, 'ctx', None) is None:
            raise NotImplementedError(
                "the sharded 'ise' swarm merges the global best in the stream of the "
                "communicator's device context: a merge over this host-only communicator of "
                "%d ranks is not implemented" % world)
        self._recheck_safe_set()

        def posterior(rows):
            post = [gp.predict_noiseless(rows) for gp in self.gps]
            return (np.stack([np.asarray(m).reshape(-1) for m, _ in post]),
                    np.stack([np.asarray(v).reshape(-1) for _, v in post]))

        ise = ise_targets(targets, self.bounds, about, self.fmin, self.beta(self.t), posterior)
        if world > 1:
            check_same_targets(self._comm, *ise)
        swarm = None                      # pso='host': a reference loop
        if isinstance(self.swarms['maximizers'], DeviceSwarmOptimization):
            swarm = DeviceSwarmOptimization(
                self.swarm_size, self.optimal_velocities, self, 'ise',
                bounds=self.bounds, rng=self.swarms['maximizers']._rng, comm=self._comm)
        x, _ = self._side_swarm_pick(
            swarm, lambda run: run.set_targets(*ise),
            partial(self._compute_ise_fitness, ise), iters)
        _, _, out = self._compute_ise_fitness(ise, x[None, :], want=('alpha', 'target'))
        alpha = float(out['alpha'][0])
        if return_state:
            return x, alpha, dict(targets=ise[0], target=ise[0][int(out['target'][0])],
                                  zmean=ise[1], zvar=ise[2])
        return x, alpha

    def info_point(self, paths=16, features=1024, targets=256, about='unsafe'):
        """ISE-BO (Bottero et al. 2023) without a grid: the ``mes_point`` pick (what a
        measurement tells about the VALUE of the safe optimum) or the ``ise_point`` pick (what
        it tells about the SAFETY of another point), whichever acquisition is larger -- both
        are mutual informations in nats.  Returns ``(x, alpha, which)``, ``which`` in
        ``{'mes', 'ise'}``; MES wins a tie, and is returned when no target is left for ISE
        (``NoIseTarget``, that outcome alone: every other error of either pick propagates).
        ``paths`` / ``features`` as for ``mes_point`` (floor ``'mean'``), ``targets`` /
        ``about`` as for ``ise_point``, whose argument refusals come before anything is drawn.
        NumPy's generator: what ``mes_point`` draws, then what ``ise_point`` draws."""
        self._ise_refusals(targets, about)
        xm, am = self.mes_point(paths=paths, features=features)
        try:
            xi, ai = self.ise_point(targets=targets, about=about)
        except NoIseTarget:               # (and nothing else: every other error is an error)
            return xm, am, 'mes'
        if ai > am:
            return xi, ai, 'ise'
        return xm, am, 'mes'

    # -- one swarm run, in the steps of gp_opt.py:1015-1134 -------------------------
    def _recheck_safe_set(self):
        """The stored safe points under the CURRENT posterior: raise if none is
        safe any more, drop the unsafe ones unless that would leave fewer than
        one swarm's worth of points."""
        _, still_safe = self._compute_particle_fitness('safe_set', self.S)
        kept = int(still_safe.sum())
        if kept == 0:
            raise RuntimeError('The safe set is empty.')
        if self.swarm_size <= kept < len(still_safe):
            logging.warning("Warning: {} unsafe points removed. "
                            "Model might be violated"
                            .format(np.count_nonzero(~still_safe)))
            self.S = self.S[still_safe]

    def _initial_particles(self, swarm_type):
        """Start positions: uniform draws (with replacement, NumPy's global
        stream -- one ``randint`` call, as in the reference) from the safe set;
        the greedy swarm swaps three of them for the previous greedy point, the
        newest observation and the best observation."""
        fixed = []
        if swarm_type == 'greedy':
            fixed = [self.greedy_point, self.gp.X[-1, :],
                     self.gp.X[np.argmax(self.gp.Y)]]
        picks = np.random.randint(self.S.shape[0],
                                  size=self.swarm_size - len(fixed))
        return np.vstack([self.S[picks, :]] + fixed)

    def _grow_safe_set(self, swarm, swarm_type):
        """Append the swarm's personal bests that are at most 0.95-correlated
        (prior correlation of GP 0) with everything already in the safe set,
        in order.  The correlation filter runs on the device (``sgp_swarm_grow``);
        the m x (|S| + m) covariance matrix of gp_opt.py:1093 is never formed."""
        gp0 = self.gp._fitted()
        keep = _hip.swarm_grow(gp0.ctx, gp0, self.S, swarm.best_positions,
                               self.scaling[0] ** 2, 0.95)
        added = int(np.count_nonzero(keep))
        if added:
            self.S = np.vstack((self.S, swarm.best_positions[keep]))
        logging.debug("At the end of swarm {}, {} points were appended to"
                      " the safeset".format(swarm_type, added))

    def _lower_bound_at(self, x, beta):
        mean, var = self.gp.predict_noiseless(x[None, :])
        return mean.squeeze() - beta * np.sqrt(var.squeeze())

    def get_new_query_point(self, swarm_type):
        """Run one swarm (``'greedy' | 'maximizers' | 'expanders'``).

        Returns ``(global_best, value)`` for the greedy swarm and
        ``(global_best, std_devs)`` -- one posterior standard deviation per GP
        at the chosen point -- otherwise.
        """
        beta = self.beta(self.t)
        self._recheck_safe_set()

        swarm = self.swarms[swarm_type]
        swarm.init_swarm(self._initial_particles(swarm_type))
        swarm.run_swarm(self.max_iters)

        if swarm_type == 'greedy':
            # keep the better of the old and the new estimate of the optimum
            best_value = np.max(swarm.best_values)
            if self._lower_bound_at(self.greedy_point, beta) < best_value:
                self.greedy_point = swarm.global_best.copy()
            return swarm.global_best.copy(), best_value

        self._grow_safe_set(swarm, swarm_type)
        point = swarm.global_best
        std = np.sqrt([gp.predict_noiseless(point[None, :])[1].item()
                       for gp in self.gps])
        return point, std

    def optimize(self, ucb=False):
        """One SafeOptSwarm step; returns the next parameters to evaluate:
        the best maximiser, or the best expander when that one is at least as
        uncertain (``ucb=True``: always the maximiser)."""
        self.greedy, self.best_lower_bound = self.get_new_query_point('greedy')

        x_maxi, std_maxi = self.get_new_query_point('maximizers')
        if ucb:
            logging.info('Using ucb criterion.')
            return x_maxi
        x_exp, std_exp = self.get_new_query_point('expanders')

        # expander uncertainty: only GPs that carry a constraint and are above
        # the threshold count, each in units of its prior std
        counts = (std_exp >= self.threshold) & (self.fmin != -np.inf)
        std_exp = np.max(np.where(counts, std_exp, 0.) / self.scaling)
        std_maxi = std_maxi[0] / self.scaling[0]

        logging.info("The best maximizer has std. dev. %f" % std_maxi)
        logging.info("The best expander has std. dev. %f" % std_exp)
        logging.info("The greedy estimate of lower bound has value %f" %
                     self.best_lower_bound)
        return x_maxi if std_maxi > std_exp else x_exp

    def get_maximum(self):
        """Best observed point ``(x, y)``."""
        maxi = np.argmax(self.gp.Y)
        return self.gp.X[maxi, :], self.gp.Y[maxi]
