"""Constrained particle swarm used by ``SafeOptSwarm`` (host side).

Same behaviour as ``/root/reference/safeopt/swarm.py:17-146``: the update
order, the two ``np.random.rand`` draws per call site (``:75`` once per
``init_swarm``, ``:104`` once per iteration, shape ``(2*swarm_size, ndim)``)
and the aliasing quirks (``positions`` is the caller's array, ``best_values``
is the fitness output, ``global_best`` is a view into ``best_positions``) are
kept, because the chosen point of ``SafeOptSwarm.optimize`` depends on them.
Only the fitness callback does arithmetic of any size, and that runs on the
GPU (``SafeOptSwarm._compute_particle_fitness``).
"""
from __future__ import annotations

import numpy as np

__all__ = ['SwarmOptimization', 'DeviceSwarmOptimization']


class SwarmOptimization(object):
    """Particle swarm maximising ``fitness`` subject to a safety mask.

    Parameters
    ----------
    swarm_size : int
    velocity : ndarray
        Velocity scale per dimension.
    fitness : callable
        ``fitness(positions) -> (values, safe_mask)``.
    bounds : list of (low, high), optional
        Box the particles are clipped to.
    """

    def __init__(self, swarm_size, velocity, fitness, bounds=None):
        self.c1 = self.c2 = 1
        self.fitness = fitness
        self.bounds = None if bounds is None else np.asarray(bounds)
        self.initial_inertia = 1.0
        self.final_inertia = 0.1
        self.velocity_scale = velocity
        self.ndim = len(velocity)
        self.swarm_size = swarm_size

        shape = (swarm_size, self.ndim)
        self.positions = np.empty(shape, dtype=float)
        self.velocities = np.empty(shape, dtype=float)
        self.best_positions = np.empty(shape, dtype=float)
        self.best_values = np.empty(swarm_size, dtype=float)
        self.global_best = None

    @property
    def max_velocity(self):
        """Velocity clip: ten times the velocity scale."""
        return 10 * self.velocity_scale

    def init_swarm(self, positions):
        """Start a run from ``positions`` (kept by reference).

        One ``np.random.rand(swarm_size, ndim)`` draw for the velocities; the
        global best is the arg-max of the raw fitness (the safety mask is not
        applied here, as in the reference)."""
        self.positions = positions
        draw = np.random.rand(*self.velocities.shape)
        self.velocities = draw * self.velocity_scale
        fit, _mask = self.fitness(self.positions)
        np.copyto(self.best_positions, self.positions)
        self.best_values = fit
        self._pick_global_best()

    def _pick_global_best(self):
        # a view into best_positions, first index among equal values
        self.global_best = self.best_positions[int(np.argmax(self.best_values)), :]

    def _move(self, inertia):
        """Velocity and position update of one iteration (one draw of
        ``np.random.rand(2 * swarm_size, ndim)``: own pull first, then global).
        The expression order is part of the contract -- bit-identical runs."""
        pull_global = self.global_best - self.positions
        pull_own = self.best_positions - self.positions
        u = np.random.rand(2 * self.swarm_size, self.ndim)
        u_own, u_global = u[:self.swarm_size], u[self.swarm_size:]
        v = self.velocities
        v *= inertia
        v += (self.c1 * u_own * pull_own +
              self.c2 * u_global * pull_global) / self.velocity_scale
        limit = self.max_velocity
        np.clip(v, -limit, limit, out=v)
        x = self.positions
        x += v
        if self.bounds is not None:
            np.clip(x, self.bounds[:, 0], self.bounds[:, 1], out=x)

    def _keep_improvements(self):
        """Personal bests move only to safe points with a higher fitness."""
        fit, mask = self.fitness(self.positions)
        take = (fit > self.best_values) & mask
        self.best_values[take] = fit[take]
        self.best_positions[take] = self.positions[take]
        self._pick_global_best()

    def run_swarm(self, max_iter):
        """Iterate the swarm ``max_iter`` times, inertia going linearly from
        ``initial_inertia`` towards ``final_inertia``."""
        step = (self.final_inertia - self.initial_inertia) / max_iter
        inertia = self.initial_inertia
        for _ in range(max_iter):
            self._move(inertia)
            inertia += step
            self._keep_improvements()

def _hip_swarm_types():
    from . import _hip
    return _hip.SWARM_TYPES


#: type code of the Thompson swarm in the Philox seed mix (``_hip.SWARM_TYPES`` holds 0..3,
#: the types ``sgp_swarm_fitness`` takes; a Thompson swarm has entry points of its own)
THOMPSON_CODE = 4
#: ... and of the max-value entropy search swarm (``kSwarmMes`` on the C side)
MES_CODE = 5
#: ... and of the information-theoretic safe exploration swarm (``kSwarmIse``)
ISE_CODE = 6
#: ... and of the expected-improvement swarm (``kSwarmEi``)
EI_CODE = 7


class DeviceSwarmOptimization(SwarmOptimization):
    """The same swarm with its state in HBM: ``init_swarm`` and ``run_swarm``
    are one C-ABI call each (``sgp_swarm_run``) -- velocity / position update,
    fused posterior fitness, personal and global bests all run on the GPU and
    nothing crosses PCIe between iterations.

    ``rng='numpy'`` (default): the uniform numbers are drawn with
    ``np.random.rand`` on the host exactly where and in the order the reference
    draws them (``swarm.py:75, 104``) and shipped with the call, so the run --
    and the state of NumPy's global generator afterwards -- is bit-identical to
    :class:`SwarmOptimization`.  ``rng='device'``: a counter-based generator
    on the GPU (Philox4x32-10); nothing but the swarm state is transferred,
    results are reproducible per ``seed`` but differ from ``np.random``.

    ``owner`` is the :class:`SafeOptSwarm` whose GPs / beta / fmin / scaling /
    best lower bound define the fitness of ``swarm_type``.

    ``comm`` with ``world > 1``: every rank runs its contiguous block of the
    particles (``shard_range``, ``sgp_swarm_run_shard``) and the global best is
    merged over the ranks on the device.  Every rank draws the initial particles
    and NumPy's numbers as the one-rank run does and uses its own rows; Philox
    draws the numbers of the block's global elements.  After a run
    ``best_positions`` / ``best_values`` are gathered over the ranks (the whole
    swarm on every rank); ``positions`` / ``velocities`` stay the rank's block.

    ``swarm_type='thompson'``: the fitness is the value of one posterior sample path of
    the owner's objective GP under the maximizers' penalty and safety rule
    (``sgp_swarm_fitness_path`` / ``sgp_swarm_run_path``); ``set_path(path)`` with ``path =
    (Omega, phase, w, v)`` comes before ``init_swarm``; with ``comm`` it is sharded like
    every other swarm (``sgp_swarm_run_path_shard``), every rank holding the same path.

    ``set_clones(clones)`` on a ``'maximizers'`` or ``'expanders'`` swarm: a hallucinated
    swarm of ``SafeOptSwarm.optimize_batch`` -- the width term of the fitness comes from the
    clones of the owner's GPs, which carry the pending picks (``sgp_swarm_fitness_hall`` /
    ``sgp_swarm_run_hall``); with ``comm`` it is sharded like every other swarm
    (``sgp_swarm_run_hall_shard``), every rank holding clones with the same pending picks.

    ``swarm_type='mes'``: max-value entropy search -- the fitness is ``alpha + total_pen``,
    ``alpha`` the acquisition of ``GPRegression.max_value_entropy`` on the posterior of the
    owner's objective GP, under the maximizers' penalty and safety rule
    (``sgp_swarm_fitness_mes`` / ``sgp_swarm_run_mes``); ``set_maxima(ystar, floor)`` comes
    before ``init_swarm``; with ``comm`` it is sharded like every other swarm
    (``sgp_swarm_run_mes_shard``), every rank holding the same maxima and floor.

    ``swarm_type='ise'``: information-theoretic safe exploration -- the fitness is ``alpha +
    total_pen``, ``alpha[p]`` the largest mutual information between a measurement at the
    particle and the safety of one of a fixed set of targets, under the maximizers' penalty
    and safety rule (``sgp_swarm_fitness_ise`` / ``sgp_swarm_run_ise``);
    ``set_targets(targets, zmean, zvar)`` comes before ``init_swarm``; with ``comm`` it is
    sharded like every other swarm (``sgp_swarm_run_ise_shard``), every rank holding the same
    targets.

    ``swarm_type='ei'``: expected improvement -- the fitness is ``alpha + total_pen``, ``alpha``
    the logarithm of ``Context.ei_eval`` (LogEI, log-PI, optionally weighed by the probability
    of feasibility) on the posterior of the owner's GPs, under the maximizers' penalty and
    safety rule -- or, ``free``, ``alpha`` alone with every particle counted safe
    (``sgp_swarm_fitness_ei`` / ``sgp_swarm_run_ei``); ``set_incumbent(kind, tau, xi,
    feasibility, free)`` comes before ``init_swarm``; with ``comm`` it is sharded like every
    other swarm (``sgp_swarm_run_ei_shard``), every rank holding the same incumbent.
    """

    def __init__(self, swarm_size, velocity, owner, swarm_type, bounds=None,
                 rng='numpy', seed=None, comm=None):
        super(DeviceSwarmOptimization, self).__init__(
            swarm_size, velocity, None, bounds=bounds)
        del self.fitness          # (the base class stored None over the method below)
        if rng not in ('numpy', 'device'):
            raise ValueError("rng must be 'numpy' or 'device'")
        from .dist import LocalComm, shard_range
        self._comm = comm if comm is not None else LocalComm()
        if self._comm.world > 1 and not callable(getattr(self._comm, 'allgather', None)):
            raise NotImplementedError(
                "a sharded swarm gathers its personal bests through the communicator's "
                "allgather: this communicator of %d ranks implements none" % self._comm.world)
        self._rows = shard_range(swarm_size, self._comm.rank, self._comm.world)
        self._owner = owner
        self._type = swarm_type
        self._rng = rng
        # Philox key of the device generator: `seed`, or one draw from NumPy's
        # global stream (so np.random.seed controls it and every swarm object gets
        # its own), mixed with the swarm type -- the greedy / maximizers /
        # expanders swarms of one optimiser must not draw the same numbers
        if rng == 'device' and seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        code = {'thompson': THOMPSON_CODE, 'mes': MES_CODE, 'ise': ISE_CODE,
                'ei': EI_CODE}.get(swarm_type)
        if code is None:
            code = _hip_swarm_types()[swarm_type]
        self._seed = (int(seed or 0) * 4 + code) & (2 ** 43 - 1)
        self._calls = 0
        self._path = None
        self._clones = None
        self._maxima = None
        self._targets = None
        self._incumbent = None
        self.global_best = np.zeros(self.ndim)

    def set_path(self, path):
        """The sample path ``(Omega, phase, w, v)`` a Thompson swarm climbs from the next
        ``init_swarm`` on."""
        if self._type != 'thompson':
            raise ValueError("only a 'thompson' swarm takes a path, this is %r" % (self._type,))
        self._path = path

    def set_clones(self, clones):
        """The clones of the owner's device GPs with the pending picks of a batch appended:
        from the next ``init_swarm`` on the swarm is a hallucinated one (``None``: a plain
        one again)."""
        if clones is not None:
            if self._type not in ('maximizers', 'expanders'):
                raise ValueError("only a 'maximizers' or an 'expanders' swarm takes clones, "
                                 "this is %r" % (self._type,))
            clones = list(clones)
        self._clones = clones

    def set_maxima(self, ystar, floor=None):
        """The maxima ``ystar`` (``1 .. SGP_MAX_MES`` finite values) and the ``floor`` under
        them (``None``: none; a float, +-inf allowed) a 'mes' swarm scores its particles with
        from the next ``init_swarm`` on."""
        if self._type != 'mes':
            raise ValueError("only a 'mes' swarm takes maxima, this is %r" % (self._type,))
        from . import _hip
        ystar = np.array(ystar, dtype=float).reshape(-1)
        if ystar.size < 1 or ystar.size > _hip.MAX_MES:
            raise ValueError("%d maxima, a 'mes' swarm takes 1 .. SGP_MAX_MES = %d"
                             % (ystar.size, _hip.MAX_MES))
        if not np.all(np.isfinite(ystar)):
            raise ValueError("a maximum is not finite")
        floor = -np.inf if floor is None else float(floor)
        if np.isnan(floor):
            raise ValueError("the floor is NaN")
        self._maxima = (ystar, floor)

    def set_targets(self, targets, zmean, zvar):
        """The targets ``(T, d)``, ``1 <= T <= SGP_MAX_ISE`` finite rows, and their noiseless
        posterior ``zmean`` / ``zvar`` ``(G, T)`` (finite, every variance ``>= 0``) an 'ise'
        swarm scores its particles with from the next ``init_swarm`` on.  The arrays are
        copied; a refused call leaves the swarm as it was."""
        if self._type != 'ise':
            raise ValueError("only an 'ise' swarm takes targets, this is %r" % (self._type,))
        from . import _hip
        targets = np.array(targets, dtype=float)
        if targets.ndim != 2 or targets.shape[1] != self.ndim:
            raise ValueError("targets must be (T, d) with d = %d, got %r"
                             % (self.ndim, targets.shape))
        T = targets.shape[0]
        if T < 1 or T > _hip.MAX_ISE:
            raise ValueError("%d targets, an 'ise' swarm takes 1 .. SGP_MAX_ISE = %d"
                             % (T, _hip.MAX_ISE))
        zmean, zvar = np.array(zmean, dtype=float), np.array(zvar, dtype=float)
        gps = getattr(self._owner, 'gps', None)
        G = len(gps) if gps is not None else (zmean.shape[0] if zmean.ndim == 2 else 0)
        if G < 1 or zmean.shape != (G, T) or zvar.shape != (G, T):
            raise ValueError("zmean and zvar must be (G, T) = (%d, %d), got %r and %r"
                             % (G, T, zmean.shape, zvar.shape))
        if not (np.all(np.isfinite(targets)) and np.all(np.isfinite(zmean))
                and np.all(np.isfinite(zvar))):
            raise ValueError("a target, a mean or a variance is not finite")
        if np.any(zvar < 0):
            raise ValueError("a variance is negative")
        self._targets = (np.ascontiguousarray(targets), np.ascontiguousarray(zmean),
                         np.ascontiguousarray(zvar))

    def set_incumbent(self, kind, tau, xi=0.0, feasibility=False, free=False):
        """What an 'ei' swarm scores its particles with from the next ``init_swarm`` on:
        ``kind`` ``'ei'`` (log expected improvement) or ``'pi'`` (log probability of
        improvement), the finite incumbent ``tau``, the finite margin ``xi >= 0``,
        ``feasibility`` (weigh by the probability that every constraint holds) and ``free``
        (no penalty, no safety rule: every particle counts as safe).  A refused call leaves
        the swarm as it was."""
        if self._type != 'ei':
            raise ValueError("only an 'ei' swarm takes an incumbent, this is %r" % (self._type,))
        if kind not in ('ei', 'pi'):
            raise ValueError("kind must be 'ei' or 'pi', got %r" % (kind,))
        tau, xi = float(tau), float(xi)
        if not np.isfinite(tau):
            raise ValueError("the incumbent must be finite, got %r" % (tau,))
        if not (np.isfinite(xi) and xi >= 0.0):
            raise ValueError("xi must be finite and >= 0, got %r" % (xi,))
        self._incumbent = (kind, tau, xi, bool(feasibility), bool(free))

    def _need_incumbent(self):
        if self._incumbent is None:
            raise ValueError("an 'ei' swarm needs set_incumbent(kind, tau, xi, feasibility, free) "
                             "before init_swarm")
        return self._incumbent

    def _need_targets(self):
        if self._targets is None:
            raise ValueError("an 'ise' swarm needs set_targets(targets, zmean, zvar) before "
                             "init_swarm")
        return self._targets

    def _need_maxima(self):
        if self._maxima is None:
            raise ValueError("a 'mes' swarm needs set_maxima(ystar, floor) before init_swarm")
        return self._maxima

    def _need_path(self):
        if self._path is None:
            raise ValueError("a 'thompson' swarm needs set_path(path) before init_swarm")
        return self._path

    def fitness(self, positions):                 # kept for API parity
        if self._type == 'thompson':
            return self._owner._compute_path_fitness(self._need_path(), positions)
        if self._type == 'mes':
            maxima = self._need_maxima()
            return self._owner._compute_mes_fitness(maxima, positions)
        if self._type == 'ise':
            targets = self._need_targets()
            return self._owner._compute_ise_fitness(targets, positions)
        if self._type == 'ei':
            incumbent = self._need_incumbent()
            return self._owner._compute_ei_fitness(incumbent, positions)
        if self._clones is not None:
            return self._owner._compute_hall_fitness(self._type, self._clones, positions)
        return self._owner._compute_particle_fitness(self._type, positions)

    def _device_run(self, init, iters, inertia0, step):
        from . import _hip
        # (a missing path, missing maxima, targets or a missing incumbent are refused before
        # anything is touched or drawn)
        path = self._need_path() if self._type == 'thompson' else None
        maxima = self._need_maxima() if self._type == 'mes' else None
        targets = self._need_targets() if self._type == 'ise' else None
        incumbent = self._need_incumbent() if self._type == 'ei' else None
        o = self._owner
        devs = [g._fitted() for g in o.gps]
        sharded = self._comm.world > 1
        d = self.positions.shape[1]
        P = self.swarm_size if sharded else self.positions.shape[0]
        self._calls += 1
        rand = None
        if self._rng == 'numpy':
            # the whole swarm's numbers on every rank, as one rank draws them
            rand = np.random.rand((P * d if init else 0) + 2 * P * d * iters)
            if sharded:
                rand = self._rows_of_draws(rand, init, iters)
        # (sharded: the rank's block of the personal bests is the run's state between calls)
        best_positions, best_values = (
            (self._local['best_positions'], self._local['best_values']) if sharded
            else (self.best_positions, self.best_values))
        _hip._swarm_run(
            devs[0].ctx, devs, self._type, (o.beta(o.t), o.fmin, o.scaling, o.best_lower_bound),
            (self.positions, self.velocities, best_positions, best_values, self.global_best,
             np.broadcast_to(self.velocity_scale, (d,)), self.bounds),
            (init, iters, inertia0, step, rand, (self._seed << 20) + self._calls),
            path=path, clones=self._clones, mes=maxima, ise=targets, ei=incumbent,
            shard=(self._rows[0], self.swarm_size) if sharded else None)
        if sharded:
            self.best_positions, self.best_values = self._gather(best_positions, best_values)

    def _rows_of_draws(self, rand, init, iters):
        """This rank's rows of every draw of the whole swarm: init's ``(P, d)``, then per
        iteration the r1 and r2 rows of ``(2 P, d)``."""
        (lo, hi), P, d = self._rows, self.swarm_size, self.positions.shape[1]
        parts, at = [], 0
        if init:
            parts.append(rand[lo * d:hi * d])
            at = P * d
        for _ in range(iters):
            it = rand[at:at + 2 * P * d]
            parts += [it[lo * d:hi * d], it[(P + lo) * d:(P + hi) * d]]
            at += 2 * P * d
        return np.concatenate(parts) if parts else None

    def _gather(self, best_positions, best_values):
        """The whole swarm's personal bests on every rank (blocks padded to one size)."""
        from .dist import allgather_rows, shard_range
        world, P = self._comm.world, self.swarm_size
        part = np.empty((best_values.shape[0], best_positions.shape[1] + 1))
        part[:, :-1] = best_positions
        part[:, -1] = best_values
        full = allgather_rows(self._comm, part, [hi - lo for lo, hi in (
            shard_range(P, r, world) for r in range(world))])
        return np.ascontiguousarray(full[:, :-1]), np.ascontiguousarray(full[:, -1])

    def init_swarm(self, positions):
        if self._type == 'thompson':
            self._need_path()
        if self._type == 'mes':
            self._need_maxima()
        if self._type == 'ise':
            self._need_targets()
        if self._type == 'ei':
            self._need_incumbent()
        positions = np.ascontiguousarray(positions, dtype=float)
        if self._comm.world > 1:
            lo, hi = self._rows
            positions = np.ascontiguousarray(positions[lo:hi])
        self.positions = positions
        shape = self.positions.shape
        self.velocities = np.empty(shape)
        self.best_positions = np.empty(shape)
        self.best_values = np.empty(shape[0])
        self.global_best = np.empty(shape[1])
        # the rank's block of the personal bests (the run's state between calls)
        self._local = dict(best_positions=self.best_positions, best_values=self.best_values)
        self._device_run(True, 0, self.initial_inertia, 0.0)

    def run_swarm(self, max_iter):
        step = (self.final_inertia - self.initial_inertia) / max_iter
        self._device_run(False, max_iter, self.initial_inertia, step)
