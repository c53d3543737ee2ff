"""Host side of ``SafeOptSwarm.mes_point`` (no GPU): the 'mes' swarm object, the reference swarm
loop under a stub MES fitness, the argument refusals that reach no device, and the conditions
the GPU tests put on their inputs, checked on the NumPy reference alone
(tests/_swarm_mes_ref.py)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _swarm_mes_ref as ref


# ---- the 'mes' swarm object (no device call is reached) ----------------------------------------

def _mes_swarm(**kw):
    from safeopt_amd.swarm import DeviceSwarmOptimization
    return DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'mes', **kw)


def test_mes_swarm_object():
    from safeopt_amd.swarm import DeviceSwarmOptimization, MES_CODE, THOMPSON_CODE
    from safeopt_amd import _hip
    assert MES_CODE == 5 and MES_CODE != THOMPSON_CODE
    assert MES_CODE not in _hip.SWARM_TYPES.values() and "mes" not in _hip.SWARM_TYPES
    sw = _mes_swarm(seed=3)
    assert sw._seed == 3 * 4 + 5
    # a run before set_maxima is refused: init_swarm, run_swarm and the fitness callback
    with pytest.raises(ValueError, match="set_maxima"):
        sw.init_swarm(np.zeros((5, 2)))
    with pytest.raises(ValueError, match="set_maxima"):
        sw.run_swarm(3)
    with pytest.raises(ValueError, match="set_maxima"):
        sw.fitness(np.zeros((5, 2)))
    # another swarm type takes no maxima
    for other in ('maximizers', 'thompson'):
        with pytest.raises(ValueError, match="only a 'mes' swarm"):
            DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, other,
                                    seed=3).set_maxima([1.0], 0.0)
    # ... and a 'mes' swarm neither a path nor clones
    with pytest.raises(ValueError, match="thompson"):
        sw.set_path((None,) * 4)
    with pytest.raises(ValueError, match="maximizers"):
        sw.set_clones([None])

    class World2(object):
        rank, world = 0, 2
    with pytest.raises(NotImplementedError, match="sharded"):
        _mes_swarm(comm=World2())
    for name in ("sgp_swarm_fitness_mes", "sgp_swarm_run_mes", "sgp_swarm_run_mes_shard"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.swarm_fitness_mes) and callable(_hip.swarm_run_mes)


def test_set_maxima_validation():
    from safeopt_amd import _hip
    sw = _mes_swarm(seed=1)
    with pytest.raises(ValueError, match="SGP_MAX_MES"):
        sw.set_maxima([])
    with pytest.raises(ValueError, match="SGP_MAX_MES"):
        sw.set_maxima(np.zeros(_hip.MAX_MES + 1))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="not finite"):
            sw.set_maxima([0.5, bad])
    with pytest.raises(ValueError, match="floor is NaN"):
        sw.set_maxima([0.5], np.nan)
    assert sw._maxima is None                    # a refused call leaves nothing behind
    ys = [0.5, 1.5]
    sw.set_maxima(ys)                            # no floor: -inf
    assert_array_equal(sw._maxima[0], ys)
    assert sw._maxima[1] == -np.inf
    ys[0] = 9.0                                  # a copy, not the caller's list
    assert sw._maxima[0][0] == 0.5
    for floor in (0.25, np.inf, -np.inf):
        sw.set_maxima(np.zeros(_hip.MAX_MES), floor)
        assert sw._maxima[1] == floor and sw._maxima[0].shape == (_hip.MAX_MES,)


# ---- the reference loop under a stub MES fitness -----------------------------------------------

def test_host_loop_two_iterations_by_hand(monkeypatch):
    """The host loop of ``mes_point`` with ``pso='host'`` -- ``SwarmOptimization`` over the
    fitness callback of a 'mes' swarm -- against two iterations worked out by hand.  The owner
    is a stub whose ``_compute_mes_fitness((ystar, floor), x)`` is value = -(x - ystar[0])^2,
    safe iff x <= floor, with ystar = [1], floor = 1.5: 2 particles, 1-D, velocity scale 0.5,
    bounds [-2, 2], the uniform numbers fixed.  Inertia 1.0, then 0.55."""
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization

    calls = []

    class Owner(object):
        def _compute_mes_fitness(self, mes, x):
            ystar, floor = mes
            calls.append((ystar.copy(), floor, x.copy()))
            return -(x[:, 0] - ystar[0]) ** 2, x[:, 0] <= floor

    dev = DeviceSwarmOptimization(2, np.array([0.5]), Owner(), 'mes', seed=0)
    dev.set_maxima([1.0], 1.5)
    draws = iter([np.array([[0.5], [1.0]]),                     # init: velocities / scale
                  np.array([[0.5], [0.5], [0.25], [0.5]]),      # it 1: own rows, global rows
                  np.array([[1.0], [1.0], [0.5], [1.0]])])      # it 2
    monkeypatch.setattr(np.random, "rand", lambda *shape: next(draws))
    sw = SwarmOptimization(2, np.array([0.5]), dev.fitness, bounds=[(-2.0, 2.0)])
    sw.init_swarm(np.array([[0.0], [2.0]]))
    # velocities 0.25, 0.5; values -1, -1: a tie, particle 0 is the global best (unmasked:
    # particle 1 at x = 2 > floor is not safe, and init_swarm does not ask)
    assert_array_equal(sw.velocities, [[0.25], [0.5]])
    assert_array_equal(sw.best_values, [-1.0, -1.0])
    assert_array_equal(sw.global_best, [0.0])
    sw.run_swarm(2)
    # it 1, inertia 1: v0 = 0.25 + (0.5 * 0 + 0.25 * 0) / 0.5 = 0.25          -> x0 = 0.25
    #                  v1 = 0.5 + (0.5 * 0 + 0.5 * (0 - 2)) / 0.5 = -1.5      -> x1 = 0.5
    #   values -0.5625, -0.25, both safe and better: bests move, global best = x1 = 0.5
    # it 2, inertia 0.55: v0 = 0.1375 + (1 * 0 + 0.5 * 0.25) / 0.5 = 0.3875   -> x0 = 0.6375
    #                  v1 = -0.825 + (1 * 0 + 1 * 0) / 0.5 = -0.825           -> x1 = -0.325
    #   values -(0.3625)^2 = -0.13140625 (better), -(1.325)^2 (worse): global best = x0
    assert len(calls) == 3
    for ystar, floor, _x in calls:               # every call carried the maxima and the floor
        assert_array_equal(ystar, [1.0])
        assert floor == 1.5
    assert_array_equal(calls[1][2], [[0.25], [0.5]])
    np.testing.assert_allclose(sw.velocities, [[0.3875], [-0.825]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.positions, [[0.6375], [-0.325]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_positions, [[0.6375], [0.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_values, [-0.13140625, -0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.global_best, [0.6375], rtol=0, atol=1e-15)


# ---- mes_point: the refusals that come before any draw or device call --------------------------

def test_mes_point_refuses_bad_arguments_before_anything_runs():
    from safeopt_amd import SafeOptSwarm, _hip
    opt = object.__new__(SafeOptSwarm)           # no GP, no device: nothing may be reached
    state = np.random.get_state()[1].copy()
    for paths in (0, -3, _hip.MAX_MES + 1):
        with pytest.raises(ValueError, match="SGP_MAX_MES"):
            opt.mes_point(paths=paths)
    with pytest.raises(ValueError, match="SGP_MAX_MES"):
        opt.mes_point(ystar=[])
    with pytest.raises(ValueError, match="SGP_MAX_MES"):
        opt.mes_point(ystar=np.zeros(_hip.MAX_MES + 1))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            opt.mes_point(ystar=[0.1, bad])
    with pytest.raises(ValueError, match="floor is NaN"):
        opt.mes_point(floor=np.nan)
    with pytest.raises(ValueError, match="'mean', None or a float"):
        opt.mes_point(floor='median')

    class World2(object):                        # several ranks, no device context
        rank, world = 0, 2
    opt._comm = World2()
    with pytest.raises(NotImplementedError, match="sharded 'mes' swarm"):
        opt.mes_point(paths=4)
    with pytest.raises(NotImplementedError, match="sharded 'mes' swarm"):
        opt.mes_point(ystar=[0.5], floor=None)
    assert_array_equal(np.random.get_state()[1], state)      # nothing was drawn


def test_check_same_maxima():
    from safeopt_amd.dist import LocalComm, check_same_maxima

    class Other(object):
        """A second rank that holds ``delta`` more in its digest."""
        rank, world = 0, 2

        def __init__(self, delta):
            self.delta = delta

        def allreduce_max(self, a):
            b = np.array([a[0] + self.delta, -(a[0] + self.delta)])
            return np.maximum(a, b)
    ys = np.array([0.5, 1.5])
    check_same_maxima(LocalComm(), ys, -np.inf)
    check_same_maxima(Other(0.0), ys, 0.25)
    for delta in (1.0, -1.0):
        with pytest.raises(ValueError, match="different maxima or floors"):
            check_same_maxima(Other(delta), ys, 0.25)
    # the digest tells the maxima, their order and the floor apart
    from safeopt_amd.dist import _digest48
    d = lambda y, f: _digest48((np.asarray(y, dtype=float), np.array([f])))  # noqa: E731
    assert len({d(ys, 0.25), d(ys[::-1], 0.25), d(ys, 0.5), d(ys, -np.inf), d(ys[:1], 0.25)}) == 5


# ---- the conditions on the inputs of the GPU tests, on the reference alone ---------------------

@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_both_signs_of_gamma_occur_without_a_floor(case):
    """Without a floor the term runs through both of its branches (gamma < 0 and gamma >= 0)
    in every case with more than one particle.  Over the maxima sets without a floor of a
    case -- K = 1 and K = 64 -- both signs occur among the particles; K = 64 alone has both
    (its maxima run from the smallest mean to 2 above the largest), while the one maximum of
    K = 1 is the smallest mean, ``linspace(min, max + 2, 1) = [min]``: gamma <= 0 there by
    construction, negative at every particle but one."""
    g1 = ref.gammas(case, 1, -np.inf)
    g64 = ref.gammas(case, 64, -np.inf)
    both = np.concatenate([g1.ravel(), g64.ravel()])
    assert np.any(both < 0) and np.any(both > 0)
    assert np.any(g64 < 0) and np.any(g64 > 0)
    assert np.all(g1 <= 0) and np.count_nonzero(g1 < 0) >= g1.size - 1
    # under the median floor gamma < 0 survives only above the median of the mean
    g5 = ref.gammas(case, 5, 'median')
    assert np.any(g5 < 0) and np.any(g5 > 0)
    for K, floor in ref.MAXIMA:
        a = ref.alpha(case, K, floor)
        assert a.shape == (case[4],) and np.all(np.isfinite(a))


@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_reference_slacks_leave_out_at_most_one_percent(case):
    low = ref.lower_bounds(case)
    fmin = np.array(ref.fmin_of(case))
    scaled = (low - fmin[:, None]) / ref.SCALING[:, None]
    assert scaled.min() >= -0.9 - 1e-12           # slope of the penalty at most 10 per GP
    assert np.count_nonzero(ref.near_band_edge(scaled)) <= 0.01 * case[4]
    safe = np.all(scaled >= 0, axis=0)
    assert 0 < safe.sum() < safe.size             # the constraints split the particles


def test_cases_cover_every_shape_once():
    keys = [(c[0], c[1], c[2], c[4]) for c in ref.CASES]
    assert len(set(keys)) == len(keys) == len(ref.IDS)
    assert [k for k, _ in ref.MAXIMA] == [1, 5, 64]
    for case in ref.CASES:
        ys, fl = ref.maxima(case, 5, 'median')
        mean = ref.posterior0(case)[0]
        assert ys.shape == (5,) and ys[0] == mean.min() and ys[-1] == mean.max() + 2.0
        assert fl == np.median(mean)
        assert ref.maxima(case, 1, -np.inf)[0][0] == mean.min()
