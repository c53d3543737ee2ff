"""Host side of ``SafeOptSwarm.thompson_points`` (no GPU): the pick rule, the reference swarm
loop under a stub path fitness, and that the NumPy reference of the GPU penalty test leaves no
particle out (tests/_swarm_thompson_ref.py)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _swarm_thompson_ref as ref


# ---- the pick rule -----------------------------------------------------------------------------

def _pick(*a):
    from safeopt_amd.gp_opt import thompson_pick
    return thompson_pick(*a)


def test_pick_takes_the_largest_safe_value():
    pos = np.arange(10.0).reshape(5, 2)
    x, i = _pick(pos, [0.1, 0.7, 0.3, 0.6, -1.0], [True] * 5)
    assert i == 1
    assert_array_equal(x, pos[1])
    x[0] = 99.0                                  # a copy, not a view into the swarm
    assert pos[1, 0] == 2.0


def test_pick_lowest_index_wins_a_tie():
    pos = np.arange(12.0).reshape(6, 2)
    vals = [0.2, 0.9, 0.9, 0.1, 0.9, 0.0]
    assert _pick(pos, vals, [True] * 6)[1] == 1
    assert _pick(pos, vals, [True, False, True, True, True, True])[1] == 2
    assert _pick(pos, [3.0] * 6, [False, False, False, True, True, False])[1] == 3


def test_pick_skips_an_unsafe_argmax():
    pos = np.arange(8.0).reshape(4, 2)
    x, i = _pick(pos, [5.0, 1.0, 2.0, -3.0], [False, True, True, True])
    assert i == 2
    assert_array_equal(x, pos[2])
    assert _pick(pos, [5.0, 1.0, 2.0, -3.0], [False, False, False, True])[1] == 3


def test_pick_none_safe_raises():
    with pytest.raises(RuntimeError, match="There are no safe points to sample in."):
        _pick(np.zeros((3, 2)), [1.0, 2.0, 3.0], [False, False, False])
    with pytest.raises(RuntimeError):
        _pick(np.zeros((0, 2)), [], [])


# ---- the reference loop under a stub path fitness ----------------------------------------------

def test_host_loop_two_iterations_by_hand(monkeypatch):
    """``SwarmOptimization`` with a path-fitness stub (value = -(x - 1)^2, safe iff x <= 1.5)
    against the two iterations worked out by hand: 2 particles, 1-D, velocity scale 0.5,
    bounds [-2, 2], the uniform numbers fixed.  Inertia 1.0, then 0.55."""
    from safeopt_amd.swarm import SwarmOptimization

    calls = []

    def fitness(x):
        calls.append(x.copy())
        return -(x[:, 0] - 1.0) ** 2, x[:, 0] <= 1.5

    draws = iter([np.array([[0.5], [1.0]]),                     # init: velocities / scale
                  np.array([[0.5], [0.5], [0.25], [0.5]]),      # it 1: own rows, global rows
                  np.array([[1.0], [1.0], [0.5], [1.0]])])      # it 2
    monkeypatch.setattr(np.random, "rand", lambda *shape: next(draws))
    sw = SwarmOptimization(2, np.array([0.5]), fitness, bounds=[(-2.0, 2.0)])
    sw.init_swarm(np.array([[0.0], [2.0]]))
    # velocities 0.25, 0.5; values -1, -1: a tie, particle 0 is the global best (unmasked)
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
    assert_array_equal(calls[1], [[0.25], [0.5]])
    np.testing.assert_allclose(sw.velocities, [[0.3875], [-0.825]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.positions, [[0.6375], [-0.325]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_positions, [[0.6375], [0.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_values, [-0.13140625, -0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.global_best, [0.6375], rtol=0, atol=1e-15)


def test_host_loop_keeps_an_unsafe_improvement_out():
    """A particle that climbs the path into the unsafe region does not move its personal best."""
    from safeopt_amd.swarm import SwarmOptimization
    rs = np.random.RandomState(5)
    state = np.random.get_state()
    try:
        np.random.set_state(rs.get_state())
        sw = SwarmOptimization(6, np.array([0.3]), lambda x: (x[:, 0].copy(), x[:, 0] <= 0.2),
                               bounds=[(-1.0, 1.0)])
        sw.init_swarm(np.linspace(-0.5, 0.1, 6)[:, None])
        sw.run_swarm(15)
    finally:
        np.random.set_state(state)
    assert np.all(sw.best_positions <= 0.2)
    assert_array_equal(sw.best_values, sw.best_positions[:, 0])


# ---- the device swarm's argument handling (no device call is reached) --------------------------

def test_thompson_swarm_objects():
    from safeopt_amd.swarm import DeviceSwarmOptimization, THOMPSON_CODE
    from safeopt_amd import _hip
    assert THOMPSON_CODE == 4 and THOMPSON_CODE not in _hip.SWARM_TYPES.values()
    assert _hip.SWARM_TYPES == {"greedy": 0, "maximizers": 1, "expanders": 2, "safe_set": 3}
    sw = DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'thompson', seed=3)
    assert sw._seed == 3 * 4 + 4
    with pytest.raises(ValueError, match="set_path"):
        sw.init_swarm(np.zeros((5, 2)))
    other = DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'maximizers', seed=3)
    with pytest.raises(ValueError, match="thompson"):
        other.set_path((None,) * 4)

    class World2(object):
        rank, world = 0, 2
    with pytest.raises(NotImplementedError, match="sharded"):
        DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'thompson', comm=World2())
    for name in ("sgp_swarm_fitness_path", "sgp_swarm_run_path"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.swarm_fitness_path) and callable(_hip.swarm_run_path)


# ---- the NumPy reference of the GPU penalty test leaves no particle out ------------------------

@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_reference_slacks_keep_clear_of_the_band_edges(case):
    low = ref.lower_bounds(case)
    fmin = np.array(ref.fmin_of(case))
    scaled = (low - fmin[:, None]) / ref.SCALING[:, None]
    assert scaled.min() >= -0.9 - 1e-12           # slope of the penalty at most 10 per GP
    assert not ref.near_band_edge(scaled).any()
    safe = np.all(scaled >= 0, axis=0)
    assert 0 < safe.sum() < safe.size or case[4] == 1     # the constraints split the particles
    # ... and every band of the penalty above -1 is met somewhere
    assert np.any((scaled < 0) & (scaled > -0.001)) or np.any((scaled <= -0.1))
