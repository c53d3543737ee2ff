"""Host side of ``SafeOptSwarm.ei_point`` (no GPU): the 'ei' swarm object, the reference swarm
loop under a stub EI fitness, the argument refusals that reach no device, the agreement check of
the ranks, and the conditions the GPU tests put on their inputs, checked on the NumPy reference
alone (tests/_swarm_ei_ref.py)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _ei_ref
import _swarm_ei_ref as ref
from safeopt_amd.dist import LocalComm, check_same_incumbent
from safeopt_amd.swarm import (SwarmOptimization, DeviceSwarmOptimization, EI_CODE, ISE_CODE,
                               MES_CODE, THOMPSON_CODE)


# ---- the 'ei' swarm object (no device call is reached) -----------------------------------------

def _ei_swarm(**kw):
    return DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'ei', **kw)


def test_ei_swarm_object():
    from safeopt_amd import _hip
    assert EI_CODE == 7 and len({EI_CODE, ISE_CODE, MES_CODE, THOMPSON_CODE}) == 4
    assert EI_CODE not in _hip.SWARM_TYPES.values() and "ei" not in _hip.SWARM_TYPES
    sw = _ei_swarm(seed=3)
    assert sw._seed == 3 * 4 + 7
    # a run before set_incumbent is refused: init_swarm, run_swarm and the fitness callback
    with pytest.raises(ValueError, match="set_incumbent"):
        sw.init_swarm(np.zeros((5, 2)))
    with pytest.raises(ValueError, match="set_incumbent"):
        sw.run_swarm(3)
    with pytest.raises(ValueError, match="set_incumbent"):
        sw.fitness(np.zeros((5, 2)))
    # another swarm type takes no incumbent
    for other in ('maximizers', 'thompson', 'mes'):
        with pytest.raises(ValueError, match="only an 'ei' swarm"):
            DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, other,
                                    seed=3).set_incumbent('ei', 0.5)
    # ... and an 'ei' swarm neither a path, clones, maxima nor targets
    with pytest.raises(ValueError, match="thompson"):
        sw.set_path((None,) * 4)
    with pytest.raises(ValueError, match="maximizers"):
        sw.set_clones([None])
    with pytest.raises(ValueError, match="only a 'mes' swarm"):
        sw.set_maxima([0.5])
    with pytest.raises(ValueError, match="only an 'ise' swarm"):
        sw.set_targets(np.zeros((1, 2)), np.zeros((1, 1)), np.ones((1, 1)))

    class World2(object):
        rank, world = 0, 2
    with pytest.raises(NotImplementedError, match="sharded"):
        _ei_swarm(comm=World2())
    for name in ("sgp_swarm_fitness_ei", "sgp_swarm_run_ei", "sgp_swarm_run_ei_shard"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.swarm_fitness_ei) and callable(_hip.swarm_run_ei)
    # the tail of the C argument list: kind by name or by code, the switches as 0 / 1
    assert _hip._swarm_ei_args(('pi', 1, 0, True, False)) == (_hip.EI_PI, 1.0, 0.0, 1, 0)
    assert _hip._swarm_ei_args((_hip.EI_EI, 0.5, 0.25, 0, 1)) == (_hip.EI_EI, 0.5, 0.25, 0, 1)


def test_set_incumbent_validation():
    sw = _ei_swarm(seed=1)
    with pytest.raises(ValueError, match="kind must be 'ei' or 'pi'"):
        sw.set_incumbent('ucb', 0.5)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="incumbent must be finite"):
            sw.set_incumbent('ei', bad)
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="xi must be finite and >= 0"):
            sw.set_incumbent('ei', 0.5, bad)
    assert sw._incumbent is None                 # a refused call leaves nothing behind
    sw.set_incumbent('ei', 0.5)
    assert sw._incumbent == ('ei', 0.5, 0.0, False, False)
    sw.set_incumbent('pi', np.float32(1.5), 1, feasibility=1, free=True)
    assert sw._incumbent == ('pi', 1.5, 1.0, True, True)
    assert [type(v) for v in sw._incumbent] == [str, float, float, bool, bool]
    with pytest.raises(ValueError):              # ... nor does a refused second call
        sw.set_incumbent('ei', np.nan)
    assert sw._incumbent == ('pi', 1.5, 1.0, True, True)


# ---- the reference loop under a stub EI fitness ------------------------------------------------

def test_host_loop_two_iterations_by_hand(monkeypatch):
    """The host loop of ``ei_point`` with ``pso='host'`` -- ``SwarmOptimization`` over the
    fitness callback of an 'ei' swarm -- against two iterations worked out by hand.  The owner
    is a stub whose ``_compute_ei_fitness((kind, tau, xi, feasibility, free), x)`` is value =
    -(x - tau)^2, safe iff x <= xi, with tau = 1, xi = 1.5: 2 particles, 1-D, velocity scale
    0.5, bounds [-2, 2], the uniform numbers fixed.  Inertia 1.0, then 0.55."""
    calls = []

    class Owner(object):
        def _compute_ei_fitness(self, ei, x):
            kind, tau, xi, feasibility, free = ei
            calls.append((ei, x.copy()))
            return -(x[:, 0] - tau) ** 2, x[:, 0] <= xi

    dev = DeviceSwarmOptimization(2, np.array([0.5]), Owner(), 'ei', seed=0)
    dev.set_incumbent('pi', 1.0, 1.5, feasibility=True)
    draws = iter([np.array([[0.5], [1.0]]),                     # init: velocities / scale
                  np.array([[0.5], [0.5], [0.25], [0.5]]),      # it 1: own rows, global rows
                  np.array([[1.0], [1.0], [0.5], [1.0]])])      # it 2
    monkeypatch.setattr(np.random, "rand", lambda *shape: next(draws))
    sw = SwarmOptimization(2, np.array([0.5]), dev.fitness, bounds=[(-2.0, 2.0)])
    sw.init_swarm(np.array([[0.0], [2.0]]))
    # velocities 0.25, 0.5; values -1, -1: a tie, particle 0 is the global best (unmasked:
    # particle 1 at x = 2 > xi is not safe, and init_swarm does not ask)
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
    for ei, _x in calls:                         # every call carried the whole incumbent
        assert ei == ('pi', 1.0, 1.5, True, False)
    assert_array_equal(calls[1][1], [[0.25], [0.5]])
    np.testing.assert_allclose(sw.velocities, [[0.3875], [-0.825]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.positions, [[0.6375], [-0.325]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_positions, [[0.6375], [0.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_values, [-0.13140625, -0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.global_best, [0.6375], rtol=0, atol=1e-15)


def test_unchecked_pick_makes_no_safe_set_call_and_draws_as_the_checked_one(monkeypatch):
    """``_side_swarm_pick(..., unchecked=True)`` -- the pick of ``within='bounds'`` -- takes the
    largest personal best, the lowest index among equals, without a ``'safe_set'`` call; the
    default is the checked pick, and both consume the generator alike."""
    from safeopt_amd import SafeOptSwarm
    opt = object.__new__(SafeOptSwarm)
    opt.S = np.array([[0.0], [0.5], [1.0]])
    opt.swarm_size, opt.optimal_velocities, opt.bounds = 4, np.array([0.5]), [(-2.0, 2.0)]
    asked = []

    def safe_set(swarm_type, x):
        asked.append(swarm_type)
        return None, x[:, 0] < 0.6
    monkeypatch.setattr(opt, "_compute_particle_fitness", safe_set, raising=False)

    def fitness(x):                              # two equal maxima: x = 0.5 and x = 1.5
        return -np.abs(np.abs(x[:, 0] - 1.0) - 0.5), np.ones(len(x), dtype=bool)
    states = []
    picks = []
    for unchecked in (True, False):
        np.random.seed(4)
        kw = dict(unchecked=True) if unchecked else {}
        picks.append(opt._side_swarm_pick(None, None, fitness, 3, **kw))
        states.append(np.random.get_state()[1].copy())
    assert asked == ['safe_set']                 # the checked pick alone asked
    assert_array_equal(states[0], states[1])
    (xu, iu), (xc, ic) = picks
    np.random.seed(4)
    start = opt.S[np.random.randint(3, size=4), :]
    sw = SwarmOptimization(4, opt.optimal_velocities, fitness, bounds=opt.bounds)
    sw.init_swarm(start.copy())
    sw.run_swarm(3)
    assert iu == int(np.argmax(sw.best_values)) and xu == sw.best_positions[iu]
    assert np.count_nonzero(sw.best_values == sw.best_values.max()) > 1      # equals: the lowest
    ok = np.flatnonzero(sw.best_positions[:, 0] < 0.6)
    assert 0 < ok.size < 4 and ic == ok[np.argmax(sw.best_values[ok])]


# ---- ei_point: the refusals that come before any draw or device call ---------------------------

def test_ei_point_refuses_bad_arguments_before_anything_runs():
    from safeopt_amd import SafeOptSwarm
    opt = object.__new__(SafeOptSwarm)           # no GP, no device: nothing may be reached
    opt._y = np.full((3, 2), np.nan)
    opt._y[:, 1] = 1.0                           # (a constraint's values are not the objective's)
    state = np.random.get_state()[1].copy()
    for within in ('all', 'MG', 'S', None):
        with pytest.raises(ValueError, match="within must be 'safe' or 'bounds'"):
            opt.ei_point(within=within)
    with pytest.raises(ValueError, match="kind must be 'ei' or 'pi'"):
        opt.ei_point(kind='ucb')
    for bad in (-1e-9, np.nan, np.inf):
        with pytest.raises(ValueError, match="xi must be finite and >= 0"):
            opt.ei_point(xi=bad)
    with pytest.raises(ValueError, match="incumbent must be 'mean', 'data' or a float"):
        opt.ei_point(incumbent='best')
    with pytest.raises(ValueError, match="the objective has no measurement"):
        opt.ei_point(incumbent='data')
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="the incumbent must be finite"):
            opt.ei_point(incumbent=bad)

    class World2(object):                        # several ranks, no device context
        rank, world = 0, 2
    opt._comm = World2()
    for within in ('safe', 'bounds'):
        with pytest.raises(NotImplementedError, match="sharded 'ei' swarm"):
            opt.ei_point(incumbent=0.5, within=within)
    assert_array_equal(np.random.get_state()[1], state)      # nothing was drawn


def test_check_same_incumbent():
    class Other(object):
        """A second rank that holds ``delta`` more in its digest."""
        rank, world = 0, 2

        def __init__(self, delta):
            self.delta = delta

        def allreduce_max(self, a):
            b = np.array([a[0] + self.delta, -(a[0] + self.delta)])
            return np.maximum(a, b)
    ei = ('ei', 0.5, 0.0, False, False)
    check_same_incumbent(LocalComm(), *ei)
    check_same_incumbent(Other(0.0), *ei)
    for delta in (1.0, -1.0):
        with pytest.raises(ValueError, match="different incumbents"):
            check_same_incumbent(Other(delta), *ei)

    # the digest tells every one of the five apart: record what each variant sends
    class Record(object):
        rank, world = 0, 1

        def __init__(self):
            self.seen = []

        def allreduce_max(self, a):
            self.seen.append(float(a[0]))
            return np.array(a)
    rec = Record()
    variants = [ei, ('pi', 0.5, 0.0, False, False), ('ei', 0.5 + 2.0 ** -53, 0.0, False, False),
                ('ei', 0.5, 0.25, False, False), ('ei', 0.5, 0.0, True, False),
                ('ei', 0.5, 0.0, False, True), ('ei', 0.0, 0.5, False, False)]
    for v in variants:
        check_same_incumbent(rec, *v)
    assert len(set(rec.seen)) == len(variants)
    assert all(h == int(h) and 0 <= h < 2.0 ** 48 for h in rec.seen)


# ---- the conditions on the inputs of the GPU tests, on the reference alone ---------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_incumbents_reach_the_branches_they_aim_at(case):
    """The claims of tests/_swarm_ei_ref.py's docstring, on the NumPy posterior of the case:
    'max+2' puts every particle into the middle form of ``ei_log_h``, 'max+1e7' every particle
    into the asymptotic form; 'median' puts particles on both sides of z = -1 in the cases
    ``BOTH_SIDES`` names and keeps every particle of the others in the direct form (a lone
    particle at z = 0 exactly).  Every reference alpha is finite."""
    name = ref.IDS[ref.CASES.index(case)]
    z = ref.z_of(case, 'max+2')
    assert np.all((z >= _ei_ref.Z_ASYMPT) & (z < _ei_ref.Z_DIRECT))
    z = ref.z_of(case, 'max+1e7')
    assert np.all(z < _ei_ref.Z_ASYMPT)
    z = ref.z_of(case, 'median')
    assert np.all(z >= _ei_ref.Z_ASYMPT)
    if name in ref.BOTH_SIDES:
        assert np.any(z >= _ei_ref.Z_DIRECT) and np.any(z < _ei_ref.Z_DIRECT)
    else:
        assert np.all(z >= _ei_ref.Z_DIRECT)
    if case[4] == 1:
        assert z[0] == 0.0
    fmin = ref.fmin_of(case)
    for which in ref.INCUMBENTS:
        for kind in ref.KINDS:
            for f in (None, fmin):
                for G in (1, 2):
                    a = ref.alpha(case, which, kind, f, G)
                    assert a.shape == (case[4],) and np.all(np.isfinite(a))
    # the weights are really there: ln Phi <= 0 at every particle (0 once Phi rounds to 1),
    # below 0 at some
    weighed, plain = ref.alpha(case, 'median', 'ei', fmin), ref.alpha(case, 'median', 'ei')
    assert np.all(weighed <= plain) and np.any(weighed < plain)


def test_both_sides_cases_cover_every_family_and_route():
    """The cases in which 'median' reaches both forms around z = -1 hold every n (posterior
    kernel family), both posterior routes (P = 37: few points, P = 5000: the sweep) and both
    input dimensions; with them the three forms of ``ei_log_h`` are all reached."""
    cases = [c for c, i in zip(ref.CASES, ref.IDS) if i in ref.BOTH_SIDES]
    assert len(cases) == len(ref.BOTH_SIDES) == 5
    assert sorted(set(c[2] for c in cases)) == [5, 60, 300]
    assert sorted(set(c[4] for c in cases)) == [37, 5000]
    assert sorted(set(c[1] for c in cases)) == [1, 3]
    assert ref.INCUMBENTS == ['median', 'max+2', 'max+1e7']
    assert ref.PENALTY_INCUMBENTS == ['median', 'max+2']
    assert len(ref.CASES) == 9 and ref.XI == 0.0


@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_reference_slacks_leave_out_at_most_one_percent(case):
    """The band-edge cap of the penalty test, a condition on its inputs: at most 1 % of a
    case's particles have a reference scaled slack within 1e-9 of a penalty band edge."""
    low = ref.lower_bounds(case)
    fmin = np.array(ref.fmin_of(case))
    scaled = (low - fmin[:, None]) / ref.SCALING[:, None]
    assert scaled.min() >= -0.9 - 1e-12           # slope of the penalty at most 10 per GP
    assert np.count_nonzero(ref.near_band_edge(scaled)) <= 0.01 * case[4]
    safe = np.all(scaled >= 0, axis=0)
    assert 0 < safe.sum() < safe.size             # the constraints split the particles
