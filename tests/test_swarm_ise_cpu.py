"""Host side of ``SafeOptSwarm.ise_point`` (no GPU): the 'ise' swarm object, ``ise_targets``, the
reference swarm loop under a stub fitness, the argument refusals that reach no device, and the
conditions the GPU tests put on their inputs, checked on the long-double reference alone
(tests/_swarm_ise_ref.py)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _swarm_ise_ref as ref


# ---- the 'ise' swarm object (no device call is reached) ----------------------------------------

def _ise_swarm(**kw):
    from safeopt_amd.swarm import DeviceSwarmOptimization
    return DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, 'ise', **kw)


def test_ise_swarm_object():
    from safeopt_amd.swarm import DeviceSwarmOptimization, ISE_CODE, MES_CODE, THOMPSON_CODE
    from safeopt_amd import _hip
    assert ISE_CODE == 6 and ISE_CODE not in (MES_CODE, THOMPSON_CODE)
    assert ISE_CODE not in _hip.SWARM_TYPES.values() and "ise" not in _hip.SWARM_TYPES
    sw = _ise_swarm(seed=3)
    assert sw._seed == 3 * 4 + 6
    # a run before set_targets is refused: init_swarm, run_swarm and the fitness callback
    with pytest.raises(ValueError, match="set_targets"):
        sw.init_swarm(np.zeros((5, 2)))
    with pytest.raises(ValueError, match="set_targets"):
        sw.run_swarm(3)
    with pytest.raises(ValueError, match="set_targets"):
        sw.fitness(np.zeros((5, 2)))
    # another swarm type takes no targets
    for other in ('maximizers', 'thompson', 'mes'):
        with pytest.raises(ValueError, match="only an 'ise' swarm"):
            DeviceSwarmOptimization(5, np.array([0.1, 0.1]), None, other, seed=3).set_targets(
                np.zeros((1, 2)), np.zeros((1, 1)), np.ones((1, 1)))
    # ... and an 'ise' swarm neither a path, clones nor maxima
    with pytest.raises(ValueError, match="thompson"):
        sw.set_path((None,) * 4)
    with pytest.raises(ValueError, match="maximizers"):
        sw.set_clones([None])
    with pytest.raises(ValueError, match="only a 'mes' swarm"):
        sw.set_maxima([1.0])

    class World2(object):
        rank, world = 0, 2
    with pytest.raises(NotImplementedError, match="sharded"):
        _ise_swarm(comm=World2())
    for name in ("sgp_swarm_fitness_ise", "sgp_swarm_run_ise", "sgp_swarm_run_ise_shard"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.swarm_fitness_ise) and callable(_hip.swarm_run_ise)

    class Gp(object):
        d = 2
    with pytest.raises(NotImplementedError, match="an 'ise' swarm takes neither"):
        _hip._swarm_call(None, "sgp_swarm_run", [Gp()], None, None, None, mes=([1.0], 0.0),
                         ise=(np.zeros((1, 2)), np.zeros((1, 1)), np.ones((1, 1))))


def test_set_targets_validation():
    from safeopt_amd import _hip
    sw = _ise_swarm(seed=1)
    tg, zm, zv = np.zeros((3, 2)), np.zeros((2, 3)), np.ones((2, 3))
    with pytest.raises(ValueError, match="SGP_MAX_ISE"):
        sw.set_targets(np.zeros((0, 2)), np.zeros((2, 0)), np.zeros((2, 0)))
    with pytest.raises(ValueError, match="SGP_MAX_ISE"):
        sw.set_targets(np.zeros((_hip.MAX_ISE + 1, 2)), np.zeros((1, _hip.MAX_ISE + 1)),
                       np.zeros((1, _hip.MAX_ISE + 1)))
    for bad in (np.zeros(3), np.zeros((3, 3)), np.zeros((3, 2, 1))):
        with pytest.raises(ValueError, match=r"\(T, d\)"):
            sw.set_targets(bad, zm, zv)
    with pytest.raises(ValueError, match=r"\(G, T\)"):
        sw.set_targets(tg, zm[:, :2], zv)
    with pytest.raises(ValueError, match=r"\(G, T\)"):
        sw.set_targets(tg, zm, zv[:1])
    for which in range(3):
        for bad in (np.nan, np.inf):
            arrs = [tg.copy(), zm.copy(), zv.copy()]
            arrs[which][1, 1] = bad
            with pytest.raises(ValueError, match="not finite"):
                sw.set_targets(*arrs)
    neg = zv.copy()
    neg[0, 2] = -1e-9
    with pytest.raises(ValueError, match="negative"):
        sw.set_targets(tg, zm, neg)
    assert sw._targets is None                   # a refused call leaves nothing behind
    sw.set_targets(tg, zm, zv)
    tg[0, 0] = 9.0                               # copies, not the caller's arrays
    zv[0, 0] = 9.0
    assert sw._targets[0][0, 0] == 0.0 and sw._targets[2][0, 0] == 1.0
    assert [a.shape for a in sw._targets] == [(3, 2), (2, 3), (2, 3)]
    held = sw._targets
    with pytest.raises(ValueError, match="negative"):
        sw.set_targets(tg, zm, neg)
    assert sw._targets is held                   # ... nor replaces what a good call left
    sw.set_targets(np.zeros((_hip.MAX_ISE, 2)), np.zeros((1, _hip.MAX_ISE)),
                   np.zeros((1, _hip.MAX_ISE)))  # the cap itself, a variance of 0


# ---- ise_targets -------------------------------------------------------------------------------

def _posterior_from(table):
    """A hand-made posterior: ``(zmean, zvar)`` (2, T) looked up by the rows' first column."""
    def posterior(rows):
        zm = np.array([[table[float(r[0])][g][0] for r in rows] for g in range(2)])
        zv = np.array([[table[float(r[0])][g][1] for r in rows] for g in range(2)])
        return zm, zv
    return posterior


def test_ise_targets_draws_one_rand_and_scales_it(monkeypatch):
    from safeopt_amd.gp_opt import ise_targets
    calls = []
    u = np.array([[0.0, 0.5], [1.0, 0.25], [0.5, 1.0]])

    def rand(*shape):
        calls.append(shape)
        return u
    monkeypatch.setattr(np.random, "rand", rand)
    seen = []

    def posterior(rows):
        seen.append(rows.copy())
        return np.zeros((1, len(rows))), np.ones((1, len(rows)))
    rows, zm, zv = ise_targets(3, [(-1.0, 1.0), (2.0, 6.0)], 'all', np.array([0.0]), 2.0,
                               posterior)
    assert calls == [(3, 2)]                     # ONE rand(T, d)
    assert_array_equal(rows, [[-1.0, 4.0], [1.0, 3.0], [0.0, 6.0]])
    assert len(seen) == 1                        # ONE posterior call
    assert_array_equal(seen[0], rows)
    assert zm.shape == (1, 3) and zv.shape == (1, 3)
    # rows given: nothing is drawn
    given = np.array([[0.5, 2.5]])
    rows, _, _ = ise_targets(given, [(-1.0, 1.0), (2.0, 6.0)], 'all', np.array([0.0]), 2.0,
                             posterior)
    assert calls == [(3, 2)]
    assert_array_equal(rows, given)
    assert rows is not given


def test_ise_targets_unsafe_filter_against_a_hand_made_posterior():
    from safeopt_amd.gp_opt import ise_targets
    # beta = 2, fmin = [0, -inf, ...]: GP 1 carries no constraint.  Per row (mean, var) of GP 0:
    #   row 0: 1.0, 0.25 -> lower 0.0  >= 0: certified safe (the bound itself is safe)
    #   row 1: 1.0, 0.36 -> lower -0.2 <  0: kept
    #   row 2: 3.0, 1.0  -> lower 1.0: safe;  row 3: -1.0, 0.0 -> lower -1: kept
    table = {0.0: ((1.0, 0.25), (-50.0, 1.0)), 1.0: ((1.0, 0.36), (50.0, 1.0)),
             2.0: ((3.0, 1.0), (-50.0, 1.0)), 3.0: ((-1.0, 0.0), (50.0, 1.0))}
    rows = np.array([[0.0], [1.0], [2.0], [3.0]])
    post = _posterior_from(table)
    out, zm, zv = ise_targets(rows, [(0.0, 3.0)], 'unsafe', np.array([0.0, -np.inf]), 2.0, post)
    assert_array_equal(out, [[1.0], [3.0]])
    assert_array_equal(zm, [[1.0, -1.0], [50.0, 50.0]])
    assert_array_equal(zv, [[0.36, 0.0], [1.0, 1.0]])
    # both GPs active: a row is certified only when EVERY active bound holds
    out, _, _ = ise_targets(rows, [(0.0, 3.0)], 'unsafe', np.array([0.0, 0.0]), 2.0, post)
    assert_array_equal(out, [[0.0], [1.0], [2.0], [3.0]])       # GP 1 fails rows 0 and 2
    out, _, _ = ise_targets(rows, [(0.0, 3.0)], 'unsafe', np.array([0.0, -60.0]), 2.0, post)
    assert_array_equal(out, [[1.0], [3.0]])
    # 'all' keeps every row
    out, zm, _ = ise_targets(rows, [(0.0, 3.0)], 'all', np.array([0.0, -np.inf]), 2.0, post)
    assert_array_equal(out, rows)
    assert zm.shape == (2, 4)
    # no row left
    from safeopt_amd.gp_opt import NoIseTarget
    with pytest.raises(NoIseTarget, match="no target is left"):
        ise_targets(rows[[0, 2]], [(0.0, 3.0)], 'unsafe', np.array([0.0, -np.inf]), 2.0, post)
    with pytest.raises(ValueError, match="'unsafe' or 'all'"):
        ise_targets(rows, [(0.0, 3.0)], 'safe', np.array([0.0, -np.inf]), 2.0, post)


# ---- the reference loop under a stub fitness ---------------------------------------------------

def test_host_loop_two_iterations_by_hand(monkeypatch):
    """The host loop of ``ise_point`` with ``pso='host'`` -- ``SwarmOptimization`` over the
    fitness callback of an 'ise' swarm -- against two iterations worked out by hand
    (tests/test_swarm_mes_host.py has the same numbers).  The owner is a stub whose
    ``_compute_ise_fitness((targets, zmean, zvar), x)`` is value = -(x - targets[0, 0])^2, safe
    iff x <= zmean[0, 0], with the target 1 and zmean 1.5: 2 particles, 1-D, velocity scale 0.5,
    bounds [-2, 2], the uniform numbers fixed.  Inertia 1.0, then 0.55."""
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization

    calls = []

    class Owner(object):
        gps = [None]

        def _compute_ise_fitness(self, ise, x):
            targets, zmean, zvar = ise
            calls.append((targets.copy(), zmean.copy(), zvar.copy(), x.copy()))
            return -(x[:, 0] - targets[0, 0]) ** 2, x[:, 0] <= zmean[0, 0]

    dev = DeviceSwarmOptimization(2, np.array([0.5]), Owner(), 'ise', seed=0)
    dev.set_targets([[1.0]], [[1.5]], [[0.25]])
    draws = iter([np.array([[0.5], [1.0]]),                     # init: velocities / scale
                  np.array([[0.5], [0.5], [0.25], [0.5]]),      # it 1: own rows, global rows
                  np.array([[1.0], [1.0], [0.5], [1.0]])])      # it 2
    monkeypatch.setattr(np.random, "rand", lambda *shape: next(draws))
    sw = SwarmOptimization(2, np.array([0.5]), dev.fitness, bounds=[(-2.0, 2.0)])
    sw.init_swarm(np.array([[0.0], [2.0]]))
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
    for targets, zmean, zvar, _x in calls:       # every call carried the targets
        assert_array_equal(targets, [[1.0]])
        assert_array_equal(zmean, [[1.5]])
        assert_array_equal(zvar, [[0.25]])
    assert_array_equal(calls[1][3], [[0.25], [0.5]])
    np.testing.assert_allclose(sw.velocities, [[0.3875], [-0.825]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.positions, [[0.6375], [-0.325]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_positions, [[0.6375], [0.5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.best_values, [-0.13140625, -0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(sw.global_best, [0.6375], rtol=0, atol=1e-15)


# ---- ise_point: the refusals that come before any draw or device call --------------------------

def test_ise_point_refuses_bad_arguments_before_anything_runs():
    from safeopt_amd import SafeOptSwarm, _hip

    class Gp(object):
        input_dim = 2
    opt = object.__new__(SafeOptSwarm)           # no device: nothing may be reached
    opt.gps = [Gp()]
    opt.gp = opt.gps[0]
    opt.fmin = np.array([0.0])
    opt.max_iters = 100
    state = np.random.get_state()[1].copy()
    for call in (opt.ise_point, lambda **kw: opt.info_point(paths=2, **kw)):
        for T in (0, -3, _hip.MAX_ISE + 1):
            with pytest.raises(ValueError, match="SGP_MAX_ISE"):
                call(targets=T)
        for bad in (np.zeros(3), np.zeros((3, 3)), np.zeros((0, 2)),
                    np.zeros((_hip.MAX_ISE + 1, 2))):
            with pytest.raises(ValueError, match=r"\(T, d\)"):
                call(targets=bad)
        for bad in (np.nan, np.inf):
            with pytest.raises(ValueError, match="not finite"):
                call(targets=np.array([[0.0, bad]]))
        with pytest.raises(ValueError, match="'unsafe' or 'all'"):
            call(about='safe')
        if call == opt.ise_point:
            for bad in (0, -2):
                with pytest.raises(ValueError, match="max_iters"):
                    call(max_iters=bad)
        opt.fmin = np.array([-np.inf])
        with pytest.raises(ValueError, match="no GP is active"):
            call(targets=4)
        opt.fmin = np.array([0.0])

    class World2(object):                        # several ranks, no device context
        rank, world = 0, 2
    opt._comm = World2()
    with pytest.raises(NotImplementedError, match="sharded 'ise' swarm"):
        opt.ise_point(targets=4)
    assert_array_equal(np.random.get_state()[1], state)      # nothing was drawn


def test_info_point_answers_no_target_left_with_mes_and_nothing_else():
    """``info_point`` returns the MES pick when ``ise_point`` has no target left
    (``NoIseTarget``); every other error -- a device error is a ``RuntimeError`` too -- goes
    through."""
    from safeopt_amd import SafeOptSwarm, _hip
    from safeopt_amd.gp_opt import NoIseTarget
    assert issubclass(NoIseTarget, RuntimeError) and issubclass(_hip.HipError, RuntimeError)
    assert not issubclass(_hip.HipError, NoIseTarget)

    class Gp(object):
        input_dim = 1

    def optimiser(ise):
        opt = object.__new__(SafeOptSwarm)
        opt.gps = [Gp()]
        opt.gp = opt.gps[0]
        opt.fmin = np.array([0.0])
        opt.mes_point = lambda **kw: (np.array([0.25]), 0.5)
        opt.ise_point = ise
        return opt

    def raising(exc):
        def ise(**kw):
            raise exc
        return ise
    x, alpha, which = optimiser(raising(NoIseTarget("no target is left"))).info_point()
    assert which == 'mes' and alpha == 0.5 and x[0] == 0.25
    for exc in (RuntimeError("no safe personal best"), _hip.HipError("hipErrorOutOfMemory"),
                ValueError("different targets")):
        with pytest.raises(type(exc), match=str(exc)):
            optimiser(raising(exc)).info_point()
    x, alpha, which = optimiser(lambda **kw: (np.array([0.75]), 0.6)).info_point()
    assert which == 'ise' and alpha == 0.6 and x[0] == 0.75
    x, alpha, which = optimiser(lambda **kw: (np.array([0.75]), 0.5)).info_point()
    assert which == 'mes'                        # MES wins a tie


def test_check_same_targets():
    from safeopt_amd.dist import LocalComm, check_same_targets, _digest48

    class Other(object):
        """A second rank that holds ``delta`` more in its digest."""
        rank, world = 0, 2

        def __init__(self, delta):
            self.delta = delta

        def allreduce_max(self, a):
            b = np.array([a[0] + self.delta, -(a[0] + self.delta)])
            return np.maximum(a, b)
    tg, zm, zv = np.array([[0.5, 1.5], [1.0, 2.0]]), np.zeros((1, 2)), np.ones((1, 2))
    check_same_targets(LocalComm(), tg, zm, zv)
    check_same_targets(Other(0.0), tg, zm, zv)
    for delta in (1.0, -1.0):
        with pytest.raises(ValueError, match="different targets"):
            check_same_targets(Other(delta), tg, zm, zv)
    # the digest tells the targets, their order, their shape and their posterior apart
    assert len({_digest48((tg, zm, zv)), _digest48((tg[::-1], zm, zv)),
                _digest48((tg.reshape(1, 4), zm, zv)), _digest48((tg, zm + 1, zv)),
                _digest48((tg, zm, zv * 2))}) == 5


# ---- the conditions on the inputs of the GPU tests, on the reference alone ---------------------

def test_cases_cover_every_shape():
    assert len(ref.CASES) == len(ref.IDS) == len(set(ref.IDS)) == 12
    assert sum(1 for c in ref.CASES if c[5] == "mid") == 1
    assert sum(1 for c in ref.CASES if c[5] == "twin") == 1
    mid = [c for c in ref.CASES if c[5] == "mid"][0]
    assert_array_equal(ref.fmin_open(mid), [0.2, -np.inf, -0.3])
    twin = [c for c in ref.CASES if c[5] == "twin"][0]
    s = ref.specs(twin)
    assert s[0] == s[1]
    for case in ref.CASES:
        X, Y, particles, targets = ref.problem(case)
        assert X.shape == (case[2], case[1]) and Y.shape == (case[2], len(ref.specs(case)))
        assert particles.shape == (case[3], case[1]) and targets.shape == (case[4], case[1])


@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_reference_pairs_are_not_degenerate(case):
    """Every case has a pair above 1e-6 nats; every case with more than one target has a
    particle whose attained target is not target 0 (with one target there is no other), and
    maxima that are unique (the permutation test maps targets back); with the open fmin every
    particle is safe by a margin the device's posterior error cannot close."""
    fmin = ref.fmin_open(case)
    pr, al, tg = ref.pairs(case, fmin)
    P, T = case[3], case[4]
    assert pr.shape == (P, T) and np.all(np.isfinite(pr)) and np.all(pr >= 0)
    assert pr.max() > 1e-6
    if T > 1:
        assert np.any(tg != 0)
        srt = np.sort(pr, axis=1)
        assert np.all(srt[:, -1] > srt[:, -2])
    if case[5] != "mid":
        low = ref.lower_bounds(case)
        assert np.all(low - fmin[:, None] >= ref.OPEN_MARGIN * (1 - 1e-12))
        assert np.all(np.isfinite(fmin))
    else:
        safe = np.all((ref.lower_bounds(case) >= fmin[:, None])[np.isfinite(fmin)], axis=0)
        assert 0 < safe.sum() < P


@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_reference_slacks_leave_out_at_most_one_percent(case):
    low = ref.lower_bounds(case)
    fmin = ref.fmin_split(case)
    G = low.shape[0]
    scaled = (low - fmin[:, None]) / ref.SCALING[:G, None]
    assert scaled.min() >= -0.9 - 1e-12           # slope of the penalty at most 10 per GP
    assert np.count_nonzero(ref.near_band_edge(scaled)) <= 0.01 * case[3]
    safe = np.all(scaled >= 0, axis=0)
    assert 0 < safe.sum() < safe.size             # the constraints split the particles
