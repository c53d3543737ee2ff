"""Thompson swarms (``sgp_swarm_fitness_path`` / ``sgp_swarm_run_path``, k_swarm_path in
csrc/paths.hip, ``SafeOptSwarm.thompson_points``) against the NumPy statement of
tests/_swarm_thompson_ref.py (needs an MI355X).  Cases and shapes: that module's docstring.

Tolerances.  Path term: the criterion of ``test_evaluation_entry_by_entry`` (tests/test_gpu_paths.py),
|device - reference| <= c x (sum of the absolute terms of the path), c = max(100 D, (m + n +
8 (d + 2) A) 2^-53), recomputed per case.  Penalty: see ``test_penalty_and_safety``.
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
import _swarm_thompson_ref as ref
from _gpu_common import mods, _swarm_problem, _PretendWorld, MEAN_TOL, VAR_TOL  # noqa: F401

pytestmark = pytest.mark.gpu

_GPS = {}


def device_gps(case):
    """The two GPs of a case on the device (objective, constraint); built once."""
    import safeopt_amd.gpy as gpy
    if case not in _GPS:
        kind, d = case[:2]
        X, Y = ref.problem(*case)[2:4]
        _GPS[case] = [
            gpy.models.GPRegression(X, Y[:, [0]], ref.make_kernel(gpy.kern, kind, d),
                                    noise_var=ref.NOISE),
            gpy.models.GPRegression(X, Y[:, [1]], ref.constraint_kernel(gpy.kern, d),
                                    noise_var=ref.NOISE)]
    return _GPS[case]


@functools.lru_cache(maxsize=None)
def device_path(case):
    """``(Omega, phase, w, v)``: the path of a case, its data weights from the device."""
    Om, b, W, E = ref.problem(*case)[5:]
    V = device_gps(case)[0]._fitted().path_weights(Om, b, W, E)
    path = (Om, b, np.ascontiguousarray(W[:, 0]), np.ascontiguousarray(V[:, 0]))
    for a in path:
        a.setflags(write=False)
    return path


def fitness(case, fmin, G=2, particles=None):
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)[:G]]
    if particles is None:
        particles = ref.problem(*case)[4]
    return _hip.swarm_fitness_path(devs[0].ctx, devs, particles, ref.BETA, fmin[:G],
                                   ref.SCALING[:G], device_path(case))


@functools.lru_cache(maxsize=None)
def unconstrained(case):
    values, safe = fitness(case, np.array([-np.inf, -np.inf]))
    values.setflags(write=False)
    return values, safe


# ---- 1. the path term --------------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_path_term_unconstrained(mods, case, G):
    """fmin = -inf: no penalty, values x scaling[0] is the path term, every particle safe."""
    kind, d, n, m, P = case
    kern0, _, X, _, particles, Om, b, W, _ = ref.problem(*case)
    _, _, w, v = device_path(case)
    values, safe = unconstrained(case) if G == 2 else fitness(case, np.array([-np.inf]), G=1)
    assert values.shape == (P,) and safe.shape == (P,) and safe.dtype == np.bool_
    assert safe.all()
    out = values * ref.SCALING[0]
    V = v[:, None]
    r = pn.paths_eval(kern0, X, Om, b, W, V, particles)[:, 0]
    rl = pn.paths_eval_ld(kern0, X, Om, b, W, V, particles)[:, 0]
    budget = pn.abs_budget(kern0, X, Om, b, W, V, particles)[:, 0]
    Dm = float(np.max(np.abs(r - rl) / budget))
    A = max(1.0, float(np.abs(pn.feature_args(Om, b, particles)).max()))
    c = max(100 * Dm, (m + n + 8 * (d + 2) * A) * 2.0 ** -53)
    err = float(np.max(np.abs(out - r) / budget))
    print("path term: |dev - ref| / budget %.3e, D %.3e, A %.1f, c %.3e, err / c %.3f"
          % (err, Dm, A, c, err / c))
    assert np.all(np.abs(out - r) <= c * budget)


# ---- 2. penalty and safety ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_penalty_and_safety(mods, case):
    """Finite fmin for both GPs: the safety flags are those of the maximizers swarm (same
    posterior, same rule), and values_constrained - values_unconstrained is the penalty of the
    slacks that ``predict_noiseless`` gives on the same device GPs.

    Tolerance.  Both posteriors (the fitness call's and predict_noiseless's) meet the criterion
    of ``_gpu_common.check_posterior`` against the truth: |d mean| <= MEAN_TOL max|mean|, |d var|
    <= VAR_TOL k(x, x); between the two, twice that.  lower = mean - beta sd and |sd - sd'| <=
    min(sqrt(|d var|), |d var| / sd), so per GP |d slack| <= 2 MEAN_TOL max|mean| + beta
    min(sqrt(dv), dv / sd) with dv = 2 VAR_TOL k(x, x).  Every scaled slack lies above -1 (the
    CPU test holds the NumPy reference to -0.9), where the slope of the penalty is at most 10:
    |d penalty| <= sum_g 10 |d slack_g| / scaling_g.  The difference of the two values adds the
    roundings of f / scaling[0] + pen: 4 x 2^-53 (|v_c| + |v_u|).  A particle whose reference
    scaled slack lies within 1e-9 of a band edge may land in the other band and is left out; at
    most 1 % may be."""
    safeopt_amd = mods[0]
    kind, d, n, m, P = case
    particles = ref.problem(*case)[4]
    gps = device_gps(case)
    fmin = np.array(ref.fmin_of(case))
    opt = safeopt_amd.SafeOptSwarm(gps, list(fmin), bounds=[(-3.0, 3.0)] * d, beta=ref.BETA,
                                   scaling=ref.SCALING, swarm_size=20)
    vu, _ = unconstrained(case)
    vc, safe = opt._compute_path_fitness(device_path(case), particles)
    assert_array_equal(fitness(case, fmin)[0], vc)          # the method is the C call
    _, safe_max = opt._compute_particle_fitness('maximizers', particles)
    assert_array_equal(safe, safe_max)
    assert 0 < safe.sum() < P

    pen = np.zeros(P)
    tol = 4 * 2.0 ** -53 * (np.abs(vc) + np.abs(vu))
    scaled = np.empty((2, P))
    for g, gp in enumerate(gps):
        mean, var = gp.predict_noiseless(particles)
        mean, var = mean[:, 0], var[:, 0]
        sd = np.sqrt(var)
        scaled[g] = (mean - ref.BETA * sd - fmin[g]) / ref.SCALING[g]
        pen += opt._compute_penalty(scaled[g])
        kdiag = pn.prior_variance(ref.problem(*case)[g])
        dv = 2 * VAR_TOL * kdiag
        d_slack = 2 * MEAN_TOL * np.abs(mean).max() + ref.BETA * np.minimum(np.sqrt(dv), dv / sd)
        tol += 10 * d_slack / ref.SCALING[g]
    assert scaled.min() > -1.0
    keep = ~ref.near_band_edge(scaled)
    assert np.count_nonzero(~keep) <= 0.01 * P
    err = np.abs((vc - vu) - pen)
    print("penalty: max |(v_c - v_u) - pen| %.3e, max err / tol %.3e, left out %d of %d"
          % (err[keep].max(), (err[keep] / tol[keep]).max(), np.count_nonzero(~keep), P))
    assert np.all(err[keep] <= tol[keep])
    # the penalty is really there
    assert np.abs(pen).max() > 1e-3


# ---- 3. same bits ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[8], ref.CASES[3]], ids=[ref.IDS[8], ref.IDS[3]])
def test_same_bits_for_a_subset_and_a_repeat(mods, case):
    """37 particles against the rows 100..136 of the 5000 that hold them, and a repeated call.
    The path term of a particle depends on its coordinates and the path alone.  (fmin = -inf: the
    fitness IS the path term -- the posterior behind a penalty comes from different kernels at
    37 and at 5000 particles; with constraints the repeat is compared.)"""
    assert case[4] == 37 and case[2] in (5, 300)
    particles = ref.problem(*case)[4]
    big = np.random.RandomState(77 + case[1]).uniform(-3, 3, (5000, case[1]))
    assert_array_equal(big[100:137], particles)
    open_ = np.array([-np.inf, -np.inf])
    few, _ = fitness(case, open_)
    many, _ = fitness(case, open_, particles=big)
    assert_array_equal(few, many[100:137])
    assert_array_equal(fitness(case, open_)[0], few)
    assert_array_equal(fitness(case, open_, particles=big[100:101])[0], few[:1])
    fmin = np.array(ref.fmin_of(case))
    a, b = fitness(case, fmin), fitness(case, fmin)
    assert_array_equal(a[0], b[0])
    assert_array_equal(a[1], b[1])


# ---- 4. device loop == host loop ---------------------------------------------------------------

@pytest.mark.parametrize("swarm_size", [40, 100])
def test_device_loop_bit_identical_to_host_loop(mods, swarm_size):
    """``sgp_swarm_run_path`` against the reference loop over ``_compute_path_fitness``, same
    np.random stream: every state array bit-identical, the generator left in the same state.
    40 particles lie below kSmallSwarm: a path run takes the general launches there too."""
    from functools import partial
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization
    opt = _swarm_problem(mods, "device", swarm_size=swarm_size)
    np.random.seed(21)
    pp = opt.gp.posterior_paths(size=2, features=96)
    path = (pp.Omega, pp.phase, np.ascontiguousarray(pp.W[:, 1]), np.ascontiguousarray(pp.V[:, 1]))
    start = np.random.default_rng(3).uniform(-0.5, 0.5, size=(swarm_size, 2))
    host = SwarmOptimization(swarm_size, opt.optimal_velocities,
                             partial(opt._compute_path_fitness, path), bounds=opt.bounds)
    dev = DeviceSwarmOptimization(swarm_size, opt.optimal_velocities, opt, 'thompson',
                                  bounds=opt.bounds, rng='numpy')
    dev.set_path(path)
    out = []
    for sw in (host, dev):
        np.random.seed(11)
        sw.init_swarm(start.copy())
        sw.run_swarm(5)
        out.append((sw.positions.copy(), sw.velocities.copy(), sw.best_positions.copy(),
                    np.array(sw.best_values), np.array(sw.global_best), np.random.rand()))
    for a, b in zip(out[0], out[1]):
        assert_array_equal(a, b)
    assert len(np.unique(out[1][0])) > swarm_size          # the swarm really moved
    assert_array_equal(dev.fitness(start)[0], host.fitness(start)[0])


# ---- 5. end to end -----------------------------------------------------------------------------

@pytest.mark.parametrize("pso", ["device", "device-rng"])
def test_thompson_points_end_to_end(mods, pso):
    np.random.seed(2)
    opt = _swarm_problem(mods, pso)
    before = (opt.S.copy(), opt.greedy_point.copy(), opt.best_lower_bound, opt.t)
    np.random.seed(5)
    x, values, pp = opt.thompson_points(size=4, features=256, return_paths=True)
    d = opt.gp.input_dim
    assert x.shape == (4, d) and values.shape == (4,) and pp.size == 4 and pp.features == 256
    bounds = np.asarray(opt.bounds)
    assert np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
    assert opt._compute_particle_fitness('safe_set', x)[1].all()
    f = pp.paths(x)
    assert_array_equal(values, np.array([f[s, 0, s] for s in range(4)]))
    assert len(np.unique(x, axis=0)) > 1
    # the same seed, the same picks; without return_paths two results
    np.random.seed(5)
    x2, values2 = opt.thompson_points(size=4, features=256)
    assert_array_equal(x2, x)
    assert_array_equal(values2, values)
    # no state of the optimiser changed
    assert_array_equal(opt.S, before[0])
    assert_array_equal(opt.greedy_point, before[1])
    assert opt.best_lower_bound == before[2] and opt.t == before[3]
    assert sorted(opt.swarms) == ['expanders', 'greedy', 'maximizers']
    # ... and optimize() goes on as if the call had not been made
    np.random.seed(9)
    after = opt.optimize()
    np.random.seed(2)
    fresh = _swarm_problem(mods, pso)
    np.random.seed(9)
    assert_array_equal(fresh.optimize(), after)
    assert_array_equal(fresh.S, opt.S)


def test_thompson_points_host_loop_matches_device(mods):
    """pso='host' (the reference loop, one fitness call per iteration) picks what pso='device'
    picks under the same seed."""
    res = []
    for pso in ("host", "device"):
        opt = _swarm_problem(mods, pso, swarm_size=20)
        np.random.seed(8)
        res.append(opt.thompson_points(size=2, features=64, max_iters=6))
    assert_array_equal(res[0][0], res[1][0])
    assert_array_equal(res[0][1], res[1][1])


# ---- 6. errors ---------------------------------------------------------------------------------

def test_errors(mods):
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd import _hip
    opt = _swarm_problem(mods, "device")
    with pytest.raises(ValueError, match="SGP_MAX_PATHS"):
        opt.thompson_points(size=_hip.MAX_PATHS + 1)
    state = np.random.get_state()[1].copy()
    opt._comm = _PretendWorld(None, 2)
    with pytest.raises(NotImplementedError, match="sharded Thompson swarm"):
        opt.thompson_points(size=2)
    assert_array_equal(np.random.get_state()[1], state)     # refused before any draw
    # a safe set that is not safe (tests/test_gpu_swarm.py::test_swarm_empty_safe_set_raises)
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[-1.]]), noise_var=0.01 ** 2)
    empty = safeopt_amd.SafeOptSwarm(gp, fmin=[0.], bounds=[[-1., 1.]])
    with pytest.raises(RuntimeError, match="The safe set is empty."):
        empty.thompson_points(size=2, features=16)


def test_c_entry_points_refuse_and_return(mods):
    """P = 0 returns 0 and writes nothing; an unfitted GP fails as ``paths_eval`` does; the
    typed entry point still has no type 4."""
    import ctypes as C
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case = ref.CASES[8]
    devs = [g._fitted() for g in device_gps(case)]
    ctx = devs[0].ctx
    Om, b, w, v = device_path(case)
    d, m = case[1], case[3]
    dp, lib = _hip.dptr, _hip.lib()
    fmin, scaling = np.array(ref.fmin_of(case)), ref.SCALING.copy()
    x = np.zeros((1, d))
    values, safe = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8)
    rc = lib.sgp_swarm_fitness_path(ctx.h, _hip._gp_array(devs), 2, dp(x), 0, 2.0, dp(fmin),
                                    dp(scaling), dp(Om), dp(b), m, dp(w), dp(v), dp(values),
                                    safe.ctypes.data_as(_hip.c_u8_p))
    assert rc == 0 and np.all(values == 7.0) and np.all(safe == 9)
    state = [np.full((1, d), 3.0), np.full((1, d), 4.0), np.full((1, d), 5.0), np.full(1, 6.0),
             np.full(d, 8.0)]
    vs = np.full(d, 0.1)
    rc = lib.sgp_swarm_run_path(ctx.h, _hip._gp_array(devs), 2, 2.0, dp(fmin), dp(scaling), 0,
                                dp(state[0]), dp(state[1]), dp(state[2]), dp(state[3]),
                                dp(state[4]), dp(vs), None, 1, 3, 1.0, -0.3, None, 5, dp(Om),
                                dp(b), m, dp(w), dp(v))
    assert rc == 0
    for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)):
        assert np.all(a == val)
    # more features than SGP_MAX_FEATURES: the limit of sgp_gp_paths_eval
    with pytest.raises(_hip.HipError, match="SGP_MAX_FEATURES"):
        ctx.check(lib.sgp_swarm_fitness_path(
            ctx.h, _hip._gp_array(devs), 2, dp(x), 1, 2.0, dp(fmin), dp(scaling), dp(Om), dp(b),
            _hip.MAX_FEATURES + 1, dp(w), dp(v), dp(values), safe.ctypes.data_as(_hip.c_u8_p)))
    # sgp_swarm_fitness knows the types 0..3 only
    with pytest.raises(_hip.HipError, match="Invalid swarm type"):
        ctx.check(lib.sgp_swarm_fitness(
            ctx.h, _hip._gp_array(devs), 2, 4, dp(x), 1, 2.0, dp(fmin), dp(scaling), 0.0,
            dp(values), safe.ctypes.data_as(_hip.c_u8_p)))
    assert "thompson" not in _hip.SWARM_TYPES


def test_unfitted_gp_raises_as_paths_eval_does(mods):
    """An infeasible theta in ``lml`` leaves the factor missing
    (tests/test_gpu_paths.py::test_unfitted_gp_raises_as_the_exact_draw_does)."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    rng = np.random.RandomState(11)
    X = rng.uniform(-2, 2, (20, 2))
    X = np.vstack([X, X])                       # duplicated inputs
    Y = np.sin(X).sum(1)[:, None]
    Y[20:] += 0.01
    k = gpy.kern.RBF(2, 1.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=ref.NOISE)
    pp = gp.posterior_paths(size=1, features=5)
    path = (pp.Omega, pp.phase, np.ascontiguousarray(pp.W[:, 0]), np.ascontiguousarray(pp.V[:, 0]))
    Xs = rng.uniform(-2, 2, (7, 2))
    dev = gp._fitted()
    desc = k._desc(2)
    assert gp._evaluate(desc[2], desc[3], -1.9e-8)[4] != 0
    with pytest.raises(_hip.HipError, match="not fitted") as exact:
        dev.paths_eval(pp.Omega, pp.phase, pp.W, pp.V, Xs)
    args = (dev.ctx, [dev], Xs, 2.0, np.array([0.0]), np.array([1.0]), path)
    with pytest.raises(_hip.HipError, match="not fitted") as err:
        _hip.swarm_fitness_path(*args)
    assert str(err.value) == str(exact.value)
    st = [Xs.copy(), np.zeros((7, 2)), np.zeros((7, 2)), np.zeros(7), np.zeros(2)]
    with pytest.raises(_hip.HipError, match="not fitted") as err:
        _hip.swarm_run_path(dev.ctx, [dev], 2.0, np.array([0.0]), np.array([1.0]), *st,
                            np.array([0.1, 0.1]), None, True, 0, 1.0, 0.0, None, path)
    assert str(err.value) == str(exact.value)
