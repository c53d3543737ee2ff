"""Max-value entropy search swarms (``sgp_swarm_fitness_mes`` / ``sgp_swarm_run_mes``,
k_swarm_mes in csrc/mes.hip, ``SafeOptSwarm.mes_point``) against tests/_swarm_mes_ref.py and
``sgp_mes_eval`` (needs an MI355X).  Cases, shapes and maxima: that module's docstring.

Tolerances.  alpha: none -- ``values`` must have the BITS of ``sgp_mes_eval`` on the posterior
the call returns (tests/test_gpu_mes.py holds ``sgp_mes_eval`` to the 50-digit reference).  That
posterior: the criterion of ``_gpu_common.check_posterior`` against the NumPy posterior,
``MEAN_TOL max|mean|`` and ``VAR_TOL k(x, x)``.  Penalty: see ``test_penalty_and_safety``.
The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
import _swarm_mes_ref as ref
from _gpu_common import mods, _swarm_problem, MEAN_TOL, VAR_TOL  # noqa: F401

pytestmark = pytest.mark.gpu

_GPS = {}
OPEN = np.array([-np.inf, -np.inf])


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


def fitness(case, fmin, K, floor, G=2, particles=None):
    """``(values, safe, post)`` of the C call on the maxima ``(K, floor)`` of a case."""
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)[:G]]
    if particles is None:
        particles = ref.problem(*case)[4]
    ystar, fl = ref.maxima(case, K, floor)
    return _hip.swarm_fitness_mes(devs[0].ctx, devs, particles, ref.BETA, fmin[:G],
                                  ref.SCALING[:G], ystar, fl, want_post=True)


@functools.lru_cache(maxsize=None)
def unconstrained(case, K, floor):
    out = fitness(case, OPEN, K, floor)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. alpha is eval's alpha ------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("K,floor", ref.MAXIMA, ids=ref.MAXIMA_IDS)
@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_alpha_is_eval_alpha(mods, case, K, floor, G):
    """fmin = -inf: no penalty, every particle safe, ``values`` is alpha -- bit for bit what
    ``sgp_mes_eval`` gives on the posterior ``post`` the call returns, and that posterior is
    the posterior (few-points path up to 4096 particles, the sweep of the GPs' family above)."""
    from safeopt_amd import _hip
    kind, d, n, m, P = case
    ystar, fl = ref.maxima(case, K, floor)
    values, safe, post = (unconstrained(case, K, floor) if G == 2
                          else fitness(case, OPEN[:1], K, floor, G=1))
    assert values.shape == (P,) and safe.shape == (P,) and safe.dtype == np.bool_
    assert post.shape == (2, P)
    assert safe.all()
    ctx = device_gps(case)[0]._fitted().ctx
    assert_array_equal(values, ctx.mes_eval(post[0], post[1], ystar, fl))
    assert np.all(np.isfinite(values)) and np.all(values >= 0.0)
    m_ref, v_ref = ref.posterior0(case)
    kdiag = pn.prior_variance(ref.problem(*case)[0])
    em = np.max(np.abs(post[0] - m_ref)) / max(np.max(np.abs(m_ref)), 1e-300)
    ev = np.max(np.abs(post[1] - v_ref)) / kdiag
    ea = np.max(np.abs(values - ref.alpha(case, K, floor)))
    print("post: |d mean| / max|mean| %.3e (allowed %.0e), |d var| / k(x,x) %.3e (allowed %.0e);"
          " max |alpha - alpha(reference posterior)| %.3e (not asserted: gamma amplifies the"
          " posterior's error by 1 / sigma)" % (em, MEAN_TOL, ev, VAR_TOL, ea))
    assert em < MEAN_TOL
    assert ev < VAR_TOL


# ---- 2. penalty and safety ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_penalty_and_safety(mods, case):
    """Finite fmin for both GPs: the safety flags are those of the maximizers swarm (same
    posterior, same rule), and values_constrained - values_unconstrained is the penalty of the
    slacks that ``predict_noiseless`` gives on the same device GPs, for every maxima set.

    Tolerance: the derivation of ``test_penalty_and_safety`` in tests/test_gpu_swarm_thompson.py
    -- the same two posteriors (the fitness call's and predict_noiseless's, each within MEAN_TOL
    max|mean| and VAR_TOL k(x, x) of the truth: twice that between them), |d slack_g| <= 2
    MEAN_TOL max|mean| + beta min(sqrt(dv), dv / sd) with dv = 2 VAR_TOL k(x, x), the slope of
    the penalty at most 10 above a scaled slack of -1, and the roundings of alpha + pen:
    4 x 2^-53 (|v_c| + |v_u|) (alpha has the same bits in both calls: the same posterior).  A
    particle whose reference scaled slack lies within 1e-9 of a band edge may land in the other
    band and is left out; at most 1 % may be."""
    safeopt_amd = mods[0]
    kind, d, n, m, P = case
    particles = ref.problem(*case)[4]
    gps = device_gps(case)
    fmin = np.array(ref.fmin_of(case))
    opt = safeopt_amd.SafeOptSwarm(gps, list(fmin), bounds=[(-3.0, 3.0)] * d, beta=ref.BETA,
                                   scaling=ref.SCALING, swarm_size=20)
    _, safe_max = opt._compute_particle_fitness('maximizers', particles)
    pen = np.zeros(P)
    slack_tol = np.zeros(P)
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
        slack_tol += 10 * d_slack / ref.SCALING[g]
    assert scaled.min() > -1.0
    keep = ~ref.near_band_edge(scaled)
    assert np.count_nonzero(~keep) <= 0.01 * P
    assert np.abs(pen).max() > 1e-3                          # the penalty is really there
    for K, floor in ref.MAXIMA:
        vu = unconstrained(case, K, floor)[0]
        vc, safe = opt._compute_mes_fitness(ref.maxima(case, K, floor), particles)
        assert_array_equal(fitness(case, fmin, K, floor)[0], vc)     # the method is the C call
        assert_array_equal(safe, safe_max)
        assert 0 < safe.sum() < P
        tol = slack_tol + 4 * 2.0 ** -53 * (np.abs(vc) + np.abs(vu))
        err = np.abs((vc - vu) - pen)
        print("K = %d: max |(v_c - v_u) - pen| %.3e, max err / tol %.3e, left out %d of %d"
              % (K, err[keep].max(), (err[keep] / tol[keep]).max(), np.count_nonzero(~keep), P))
        assert np.all(err[keep] <= tol[keep])


# ---- 3. repeat ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[8]], ids=[ref.IDS[2], ref.IDS[8]])
def test_repeat_gives_the_same_bits(mods, case):
    """The same call twice (5000 particles through the sweep, 37 through the few-points path):
    the same bits for values, safe and post; ``_compute_mes_fitness`` returns exactly what the
    C call returns; without ``post`` the values are the same."""
    safeopt_amd = mods[0]
    from safeopt_amd import _hip
    assert case[4] in (37, 5000)
    fmin = np.array(ref.fmin_of(case))
    K, floor = ref.MAXIMA[1]
    a, b = fitness(case, fmin, K, floor), fitness(case, fmin, K, floor)
    for u, w in zip(a, b):
        assert_array_equal(u, w)
    gps = device_gps(case)
    opt = safeopt_amd.SafeOptSwarm(gps, list(fmin), bounds=[(-3.0, 3.0)] * case[1],
                                   beta=ref.BETA, scaling=ref.SCALING, swarm_size=20)
    mes = ref.maxima(case, K, floor)
    values, safe = opt._compute_mes_fitness(mes, ref.problem(*case)[4])
    assert_array_equal(values, a[0])
    assert_array_equal(safe, a[1])
    devs = [g._fitted() for g in gps]
    plain = _hip.swarm_fitness_mes(devs[0].ctx, devs, ref.problem(*case)[4], ref.BETA, fmin,
                                   ref.SCALING, mes[0], mes[1])
    assert len(plain) == 2
    assert_array_equal(plain[0], a[0])
    # a particle's value depends on its posterior and (ystar, floor) alone: alpha of the
    # constrained call is eval's alpha on its post, the rest is the penalty
    al = devs[0].ctx.mes_eval(a[2][0], a[2][1], mes[0], mes[1])
    vu = unconstrained(case, K, floor)[0]
    assert_array_equal(al, vu)


# ---- 4. device loop == host loop ---------------------------------------------------------------

@pytest.mark.parametrize("swarm_size", [40, 100])
def test_device_loop_bit_identical_to_host_loop(mods, swarm_size):
    """``sgp_swarm_run_mes`` against the reference loop over ``_compute_mes_fitness``, same
    np.random stream: every state array bit-identical, the generator left in the same state.
    40 particles lie below kSmallSwarm: a 'mes' run takes the general launches there too."""
    from functools import partial
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization
    opt = _swarm_problem(mods, "device", swarm_size=swarm_size)
    start = np.random.default_rng(3).uniform(-0.5, 0.5, size=(swarm_size, 2))
    mean = opt.gp.predict_noiseless(start)[0][:, 0]
    ystar = np.linspace(mean.min(), mean.max() + 2.0, 5)
    floor = float(np.median(mean))
    host = SwarmOptimization(swarm_size, opt.optimal_velocities,
                             partial(opt._compute_mes_fitness, (ystar, floor)),
                             bounds=opt.bounds)
    dev = DeviceSwarmOptimization(swarm_size, opt.optimal_velocities, opt, 'mes',
                                  bounds=opt.bounds, rng='numpy')
    dev.set_maxima(ystar, floor)
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
    assert not np.array_equal(out[1][0], start)
    assert_array_equal(dev.fitness(start)[0], host.fitness(start)[0])


# ---- 5. end to end -----------------------------------------------------------------------------

def _standing_state(opt):
    out = []
    for name in ('greedy', 'maximizers', 'expanders'):
        sw = opt.swarms[name]
        out += [np.array(a) for a in (sw.positions, sw.velocities, sw.best_positions,
                                      sw.best_values, sw.global_best)]
        out.append(np.array([sw._calls]))
    return out


@pytest.mark.parametrize("pso", ["device", "device-rng"])
def test_mes_point_end_to_end(mods, pso):
    np.random.seed(2)
    opt = _swarm_problem(mods, pso)
    opt.optimize()                                # the standing swarms hold a real state
    before = (opt.S.copy(), opt.greedy_point.copy(), opt.best_lower_bound, opt.t)
    swarms = _standing_state(opt)
    ids = {k: id(v) for k, v in opt.swarms.items()}
    np.random.seed(5)
    x, alpha, st = opt.mes_point(paths=4, features=256, return_state=True)
    d = opt.gp.input_dim
    assert x.shape == (d,) and isinstance(alpha, float)
    assert sorted(st) == ['floor', 'thompson_x', 'ystar']
    assert st['ystar'].shape == (4,) and st['thompson_x'].shape == (4, d)
    bounds = np.asarray(opt.bounds)
    assert np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
    assert opt._compute_particle_fitness('safe_set', x[None, :])[1].all()
    assert alpha >= 0.0
    assert alpha == opt.gp.max_value_entropy(x[None, :], st['ystar'], st['floor'])[0, 0]
    # the default floor: the largest posterior mean over S and the Thompson picks
    rows = np.vstack((opt.S, st['thompson_x']))
    assert st['floor'] == float(np.max(opt.gp.predict_noiseless(rows)[0]))
    # the same seed, the same result; without return_state two results
    np.random.seed(5)
    x2, alpha2 = opt.mes_point(paths=4, features=256)
    assert_array_equal(x2, x)
    assert alpha2 == alpha
    # no state of the optimiser changed
    assert_array_equal(opt.S, before[0])
    assert_array_equal(opt.greedy_point, before[1])
    assert opt.best_lower_bound == before[2] and opt.t == before[3]
    assert sorted(opt.swarms) == ['expanders', 'greedy', 'maximizers']
    assert {k: id(v) for k, v in opt.swarms.items()} == ids
    for a, b in zip(swarms, _standing_state(opt)):
        assert_array_equal(a, b)
    # with ystar given no path is drawn: the generator is consumed by one swarm's draws
    P, iters = opt.swarm_size, 7
    np.random.seed(13)
    state = np.random.get_state()
    x3, alpha3, st3 = opt.mes_point(ystar=st['ystar'], floor=None, max_iters=iters,
                                    return_state=True)
    after = np.random.get_state()
    assert st3['thompson_x'] is None and st3['floor'] == -np.inf
    assert_array_equal(st3['ystar'], st['ystar'])
    assert alpha3 == opt.gp.max_value_entropy(x3[None, :], st['ystar'], None)[0, 0]
    np.random.set_state(state)
    if pso == 'device-rng':
        np.random.randint(0, 2 ** 31 - 1)         # the key of the swarm's device generator
    np.random.randint(opt.S.shape[0], size=P)
    if pso == 'device':
        np.random.rand(P * d)
        np.random.rand(2 * P * d * iters)
    mine = np.random.get_state()
    assert mine[0] == after[0] and mine[2:] == after[2:]
    assert_array_equal(mine[1], after[1])
    # ... and optimize() goes on as if the calls had not been made
    np.random.seed(9)
    nxt = opt.optimize()
    np.random.seed(2)
    fresh = _swarm_problem(mods, pso)
    fresh.optimize()
    np.random.seed(9)
    assert_array_equal(fresh.optimize(), nxt)
    assert_array_equal(fresh.S, opt.S)


def test_mes_point_host_loop_matches_device(mods):
    """pso='host' (the reference loop, one fitness call per iteration) picks what pso='device'
    picks under the same seed, bit for bit."""
    res = []
    for pso in ("host", "device"):
        opt = _swarm_problem(mods, pso, swarm_size=20)
        np.random.seed(8)
        res.append(opt.mes_point(paths=2, features=64, max_iters=6, return_state=True))
    assert_array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    assert_array_equal(res[0][2]['ystar'], res[1][2]['ystar'])
    assert res[0][2]['floor'] == res[1][2]['floor']


# ---- 6. refusals -------------------------------------------------------------------------------

def _raw(case):
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)]
    return _hip, devs, devs[0].ctx, _hip.lib(), _hip.dptr


def _call_fitness(case, x, P, ystar, K, floor, values, safe, post):
    _hip, devs, ctx, lib, dp = _raw(case)
    fmin, scaling = np.array(ref.fmin_of(case)), ref.SCALING.copy()
    ys = np.ascontiguousarray(ystar, dtype=np.float64)
    return ctx, lib.sgp_swarm_fitness_mes(
        ctx.h, _hip._gp_array(devs), 2, dp(x), P, 2.0, dp(fmin), dp(scaling), dp(ys), K,
        float(floor), dp(values), safe.ctypes.data_as(_hip.c_u8_p), dp(post))


def _call_run(case, state, P, ystar, K, floor, shard=None, entry=None):
    _hip, devs, ctx, lib, dp = _raw(case)
    fmin, scaling = np.array(ref.fmin_of(case)), ref.SCALING.copy()
    ys = np.ascontiguousarray(ystar, dtype=np.float64)
    vs = np.full(case[1], 0.1)
    args = (ctx.h, _hip._gp_array(devs), 2, 2.0, dp(fmin), dp(scaling), P, dp(state[0]),
            dp(state[1]), dp(state[2]), dp(state[3]), dp(state[4]), dp(vs), None, 1, 3, 1.0,
            -0.3, None, 5, dp(ys), K, float(floor))
    if shard is not None:
        return ctx, lib.sgp_swarm_run_mes_shard(*(args + shard))
    return ctx, lib.sgp_swarm_run_mes(*args)


BAD = [([], 0, 0.0, "SGP_MAX_MES"), (list(range(65)), 65, 0.0, "SGP_MAX_MES"),
       ([0.5, float("nan")], 2, 0.0, "not finite"), ([float("inf")], 1, 0.0, "not finite"),
       ([0.5, 1.0], 2, float("nan"), "floor is NaN")]


@pytest.mark.parametrize("ystar,K,floor,msg", BAD, ids=["K=0", "K=65", "nan", "inf", "nan-floor"])
def test_bad_maxima_are_refused_with_nothing_written(mods, ystar, K, floor, msg):
    from safeopt_amd import _hip
    case = ref.CASES[8]
    d = case[1]
    x = np.zeros((3, d))
    values, safe, post = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8), np.full((2, 3), -5.0)
    ys = ystar if len(ystar) else [0.0]           # (a valid pointer behind K = 0)
    ctx, rc = _call_fitness(case, x, 3, ys, K, floor, values, safe, post)
    assert rc != 0
    with pytest.raises(_hip.HipError, match=msg):
        ctx.check(rc)
    assert np.all(values == 7.0) and np.all(safe == 9) and np.all(post == -5.0)
    state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0), np.full(3, 6.0),
             np.full(d, 8.0)]
    for shard in (None, (0, 3)):
        ctx, rc = _call_run(case, state, 3, ys, K, floor, shard=shard)
        with pytest.raises(_hip.HipError, match=msg):
            ctx.check(rc)
        for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)):
            assert np.all(a == val)
    # the Python side refuses the same before the C call
    if K in (0, 65):
        from safeopt_amd.swarm import DeviceSwarmOptimization
        with pytest.raises(ValueError, match="SGP_MAX_MES"):
            DeviceSwarmOptimization(5, np.full(d, 0.1), None, 'mes', seed=1).set_maxima(ystar)


def test_empty_calls_return_and_empty_blocks_are_refused(mods):
    """P <= 0 returns 0 and writes nothing; an empty block of a sharded swarm is refused with
    nothing written; the typed entry points still know the types 0 .. 3 only."""
    from safeopt_amd import _hip
    case = ref.CASES[8]
    d = case[1]
    x = np.zeros((1, d))
    ys = [0.5, 1.5]
    values, safe, post = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8), np.full((2, 3), -5.0)
    for P in (0, -2):
        ctx, rc = _call_fitness(case, x, P, ys, 2, 0.0, values, safe, post)
        assert rc == 0 and np.all(values == 7.0) and np.all(safe == 9) and np.all(post == -5.0)
    state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0), np.full(3, 6.0),
             np.full(d, 8.0)]

    def untouched():
        return all(np.all(a == val) for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)))
    ctx, rc = _call_run(case, state, 0, ys, 2, 0.0)
    assert rc == 0 and untouched()
    ctx, rc = _call_run(case, state, 0, ys, 2, 0.0, shard=(0, 0))
    assert rc == 0 and untouched()
    # ... but bad maxima are refused even then
    ctx, rc = _call_run(case, state, 0, ys, 65, 0.0)
    assert rc != 0 and untouched()
    # (a block of a larger swarm without a communicator: the test below, on a context of its own)
    # an empty block of a sharded swarm
    ctx, rc = _call_run(case, state, 0, ys, 2, 0.0, shard=(0, 6))
    with pytest.raises(_hip.HipError, match="bad swarm size"):
        ctx.check(rc)
    assert untouched()
    # sgp_swarm_fitness knows the types 0..3 only
    devs = _raw(case)[1]
    fmin, scaling = np.array(ref.fmin_of(case)), ref.SCALING.copy()
    with pytest.raises(_hip.HipError, match="Invalid swarm type"):
        ctx.check(_hip.lib().sgp_swarm_fitness(
            ctx.h, _hip._gp_array(devs), 2, 5, _hip.dptr(x), 1, 2.0, _hip.dptr(fmin),
            _hip.dptr(scaling), 0.0, _hip.dptr(values), safe.ctypes.data_as(_hip.c_u8_p)))
    assert "mes" not in _hip.SWARM_TYPES


def test_a_block_without_a_communicator_is_refused(mods):
    """``sgp_swarm_run_mes_shard`` with ``P < P_total`` on a context without a communicator is
    refused with nothing written; ``p0 = 0, P = P_total`` is ``sgp_swarm_run_mes``, bit for bit."""
    from safeopt_amd import _hip
    case = ref.CASES[8]
    d = case[1]
    # a context of its own: the default one may carry a communicator by now
    ctx = _hip.Context(0)
    devs = []
    for g in device_gps(case):
        dv = _hip.DeviceGP(ctx, g.kern._desc(d), ref.NOISE)
        dv.set_data(np.asarray(g.X), np.asarray(g.Y)[:, 0])
        devs.append(dv)
    fit = (ref.BETA, np.array(ref.fmin_of(case)), ref.SCALING.copy())
    ys, P = np.array([0.5, 1.5]), 40
    start = np.random.default_rng(1).uniform(-0.5, 0.5, size=(P, d))

    def state(rows):
        return [start[:rows].copy(), np.full((rows, d), 4.0), np.full((rows, d), 5.0),
                np.full(rows, 6.0), np.full(d, 8.0)]
    st = state(10)
    with pytest.raises(_hip.HipError, match="needs a communicator"):
        _hip.swarm_run_mes(ctx, devs, *fit, *st, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                           ys, 0.25, seed=7, shard=(0, P))
    assert_array_equal(st[0], start[:10])
    for a, val in zip(st[1:], (4.0, 5.0, 6.0, 8.0)):
        assert np.all(a == val)
    whole, same = state(P), state(P)
    _hip.swarm_run_mes(ctx, devs, *fit, *whole, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                       ys, 0.25, seed=7)
    _hip.swarm_run_mes(ctx, devs, *fit, *same, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                       ys, 0.25, seed=7, shard=(0, P))
    for a, b in zip(whole, same):
        assert_array_equal(a, b)
    assert np.isfinite(whole[3]).all() and not np.array_equal(whole[0], start)


def test_unfitted_gp_is_refused_with_nothing_written(mods):
    """An infeasible theta in ``lml`` leaves the factor of GP 0 missing
    (tests/test_gpu_swarm_thompson.py::test_unfitted_gp_raises_as_paths_eval_does)."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    rng = np.random.RandomState(11)
    X = rng.uniform(-2, 2, (20, 2))
    X = np.vstack([X, X])                       # duplicated inputs
    Y = np.sin(X).sum(1)[:, None]
    Y[20:] += 0.01
    k = gpy.kern.RBF(2, 1.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=ref.NOISE)
    Xs = rng.uniform(-2, 2, (7, 2))
    dev = gp._fitted()
    desc = k._desc(2)
    assert gp._evaluate(desc[2], desc[3], -1.9e-8)[4] != 0
    ys = np.array([0.5, 1.5])
    with pytest.raises(_hip.HipError, match="not fitted"):
        _hip.swarm_fitness_mes(dev.ctx, [dev], Xs, 2.0, np.array([0.0]), np.array([1.0]), ys, 0.0)
    values, safe, post = np.full(7, 7.0), np.full(7, 9, dtype=np.uint8), np.full((2, 7), -5.0)
    dp = _hip.dptr
    fmin, scaling = np.array([0.0]), np.array([1.0])
    rc = _hip.lib().sgp_swarm_fitness_mes(
        dev.ctx.h, _hip._gp_array([dev]), 1, dp(Xs), 7, 2.0, dp(fmin), dp(scaling), dp(ys), 2,
        0.0, dp(values), safe.ctypes.data_as(_hip.c_u8_p), dp(post))
    assert rc != 0 and np.all(values == 7.0) and np.all(safe == 9) and np.all(post == -5.0)
    st = [Xs.copy(), np.zeros((7, 2)), np.zeros((7, 2)), np.zeros(7), np.zeros(2)]
    with pytest.raises(_hip.HipError, match="not fitted"):
        _hip.swarm_run_mes(dev.ctx, [dev], 2.0, fmin, scaling, *st, np.array([0.1, 0.1]), None,
                           True, 0, 1.0, 0.0, None, ys, 0.0)
    assert_array_equal(st[0], Xs)
    assert not st[1].any() and not st[2].any() and not st[3].any() and not st[4].any()


def test_mes_point_errors(mods):
    safeopt_amd, gpy, _, _ = mods
    # a safe set that is not safe (tests/test_gpu_swarm.py::test_swarm_empty_safe_set_raises)
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[-1.]]), noise_var=0.01 ** 2)
    empty = safeopt_amd.SafeOptSwarm(gp, fmin=[0.], bounds=[[-1., 1.]])
    with pytest.raises(RuntimeError, match="The safe set is empty."):
        empty.mes_point(paths=2, features=16)
    with pytest.raises(RuntimeError, match="The safe set is empty."):
        empty.mes_point(ystar=[0.5])
