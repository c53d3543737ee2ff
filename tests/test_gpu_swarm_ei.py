"""Expected-improvement swarms (``sgp_swarm_fitness_ei`` / ``sgp_swarm_run_ei``, k_swarm_ei in
csrc/ei.hip, ``SafeOptSwarm.ei_point``) against tests/_swarm_ei_ref.py and ``sgp_ei_eval`` (needs
an MI355X).  Cases, shapes and incumbents: that module's docstring.

Tolerances.  alpha: none -- ``values`` must have the BITS of ``sgp_ei_eval`` on the posterior
the call returns (tests/test_gpu_ei.py holds ``sgp_ei_eval`` to the 50-digit reference).  That
posterior: the criterion of ``_gpu_common.check_posterior`` against the NumPy posterior,
``MEAN_TOL max|mean|`` and ``VAR_TOL k(x, x)`` per GP.  Penalty: see ``test_penalty_and_safety``.
The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import functools
import itertools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
import _swarm_ei_ref as ref
from _gpu_common import mods, _swarm_problem, MEAN_TOL, VAR_TOL  # noqa: F401

pytestmark = pytest.mark.gpu

_GPS = {}
OPEN = np.array([-np.inf, -np.inf])
COMBOS = list(itertools.product(ref.INCUMBENTS, ref.KINDS, (0, 1)))    # incumbent, kind, weigh


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


def code(kind):
    from safeopt_amd import _hip
    return _hip.EI_EI if kind == 'ei' else _hip.EI_PI


def fitness(case, fmin, which, kind, weigh, free, G=2, particles=None, xi=ref.XI,
            alpha=True, post=True):
    """``(values, safe[, alpha][, post])`` of the C call under the incumbent ``which`` of a
    case."""
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)[:G]]
    if particles is None:
        particles = ref.problem(*case)[4]
    return _hip.swarm_fitness_ei(devs[0].ctx, devs, particles, ref.BETA, np.asarray(fmin)[:G],
                                 ref.SCALING[:G], kind, ref.incumbent(case, which), xi, weigh,
                                 free, want_alpha=alpha, want_post=post)


@functools.lru_cache(maxsize=None)
def unconstrained(case, which, kind, G=2):
    """fmin = -inf, safe mode, no weights: alpha alone.  Computed once, read-only."""
    out = fitness(case, OPEN, which, kind, 0, 0, G=G)
    for a in out:
        a.setflags(write=False)
    return out


def eval_alpha(case, post, which, kind, fmin=None, xi=ref.XI):
    """``ctx.ei_eval`` on the posterior ``post`` (G, 2, P) a fitness call returned."""
    ctx = device_gps(case)[0]._fitted().ctx
    return ctx.ei_eval(np.ascontiguousarray(post[:, 0]), np.ascontiguousarray(post[:, 1]),
                       ref.incumbent(case, which), xi, code(kind), fmin)


# ---- 1. alpha is eval's alpha ------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_alpha_is_eval_alpha(mods, case, G):
    """Every incumbent, kind and ``weigh``.  fmin = -inf (no penalty, and ``weigh`` adds
    nothing: no fmin is finite) and, separately, ``free = 1`` with the case's finite fmin (the
    weights are there with ``weigh = 1``): ``values`` is alpha -- bit for bit what
    ``sgp_ei_eval`` gives on the posterior ``post`` the call returns --, the ``alpha`` output is
    ``values``, every particle is safe, every value finite, and that posterior is the posterior
    (few-points path up to 4096 particles, the sweep of the GPs' family above)."""
    kind_, d, n, m, P = case
    fmin = np.array(ref.fmin_of(case))[:G]
    mean_ref, var_ref = ref.posterior_all(case)
    for which, kind, weigh in COMBOS:
        for free, f in ((0, OPEN[:G]), (1, fmin)):
            values, safe, alpha, post = (
                unconstrained(case, which, kind, G) if (free, weigh) == (0, 0)
                else fitness(case, f, which, kind, weigh, free, G=G))
            assert values.shape == (P,) and safe.shape == (P,) and safe.dtype == np.bool_
            assert alpha.shape == (P,) and post.shape == (G, 2, P)
            assert safe.all()
            weights = fmin if (free and weigh) else None
            assert_array_equal(values, eval_alpha(case, post, which, kind, weights))
            assert_array_equal(alpha, values)
            assert np.all(np.isfinite(values))
            if free and weigh:                   # ln Phi <= 0, below 0 somewhere unless P = 1
                plain = eval_alpha(case, post, which, kind)
                assert np.all(values <= plain) and (P == 1 or np.any(values < plain))
            for g in range(G):
                kdiag = pn.prior_variance(ref.problem(*case)[g])
                em = np.max(np.abs(post[g, 0] - mean_ref[g])) / max(np.max(np.abs(mean_ref[g])),
                                                                   1e-300)
                ev = np.max(np.abs(post[g, 1] - var_ref[g])) / kdiag
                assert em < MEAN_TOL, (which, kind, weigh, free, g, em)
                assert ev < VAR_TOL, (which, kind, weigh, free, g, ev)
    a_ref = ref.alpha(case, 'median', 'ei', G=G)
    ea = np.max(np.abs(unconstrained(case, 'median', 'ei', G)[0] - a_ref))
    print("post: |d mean| / max|mean| %.3e (allowed %.0e), |d var| / k(x,x) %.3e (allowed %.0e);"
          " max |alpha - alpha(reference posterior)| at the median incumbent %.3e (not asserted:"
          " z amplifies the posterior's error by 1 / sigma)" % (em, MEAN_TOL, ev, VAR_TOL, ea))


# ---- 2. penalty and safety ---------------------------------------------------------------------

@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_penalty_and_safety(mods, case, G):
    """Finite fmin, safe mode: the safety flags are those of the maximizers swarm (same
    posterior, same rule), and v_c - v_u -- v_u the free call with the same fmin and weights,
    i.e. the same alpha bits -- is the penalty of the slacks that ``predict_noiseless`` gives on
    the same device GPs; ``_compute_ei_fitness`` returns exactly the C call's arrays.

    Tolerance: the derivation of ``test_penalty_and_safety`` in tests/test_gpu_swarm_mes.py,
    restated -- the two posteriors (the fitness call's and predict_noiseless's, each within
    MEAN_TOL max|mean| and VAR_TOL k(x, x) of the truth: twice that between them), |d slack_g|
    <= 2 MEAN_TOL max|mean| + beta min(sqrt(dv), dv / sd) with dv = 2 VAR_TOL k(x, x), the slope
    of the penalty at most 10 above a scaled slack of -1, and the roundings of alpha + pen:
    4 x 2^-53 (|v_c| + |v_u|).  A particle whose reference scaled slack lies within 1e-9 of a
    band edge may land in the other band and is left out; at most 1 % may be.  |alpha| reaches
    ~5e13 under the incumbent max + 1e7, where the rounding term swamps the penalty: the
    penalty identity is asserted under the first two incumbents only; flags, the method and the
    split are asserted under all three."""
    safeopt_amd = mods[0]
    kind_, d, n, m, P = case
    particles = ref.problem(*case)[4]
    gps = device_gps(case)[:G]
    fmin = np.array(ref.fmin_of(case))[:G]
    opt = safeopt_amd.SafeOptSwarm(gps if G > 1 else gps[0], list(fmin),
                                   bounds=[(-3.0, 3.0)] * d, beta=ref.BETA,
                                   scaling=list(ref.SCALING[:G]), swarm_size=20)
    _, safe_max = opt._compute_particle_fitness('maximizers', particles)
    pen = np.zeros(P)
    slack_tol = np.zeros(P)
    scaled = np.empty((G, P))
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
    for which, kind, weigh in COMBOS:
        tau = ref.incumbent(case, which)
        vu = fitness(case, fmin, which, kind, weigh, 1, G=G)[0]
        vc, safe = opt._compute_ei_fitness((kind, tau, ref.XI, bool(weigh), False), particles)
        raw = fitness(case, fmin, which, kind, weigh, 0, G=G, alpha=False, post=False)
        assert len(raw) == 2
        assert_array_equal(raw[0], vc)                       # the method is the C call
        assert_array_equal(raw[1], safe)
        assert_array_equal(safe, safe_max)
        assert 0 < safe.sum() < P
        tol = slack_tol + 4 * 2.0 ** -53 * (np.abs(vc) + np.abs(vu))
        err = np.abs((vc - vu) - pen)
        print("%s %s weigh %d: max |(v_c - v_u) - pen| %.3e, max err / tol %.3e, max |v| %.3e,"
              " left out %d of %d%s"
              % (which, kind, weigh, err[keep].max(), (err[keep] / tol[keep]).max(),
                 np.abs(vc).max(), np.count_nonzero(~keep), P,
                 "" if which in ref.PENALTY_INCUMBENTS else " (not asserted)"))
        if which in ref.PENALTY_INCUMBENTS:
            assert np.all(err[keep] <= tol[keep])


# ---- 3. free mode ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_free_mode_ignores_penalty_and_flags(mods, case):
    """Finite fmin that splits the particles, ``free = 1``, no weights: the values have the
    bits of the unconstrained call, every flag is 1 -- while the safe-mode call on the same
    fmin flags the particles below the constraints."""
    fmin = np.array(ref.fmin_of(case))
    P = case[4]
    for which in ref.INCUMBENTS:
        for kind in ref.KINDS:
            values, safe, alpha, post = fitness(case, fmin, which, kind, 0, 1)
            vu, _, au, pu = unconstrained(case, which, kind)
            assert_array_equal(values, vu)
            assert_array_equal(alpha, au)
            assert_array_equal(post, pu)
            assert safe.dtype == np.bool_ and safe.all()
            if P > 1:
                vs, ss, als, _ = fitness(case, fmin, which, kind, 0, 0)
                assert 0 < ss.sum() < P
                assert_array_equal(als, au)      # alpha is alpha in either mode
                assert np.all(vs <= au)          # the penalty is <= 0 ...
                if which in ref.PENALTY_INCUMBENTS:      # ... and not lost in alpha's rounding
                    assert np.any(vs < au)


# ---- 4. repeat ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[8]], ids=[ref.IDS[2], ref.IDS[8]])
def test_repeat_gives_the_same_bits(mods, case):
    """The same call twice (5000 particles through the sweep, 37 through the few-points path),
    with a margin xi > 0: the same bits for values, safe, alpha and post; without ``alpha``,
    without ``post`` and without either the values and flags are the same."""
    assert case[4] in (37, 5000)
    fmin = np.array(ref.fmin_of(case))
    for kind, weigh, free in (('ei', 1, 0), ('pi', 0, 0), ('ei', 1, 1)):
        a = fitness(case, fmin, 'median', kind, weigh, free, xi=0.25)
        b = fitness(case, fmin, 'median', kind, weigh, free, xi=0.25)
        assert len(a) == 4
        for u, w in zip(a, b):
            assert_array_equal(u, w)
        for want_alpha, want_post in ((False, False), (True, False), (False, True)):
            c = fitness(case, fmin, 'median', kind, weigh, free, xi=0.25, alpha=want_alpha,
                        post=want_post)
            assert len(c) == 2 + want_alpha + want_post
            assert_array_equal(c[0], a[0])
            assert_array_equal(c[1], a[1])
            if want_alpha:
                assert_array_equal(c[2], a[2])
            if want_post:
                assert_array_equal(c[2], a[3])
        # the margin is really there, and alpha is eval's alpha under it
        assert_array_equal(a[2], eval_alpha(case, a[3], 'median', kind, fmin if weigh else None,
                                            xi=0.25))
        assert not np.array_equal(a[2], eval_alpha(case, a[3], 'median', kind,
                                                   fmin if weigh else None))


# ---- 5. a particle's value does not depend on the block it is evaluated in ---------------------

BLOCK_CASES = [(c, i) for c, i in zip(ref.CASES, ref.IDS) if c[4] == 5000]


@pytest.mark.parametrize("case", [c for c, _ in BLOCK_CASES], ids=[i for _, i in BLOCK_CASES])
def test_value_does_not_depend_on_block(mods, case):
    """The 5000 particles as a whole and as three uneven slices (1, 36, the rest): the same
    bits per particle for values, flags, alpha and the posterior -- wherever the slice's
    posterior is formed by the kernels the whole call takes: every slice for n = 5 and n = 60
    (below 128 observations every P takes the sweep of the GPs' family), the slice of 4963 for
    n = 300.  There the slices of 1 and 36 particles take the few-points posterior (n >= 128, P
    <= 4096), another kernel: their posterior is held to twice the posterior tolerance against
    the whole call's, and their alpha to the bits of ``sgp_ei_eval`` on their own posterior."""
    kind_, d, n, m, P = case
    fmin = np.array(ref.fmin_of(case))
    particles = ref.problem(*case)[4]
    for kind, weigh, free in (('ei', 1, 0), ('pi', 1, 1)):
        whole = fitness(case, fmin, 'median', kind, weigh, free)
        for lo, hi in ((0, 1), (1, 37), (37, P)):
            part = fitness(case, fmin, 'median', kind, weigh, free,
                           particles=np.ascontiguousarray(particles[lo:hi]))
            same_route = n < 128 or hi - lo > 4096
            if same_route:
                for u, w in zip(part[:3], whole[:3]):
                    assert_array_equal(u, w[lo:hi])
                assert_array_equal(part[3], whole[3][:, :, lo:hi])
                continue
            assert_array_equal(part[2], eval_alpha(case, part[3], 'median', kind, fmin))
            for g in range(2):
                kdiag = pn.prior_variance(ref.problem(*case)[g])
                wm, wv = whole[3][g, 0], whole[3][g, 1]
                em = np.max(np.abs(part[3][g, 0] - wm[lo:hi])) / np.max(np.abs(wm))
                ev = np.max(np.abs(part[3][g, 1] - wv[lo:hi])) / kdiag
                print("rows %d..%d GP %d: few-points against sweep |d mean| %.3e, |d var| %.3e"
                      % (lo, hi, g, em, ev))
                assert em < 2 * MEAN_TOL and ev < 2 * VAR_TOL


# ---- 6. device loop == host loop ---------------------------------------------------------------

@pytest.mark.parametrize("free", [False, True], ids=["safe", "free"])
@pytest.mark.parametrize("swarm_size", [40, 100])
def test_device_loop_bit_identical_to_host_loop(mods, swarm_size, free):
    """``sgp_swarm_run_ei`` against the reference loop over ``_compute_ei_fitness``, same
    np.random stream, five iterations: every state array bit-identical, the generator left in
    the same state.  40 particles lie below kSmallSwarm: an 'ei' run takes the general launches
    there too."""
    from functools import partial
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization
    opt = _swarm_problem(mods, "device", swarm_size=swarm_size)
    start = np.random.default_rng(3).uniform(-0.5, 0.5, size=(swarm_size, 2))
    mean = opt.gp.predict_noiseless(start)[0][:, 0]
    ei = ('ei', float(np.median(mean)), 0.125, True, free)
    host = SwarmOptimization(swarm_size, opt.optimal_velocities,
                             partial(opt._compute_ei_fitness, ei), bounds=opt.bounds)
    dev = DeviceSwarmOptimization(swarm_size, opt.optimal_velocities, opt, 'ei',
                                  bounds=opt.bounds, rng='numpy')
    dev.set_incumbent(*ei)
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
    assert np.all(np.isfinite(out[1][3]))
    for u, w in zip(dev.fitness(start), host.fitness(start)):
        assert_array_equal(u, w)
    flags = dev.fitness(start)[1]
    if free:
        assert flags.all()
    else:
        assert_array_equal(flags, opt._compute_particle_fitness('maximizers', start)[1])


# ---- 7. end to end -----------------------------------------------------------------------------

def _standing_state(opt):
    out = []
    for name in ('greedy', 'maximizers', 'expanders'):
        sw = opt.swarms[name]
        out += [np.array(a) for a in (sw.positions, sw.velocities, sw.best_positions,
                                      sw.best_values, sw.global_best)]
        if hasattr(sw, '_calls'):
            out.append(np.array([sw._calls]))
    for gp in opt.gps:
        out += [np.array(gp.X), np.array(gp.Y)]
    return out


def _alpha_at(opt, x, st, feasibility=False):
    post = [gp.predict_noiseless(x[None, :]) for gp in opt.gps]
    mean = np.stack([m.reshape(-1) for m, _ in post])
    var = np.stack([v.reshape(-1) for _, v in post])
    ctx = opt.gp._fitted().ctx
    return float(ctx.ei_eval(mean, var, st['tau'], st['xi'], code(st['kind']),
                             np.asarray(opt.fmin, dtype=float) if feasibility else None)[0])


@pytest.mark.parametrize("pso", ["device", "device-rng", "host"])
def test_ei_point_end_to_end(mods, pso):
    np.random.seed(2)
    opt = _swarm_problem(mods, pso)
    opt.optimize()                                # the standing swarms hold a real state
    opt._recheck_safe_set()                       # (what ei_point may do to S, done up front)
    before = (opt.S.copy(), opt.greedy_point.copy(), opt.best_lower_bound, opt.t)
    swarms = _standing_state(opt)
    ids = {k: id(v) for k, v in opt.swarms.items()}
    d = opt.gp.input_dim
    bounds = np.asarray(opt.bounds)
    P, iters = opt.swarm_size, 7
    np.random.seed(5)
    state = np.random.get_state()
    x, alpha, st = opt.ei_point(max_iters=iters, return_state=True)
    after = np.random.get_state()
    assert x.shape == (d,) and isinstance(alpha, float) and np.isfinite(alpha)
    assert sorted(st) == ['kind', 'safe', 'tau', 'xi']
    assert st['kind'] == 'ei' and st['xi'] == 0.0 and st['safe'] is True
    assert np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
    assert opt._compute_particle_fitness('safe_set', x[None, :])[1].all()
    # the default incumbent: the largest posterior mean over S
    assert st['tau'] == float(np.max(opt.gp.predict_noiseless(opt.S)[0]))
    assert alpha == _alpha_at(opt, x, st)
    # the generator: one swarm's worth, no path
    np.random.set_state(state)
    if pso == 'device-rng':
        np.random.randint(0, 2 ** 31 - 1)         # the key of the swarm's device generator
    np.random.randint(opt.S.shape[0], size=P)
    if pso == 'device':
        np.random.rand(P * d)
        np.random.rand(2 * P * d * iters)
    if pso == 'host':
        np.random.rand(P, d)
        for _ in range(iters):
            np.random.rand(2 * P, d)
    mine = np.random.get_state()
    assert mine[0] == after[0] and mine[2:] == after[2:]
    assert_array_equal(mine[1], after[1])
    # the same seed, the same result; without return_state two results
    np.random.seed(5)
    x2, alpha2 = opt.ei_point(max_iters=iters)
    assert_array_equal(x2, x)
    assert alpha2 == alpha
    # incumbent='data' and a float; log-PI with a margin and the weights
    np.random.seed(6)
    xd, ad, sd = opt.ei_point(incumbent='data', max_iters=iters, return_state=True)
    assert sd['tau'] == float(np.nanmax(opt.y[:, 0])) and ad == _alpha_at(opt, xd, sd)
    assert sd['safe'] is True
    np.random.seed(6)
    xf, af, sf = opt.ei_point(incumbent=sd['tau'], max_iters=iters, return_state=True)
    assert_array_equal(xf, xd)
    assert af == ad and sf['tau'] == sd['tau']
    np.random.seed(6)
    xp, ap, sp = opt.ei_point(incumbent=0.25, xi=0.5, kind='pi', feasibility=True,
                              max_iters=iters, return_state=True)
    assert (sp['tau'], sp['xi'], sp['kind'], sp['safe']) == (0.25, 0.5, 'pi', True)
    assert ap == _alpha_at(opt, xp, sp, feasibility=True) and ap <= 0.0
    # within='bounds': not a safe pick -- in bounds, the flag reported, no safe_set call but
    # the one return_state asks for
    calls = []
    orig = opt._compute_particle_fitness

    def counted(swarm_type, particles):
        calls.append((swarm_type, np.atleast_2d(particles).shape[0]))
        return orig(swarm_type, particles)
    opt._compute_particle_fitness = counted
    try:
        np.random.seed(7)
        xb, ab, sb = opt.ei_point(within='bounds', feasibility=True, max_iters=iters,
                                  return_state=True)
        with_state = list(calls)
        del calls[:]
        np.random.seed(7)
        xb2, ab2 = opt.ei_point(within='bounds', feasibility=True, max_iters=iters)
        without_state = list(calls)
    finally:
        del opt._compute_particle_fitness
    assert np.all(xb >= bounds[:, 0]) and np.all(xb <= bounds[:, 1])
    assert isinstance(sb['safe'], bool)
    assert sb['safe'] == bool(orig('safe_set', xb[None, :])[1][0])
    assert ab == _alpha_at(opt, xb, sb, feasibility=True)
    assert_array_equal(xb2, xb)
    assert ab2 == ab
    rows = opt.S.shape[0]
    assert with_state == [('safe_set', rows), ('safe_set', 1)]     # recheck, the pick's flag
    assert without_state == [('safe_set', rows)]                   # the recheck alone
    # no state of the optimiser changed
    assert_array_equal(opt.S, before[0])
    assert_array_equal(opt.greedy_point, before[1])
    assert opt.best_lower_bound == before[2] and opt.t == before[3]
    assert sorted(opt.swarms) == ['expanders', 'greedy', 'maximizers']
    assert {k: id(v) for k, v in opt.swarms.items()} == ids
    for a, b in zip(swarms, _standing_state(opt)):
        assert_array_equal(a, b)


def test_ei_point_host_loop_matches_device(mods):
    """pso='host' (the reference loop, one fitness call per iteration) picks what pso='device'
    picks under the same seed, bit for bit, in safe and in free mode."""
    for kw in (dict(), dict(within='bounds', kind='pi', feasibility=True)):
        res = []
        for pso in ("host", "device"):
            opt = _swarm_problem(mods, pso, swarm_size=20)
            np.random.seed(8)
            res.append(opt.ei_point(max_iters=6, return_state=True, **kw))
        assert_array_equal(res[0][0], res[1][0])
        assert res[0][1] == res[1][1]
        assert res[0][2] == res[1][2]


# ---- 8. the converged state ------------------------------------------------------------------

def test_converged_state_where_ei_underflows(mods):
    """The property LogEI exists for.  The converged run of tests/_ei_problems.py as a swarm
    problem -- 42 observations, sigma tiny around them, the margin 0.5 hundreds of sigma above
    every mean: EI is exactly 0 at every personal best, from the start positions to the end, so
    a swarm on EI itself would have nothing to climb and its pick would be "the lowest index
    among equals".  alpha = ln EI is finite there and differs from start position to start
    position; the swarm climbs it -- no personal best ends below its start, some end above --
    and the pick is the arg-max of the personal bests (the lowest index among equals: within
    five iterations particles may well have met at one maximiser)."""
    import _ei_problems as prob
    from safeopt_amd.swarm import DeviceSwarmOptimization
    safeopt_amd, gpy, _, _ = mods
    z, meta = prob.converged()
    k = gpy.kern.RBF(1, variance=1.7, lengthscale=[0.6], ARD=True)
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"], k, noise_var=prob.NOISE)
    opt = safeopt_amd.SafeOptSwarm(gp, [prob.FMIN], bounds=[(-1.0, 1.0)], beta=prob.BETA,
                                   threshold=0.1, swarm_size=40)
    iters = 5
    np.random.seed(4)
    x, alpha, st = opt.ei_point(xi=prob.XI, max_iters=iters, return_state=True)
    assert st['safe'] is True and np.isfinite(alpha) and np.exp(alpha) == 0.0
    # the same swarm by hand, from the same seed: the personal bests behind the pick
    np.random.seed(4)
    picks = np.random.randint(opt.S.shape[0], size=opt.swarm_size)
    assert len(np.unique(opt.S[picks, 0])) > 2    # (several different start points)
    sw = DeviceSwarmOptimization(opt.swarm_size, opt.optimal_velocities, opt, 'ei',
                                 bounds=opt.bounds, rng='numpy')
    sw.set_incumbent('ei', st['tau'], prob.XI)
    sw.init_swarm(opt.S[picks, :])
    first = np.array(sw.best_values)              # alpha at the start positions
    sw.run_swarm(iters)
    bests = np.array(sw.best_values)
    _, safe = opt._compute_particle_fitness('safe_set', sw.best_positions)
    assert safe.all()                             # no penalty in the values: they are alpha
    values, _, out = opt._compute_ei_fitness(('ei', st['tau'], prob.XI, False, False),
                                             sw.best_positions, want=('alpha',))
    assert_array_equal(values, out['alpha'])
    assert_array_equal(values, bests)             # a particle's bits: its coordinates alone
    for a in (first, bests):
        assert np.all(np.isfinite(a)) and a.max() < -700.0
        assert np.all(np.exp(a) == 0.0)           # EI itself: 0 at every one of them
    assert len(np.unique(first)) > 2              # ... where alpha tells the points apart
    assert np.all(bests >= first) and np.any(bests > first)      # and can be climbed
    print("alpha at the start %.6g .. %.6g, at the end %.6g .. %.6g (%d different values)"
          % (first.min(), first.max(), bests.min(), bests.max(), len(np.unique(bests))))
    i = int(np.argmax(bests))                     # (argmax: the lowest index among equals)
    assert_array_equal(x, sw.best_positions[i])
    assert alpha == _alpha_at(opt, x, st)
    # EI at the same points is one plateau: its arg-max is index 0 whatever the points are
    assert int(np.argmax(np.exp(first))) == 0 and int(np.argmax(np.exp(bests))) == 0


# ---- 9. refusals -------------------------------------------------------------------------------

def _raw(case):
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)]
    return _hip, devs, devs[0].ctx, _hip.lib(), _hip.dptr


GOOD = dict(kind=0, tau=0.5, xi=0.0, weigh=1, free=0, fmin=None)


def _call_fitness(case, x, P, values, safe, alpha, post, G=2, gps=None, **kw):
    _hip, devs, ctx, lib, dp = _raw(case)
    a = dict(GOOD, **kw)
    fmin = np.array(ref.fmin_of(case) if a['fmin'] is None else a['fmin'], dtype=float)
    scaling = ref.SCALING.copy()
    arr = _hip._gp_array(devs) if gps is None else gps
    return ctx, lib.sgp_swarm_fitness_ei(
        ctx.h, arr, G, dp(x), P, 2.0, dp(fmin), dp(scaling), a['kind'], a['tau'], a['xi'],
        a['weigh'], a['free'], dp(values), safe.ctypes.data_as(_hip.c_u8_p), dp(alpha), dp(post))


def _call_run(case, state, P, shard=None, G=2, gps=None, **kw):
    _hip, devs, ctx, lib, dp = _raw(case)
    a = dict(GOOD, **kw)
    fmin = np.array(ref.fmin_of(case) if a['fmin'] is None else a['fmin'], dtype=float)
    scaling = ref.SCALING.copy()
    vs = np.full(case[1], 0.1)
    arr = _hip._gp_array(devs) if gps is None else gps
    args = (ctx.h, arr, G, 2.0, dp(fmin), dp(scaling), P, dp(state[0]),
            dp(state[1]), dp(state[2]), dp(state[3]), dp(state[4]), dp(vs), None, 1, 3, 1.0,
            -0.3, None, 5, a['kind'], a['tau'], a['xi'], a['weigh'], a['free'])
    if shard is not None:
        return ctx, lib.sgp_swarm_run_ei_shard(*(args + shard))
    return ctx, lib.sgp_swarm_run_ei(*args)


NAN, INF = float("nan"), float("inf")
#: one bad argument each, in the documented order; every LATER argument is bad as well, so the
#: message also shows which check came first
BAD = [
    (dict(G=0, kind=7, tau=NAN, xi=-1.0, weigh=2, free=2, fmin=[NAN, 0.0]), "no GP"),
    (dict(kind=7, tau=NAN, xi=-1.0, weigh=2, free=2, fmin=[NAN, 0.0]), "kind = 7 is not"),
    (dict(kind=-1, tau=INF), "kind = -1 is not"),
    (dict(tau=NAN, xi=-1.0, weigh=2, free=2, fmin=[NAN, 0.0]), "incumbent tau = nan is not finite"),
    (dict(tau=-INF, xi=NAN), "incumbent tau = -inf is not finite"),
    (dict(xi=-1.0, weigh=2, free=2, fmin=[NAN, 0.0]), "xi = -1 is negative or not finite"),
    (dict(xi=INF, weigh=-1), "xi = inf is negative or not finite"),
    (dict(xi=NAN, weigh=-1), "xi = nan is negative or not finite"),
    (dict(weigh=2, free=2, fmin=[NAN, 0.0]), "weigh = 2 is not 0 or 1"),
    (dict(weigh=1, free=-1, fmin=[NAN, 0.0]), "free = -1 is not 0 or 1"),
    (dict(weigh=1, fmin=[0.0, NAN]), r"fmin\[1\] is NaN or \+inf"),
    (dict(weigh=1, fmin=[INF, 0.0]), r"fmin\[0\] is NaN or \+inf"),
]


@pytest.mark.parametrize("bad,msg", BAD, ids=[m.split(" is")[0].replace("\\", "") + "-%d" % i
                                              for i, (_, m) in enumerate(BAD)])
def test_bad_arguments_are_refused_in_order_with_nothing_written(mods, bad, msg):
    from safeopt_amd import _hip
    case = ref.CASES[8]
    d = case[1]
    x = np.zeros((3, d))
    values, safe = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8)
    alpha, post = np.full(3, -4.0), np.full((2, 2, 3), -5.0)

    def outputs_untouched():
        return (np.all(values == 7.0) and np.all(safe == 9) and np.all(alpha == -4.0)
                and np.all(post == -5.0))
    ctx, rc = _call_fitness(case, x, 3, values, safe, alpha, post, **bad)
    assert rc != 0
    with pytest.raises(_hip.HipError, match=msg):
        ctx.check(rc)
    assert outputs_untouched()
    # ... and with P <= 0: the refusals come before the empty return
    ctx, rc = _call_fitness(case, x, 0, values, safe, alpha, post, **bad)
    assert rc != 0 and outputs_untouched()
    state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0), np.full(3, 6.0),
             np.full(d, 8.0)]
    for P, shard in ((3, None), (3, (0, 3)), (0, None), (0, (0, 0))):
        ctx, rc = _call_run(case, state, P, shard=shard, **bad)
        with pytest.raises(_hip.HipError, match=msg):
            ctx.check(rc)
        for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)):
            assert np.all(a == val)


def test_fmin_is_checked_with_weigh_only(mods):
    """Without ``weigh`` an fmin of +inf is no refusal of the 'ei' checks (it is what
    sgp_swarm_fitness makes of it: a constraint no particle meets); a -inf fmin is never one."""
    case = ref.CASES[8]
    particles = ref.problem(*case)[4]
    v, s = fitness(case, np.array([np.inf, -np.inf]), 'median', 'ei', 0, 0, alpha=False,
                   post=False)
    assert not s.any() and v.shape == (case[4],)
    v, s = fitness(case, np.array([-np.inf, -np.inf]), 'median', 'ei', 1, 0, alpha=False,
                   post=False)
    assert s.all()
    assert_array_equal(v, unconstrained(case, 'median', 'ei')[0])
    assert particles.shape[0] == case[4]


def test_empty_calls_return_and_empty_blocks_are_refused(mods):
    """P <= 0 returns 0 and writes nothing; an empty block of a sharded swarm is refused with
    nothing written; the typed entry points still know the types 0 .. 3 only."""
    from safeopt_amd import _hip
    case = ref.CASES[8]
    d = case[1]
    x = np.zeros((1, d))
    values, safe = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8)
    alpha, post = np.full(3, -4.0), np.full((2, 2, 3), -5.0)
    for P in (0, -2):
        ctx, rc = _call_fitness(case, x, P, values, safe, alpha, post)
        assert rc == 0 and np.all(values == 7.0) and np.all(safe == 9)
        assert np.all(alpha == -4.0) and np.all(post == -5.0)
    state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0), np.full(3, 6.0),
             np.full(d, 8.0)]

    def untouched():
        return all(np.all(a == val) for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)))
    ctx, rc = _call_run(case, state, 0)
    assert rc == 0 and untouched()
    ctx, rc = _call_run(case, state, 0, shard=(0, 0))
    assert rc == 0 and untouched()
    # an empty block of a sharded swarm
    ctx, rc = _call_run(case, state, 0, shard=(0, 6))
    with pytest.raises(_hip.HipError, match="bad swarm size"):
        ctx.check(rc)
    assert untouched()
    # a block outside its swarm
    ctx, rc = _call_run(case, state, 3, shard=(4, 6))
    with pytest.raises(_hip.HipError, match="bad block"):
        ctx.check(rc)
    assert untouched()
    # sgp_swarm_fitness knows the types 0..3 only
    devs = _raw(case)[1]
    fmin, scaling = np.array(ref.fmin_of(case)), ref.SCALING.copy()
    with pytest.raises(_hip.HipError, match="Invalid swarm type"):
        ctx.check(_hip.lib().sgp_swarm_fitness(
            ctx.h, _hip._gp_array(devs), 2, 7, _hip.dptr(x), 1, 2.0, _hip.dptr(fmin),
            _hip.dptr(scaling), 0.0, _hip.dptr(values), safe.ctypes.data_as(_hip.c_u8_p)))
    assert "ei" not in _hip.SWARM_TYPES


def test_a_block_without_a_communicator_is_refused(mods):
    """``sgp_swarm_run_ei_shard`` with ``P < P_total`` on a context without a communicator is
    refused with nothing written; ``p0 = 0, P = P_total`` is ``sgp_swarm_run_ei``, bit for bit."""
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
    ei, P = ('ei', 0.5, 0.0, 1, 0), 40
    start = np.random.default_rng(1).uniform(-0.5, 0.5, size=(P, d))

    def state(rows):
        return [start[:rows].copy(), np.full((rows, d), 4.0), np.full((rows, d), 5.0),
                np.full(rows, 6.0), np.full(d, 8.0)]
    st = state(10)
    with pytest.raises(_hip.HipError, match="needs a communicator"):
        _hip.swarm_run_ei(ctx, devs, *fit, *st, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                          *ei, seed=7, shard=(0, P))
    assert_array_equal(st[0], start[:10])
    for a, val in zip(st[1:], (4.0, 5.0, 6.0, 8.0)):
        assert np.all(a == val)
    whole, same = state(P), state(P)
    _hip.swarm_run_ei(ctx, devs, *fit, *whole, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                      *ei, seed=7)
    _hip.swarm_run_ei(ctx, devs, *fit, *same, np.full(d, 0.1), None, True, 2, 1.0, -0.4, None,
                      *ei, seed=7, shard=(0, P))
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
    fmin, scaling = np.array([0.0]), np.array([1.0])
    with pytest.raises(_hip.HipError, match="not fitted"):
        _hip.swarm_fitness_ei(dev.ctx, [dev], Xs, 2.0, fmin, scaling, 'ei', 0.5, 0.0, 1, 0)
    values, safe = np.full(7, 7.0), np.full(7, 9, dtype=np.uint8)
    alpha, post = np.full(7, -4.0), np.full((1, 2, 7), -5.0)
    dp = _hip.dptr
    rc = _hip.lib().sgp_swarm_fitness_ei(
        dev.ctx.h, _hip._gp_array([dev]), 1, dp(Xs), 7, 2.0, dp(fmin), dp(scaling), 0, 0.5, 0.0,
        1, 0, dp(values), safe.ctypes.data_as(_hip.c_u8_p), dp(alpha), dp(post))
    assert rc != 0 and np.all(values == 7.0) and np.all(safe == 9)
    assert np.all(alpha == -4.0) and np.all(post == -5.0)
    st = [Xs.copy(), np.zeros((7, 2)), np.zeros((7, 2)), np.zeros(7), np.zeros(2)]
    with pytest.raises(_hip.HipError, match="not fitted"):
        _hip.swarm_run_ei(dev.ctx, [dev], 2.0, fmin, scaling, *st, np.array([0.1, 0.1]), None,
                          True, 0, 1.0, 0.0, None, 'ei', 0.5, 0.0, 1, 0)
    assert_array_equal(st[0], Xs)
    assert not st[1].any() and not st[2].any() and not st[3].any() and not st[4].any()


def test_ei_point_errors(mods):
    safeopt_amd, gpy, _, _ = mods
    # a safe set that is not safe (tests/test_gpu_swarm.py::test_swarm_empty_safe_set_raises)
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[-1.]]), noise_var=0.01 ** 2)
    empty = safeopt_amd.SafeOptSwarm(gp, fmin=[0.], bounds=[[-1., 1.]])
    for kw in (dict(), dict(incumbent=0.5), dict(within='bounds')):
        with pytest.raises(RuntimeError, match="The safe set is empty."):
            empty.ei_point(**kw)
    # a swarm that ends with no safe personal best: the recheck passes, the one real
    # 'safe_set' call behind the run flags every personal best
    opt = _swarm_problem(mods, "device", swarm_size=20)
    orig = opt._compute_particle_fitness
    calls = []

    def second_call_unsafe(swarm_type, particles):
        values, safe = orig(swarm_type, particles)
        calls.append(swarm_type)
        return (values, np.zeros_like(safe)) if len(calls) == 2 else (values, safe)
    opt._compute_particle_fitness = second_call_unsafe
    np.random.seed(1)
    with pytest.raises(RuntimeError, match="There are no safe points to sample in."):
        opt.ei_point(max_iters=2)
    assert calls == ['safe_set', 'safe_set']
    # ... which within='bounds' never asks
    del calls[:]
    np.random.seed(1)
    x, alpha = opt.ei_point(within='bounds', max_iters=2)
    assert calls == ['safe_set'] and np.isfinite(alpha)
