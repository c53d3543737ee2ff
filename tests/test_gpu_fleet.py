"""``SafeOptFleet`` on the device: many small problems stepped in one call
(``sgp_grid_step_small_many``, one workgroup per member) against TWINS built from the same
data and stepped one by one.  The arithmetic and its order are the same -- one copy of the
step's phases serves both kernels -- so every comparison is for equality."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _gpu_common import mods, smooth, product_kernel  # noqa: F401

pytestmark = pytest.mark.gpu


def _maker(mods, d, sides, n, seed, kind="RBF", G=1, fmin=0.0, kernel=None, rows=None, **kw):
    """``make()`` builds a fresh optimiser from the same data every time: ``n`` observations
    ON rows of the ``sides`` grid over [-4, 4]^d, at least 0.3 above ``fmin = 0``, so some
    row is safe."""
    safeopt_amd, gpy, _, _ = mods
    rng = np.random.default_rng(seed)
    grid = safeopt_amd.linearly_spaced_combinations([(-4., 4.)] * d, sides)
    pick = rng.choice(len(grid), size=n, replace=False) if rows is None else rows
    X = grid[np.sort(pick)]
    Ys = [smooth(X, 70 + g) - smooth(X, 70 + g).min() + 0.3 for g in range(G)]
    ls = list(rng.uniform(0.8, 1.4, size=d))

    def make():
        ks = [kernel() if kernel else getattr(gpy.kern, kind)(d, 2.0, ls, ARD=True)
              for _ in range(G)]
        gps = [gpy.models.GPRegression(X, Ys[g], ks[g], noise_var=0.05 ** 2) for g in range(G)]
        return safeopt_amd.SafeOpt(gps if G > 1 else gps[0], grid, fmin, threshold=0.2, **kw)
    return make


def _measure(opt, x):
    return np.array([float(smooth(np.atleast_2d(x), 70 + g)[0, 0]) + 0.3
                     for g in range(len(opt.gps))])


def _same_state(mods, o, t):
    _hip = mods[0]._hip
    for name in "QSMG":
        assert_array_equal(getattr(o, name), getattr(t, name))
    assert_array_equal(o._backend.download(_hip.CAND), t._backend.download(_hip.CAND))
    assert o._ci_fresh == t._ci_fresh and o._stale == t._stale
    assert o._argmax_cache == t._argmax_cache
    # (serials differ between twins: the data versions and "is current" must agree)
    assert [s[1] for s in o._backend._seen] == [s[1] for s in t._backend._seen]
    assert o._backend.posterior_is_current() and t._backend.posterior_is_current()


def _same(a, b):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert_array_equal(np.asarray(a), np.asarray(b))


def _step_both(mods, fleet, twins, contexts=None):
    X = fleet.optimize(contexts=contexts)
    # (the members rode the many-problem launch: a plan exists, and the last sweep of the
    # context -- the continuation of a member runs none -- is the one-launch step)
    assert fleet._plan is not None and len(fleet._plan_key) == len(twins)
    assert fleet.opts[0]._backend.ctx.last_sweep() == "step-small"
    for b, (o, t) in enumerate(zip(fleet.opts, twins)):
        xt = t.optimize(context=None if contexts is None else contexts[b])
        assert_array_equal(X[b], xt)
        _same_state(mods, o, t)
    return X


def test_identity_over_a_run(mods):
    """Three members, three kernel instances (1-D / 2-D single-part in the class of 24
    observations, 3-D product kernel in the class of 32): four BO iterations."""
    safeopt_amd, gpy, _, _ = mods
    makers = [
        _maker(mods, 1, [50], 1, 1, fmin=0),
        _maker(mods, 2, [12, 11], 7, 2, kind="Matern52", G=2, fmin=[0.0, -np.inf]),
        _maker(mods, 3, [6, 5, 5], 25, 3,
               kernel=lambda: product_kernel(gpy.kern, 3, [("RBF", [0, 1]), ("Matern32", [2])], 4)),
    ]
    fleet = safeopt_amd.SafeOptFleet([m() for m in makers])
    twins = [m() for m in makers]
    for it in range(4):
        X = _step_both(mods, fleet, twins)
        for o, t, x in zip(fleet.opts, twins, X):
            y = _measure(o, x)
            o.add_new_data_point(x, y)
            t.add_new_data_point(x, y)


def test_boundaries_of_an_observation_class(mods):
    safeopt_amd = mods[0]
    makers = [_maker(mods, 1, [64], n, 10 + n) for n in (24, 25, 32, 33)]
    fleet = safeopt_amd.SafeOptFleet([m() for m in makers])
    twins = [m() for m in makers]
    for it in range(2):
        X = _step_both(mods, fleet, twins)
        for o, t, x in zip(fleet.opts, twins, X):
            y = _measure(o, x)
            o.add_new_data_point(x, y)
            t.add_new_data_point(x, y)


def test_more_members_than_compute_units(mods):
    safeopt_amd = mods[0]
    makers = [_maker(mods, 1, [64], 3, 1000 + b) for b in range(257)]
    fleet = safeopt_amd.SafeOptFleet([m() for m in makers])
    twins = [m() for m in makers]
    _step_both(mods, fleet, twins)


def test_one_member(mods):
    safeopt_amd = mods[0]
    make = _maker(mods, 1, [64], 5, 7)
    fleet, twin = safeopt_amd.SafeOptFleet([make()]), make()
    X = _step_both(mods, fleet, [twin])
    assert len(X) == 1


def _mixed(mods):
    off = _maker(mods, 1, [64], 5, 21)
    many = _maker(mods, 1, [200], 49, 22)
    lip = _maker(mods, 1, [64], 5, 23, lipschitz=1.0)
    unsafe = _maker(mods, 1, [64], 5, 24, fmin=10.0)
    plain = [_maker(mods, 1, [64], 6, 25), _maker(mods, 2, [9, 8], 8, 26)]

    def build():
        opts = [off(), many(), lip(), unsafe(), plain[0](), plain[1]()]
        opts[0].small_step = False
        return opts
    return build


def test_mixed_fleet(mods):
    safeopt_amd = mods[0]
    build = _mixed(mods)
    twins = build()
    want = []
    for t in twins:
        try:
            want.append(t.optimize())
        except EnvironmentError as e:
            want.append(e)
    assert isinstance(want[3], EnvironmentError)
    fleet = safeopt_amd.SafeOptFleet(build())
    X = fleet.optimize(return_exceptions=True)
    for b, (o, t) in enumerate(zip(fleet.opts, twins)):
        if b == 3:
            assert isinstance(X[b], EnvironmentError)
        else:
            assert_array_equal(X[b], want[b])
        for name in "QSMG":
            assert_array_equal(getattr(o, name), getattr(t, name))
    fleet = safeopt_amd.SafeOptFleet(build())
    with pytest.raises(EnvironmentError):
        fleet.optimize()
    for o, t in zip(fleet.opts, twins):
        assert_array_equal(o.Q, t.Q)
        assert_array_equal(o.S, t.S)


def test_converged_member_continues_alone(mods):
    """The benchmark's config 1 (1-D RBF, the 1000-point grid, SafeOpt from x0 = 0 on a
    sampled function): once the safe set stops growing the launch certifies no first
    candidate and the member goes through the individual continuation."""
    safeopt_amd, gpy, _, _ = mods
    state = np.random.get_state()
    np.random.seed(0)
    try:
        bounds = [(-10., 10.)]
        kern = gpy.kern.RBF(1, variance=2.0, lengthscale=1.0)
        grid = safeopt_amd.linearly_spaced_combinations(bounds, 1000)
        fun = safeopt_amd.sample_gp_function(kern, bounds, 0.05 ** 2, 100)
        x0 = np.zeros((1, 1))
        y0 = fun(x0)
        fmin = float(fun(x0, noise=False)[0, 0]) - 1.0

        def make():
            k = gpy.kern.RBF(1, variance=2.0, lengthscale=1.0)
            return safeopt_amd.SafeOpt(gpy.models.GPRegression(x0, y0, k, noise_var=0.05 ** 2),
                                       grid, fmin, threshold=0.2)
        fleet, twin = safeopt_amd.SafeOptFleet([make()]), make()
        member = fleet.opts[0]
        visits = []
        inner = member._visit_candidates
        member._visit_candidates = lambda *a, **k: (visits.append(1), inner(*a, **k))[1]
        for it in range(19):
            X = _step_both(mods, fleet, [twin])
            y = fun(X[0])
            member.add_new_data_point(X[0], y)
            twin.add_new_data_point(X[0], y)
    finally:
        np.random.set_state(state)
    assert visits, "the run never reached a step whose first candidate was not certified"


def test_context_argument(mods):
    """The contextual example's shape: one context column, RBF(parameters) x RBF(context)."""
    safeopt_amd, gpy, _, _ = mods
    ps = safeopt_amd.linearly_spaced_combinations([(-5., 5.)], 300)

    def make(seed):
        x = np.array([[0., 0.], [0.5, 0.1]])
        y = smooth(x, seed) - smooth(np.zeros((1, 2)), seed) + 1.0
        k = (gpy.kern.RBF(1, variance=2., lengthscale=1.0, active_dims=[0])
             * gpy.kern.RBF(1, variance=2., lengthscale=1.0, active_dims=[1]))
        return safeopt_amd.SafeOpt(gpy.models.GPRegression(x, y, k, noise_var=0.05 ** 2), ps, 0.,
                                   threshold=0.5, num_contexts=1)
    fleet = safeopt_amd.SafeOptFleet([make(7), make(8)])
    twins = [make(7), make(8)]
    for cs in ([np.array([[0.1]]), np.array([[-0.2]])], [np.array([[0.0]]), np.array([[0.1]])]):
        X = _step_both(mods, fleet, twins, contexts=cs)
        for o, t, c in zip(fleet.opts, twins, cs):
            assert_array_equal(o.context, t.context)
            assert_array_equal(o.context, c.ravel())
        assert X[0].shape == (1,)


def test_refusals(mods):
    safeopt_amd = mods[0]
    _hip = safeopt_amd._hip
    a, b = _maker(mods, 1, [64], 5, 31)(), _maker(mods, 1, [64], 6, 32)()
    big = _maker(mods, 1, [200], 49, 33)()
    members = [a, b, big]
    for o in members:
        o.optimize()
    ctx = a._backend.ctx

    def attempt(opts, gps=None):
        plan = _hip.FleetPlan(ctx, [o._backend.grid for o in opts])
        for j, o in enumerate(opts):
            plan.set_gps(j, (gps or [p._backend._dev() for p in opts])[j])
            plan.beta[j] = 2.0
            fm, sc, tb = plan.rows[j]
            fm[:], sc[:] = o.fmin, o.scaling
            tb[:] = 0.0 if o._thr_beta is None else o._thr_beta
        before = [o._backend.download(_hip.Q) for o in members]
        with pytest.raises(_hip.HipError) as err:
            ctx.step_small_many(plan)
        for o, q in zip(members, before):
            assert_array_equal(o._backend.download(_hip.Q), q)
        return str(err.value)

    assert "member 1" in attempt([a, a])                                  # one grid twice
    assert "member 1" in attempt([a, b], [a._backend._dev(), a._backend._dev()])   # one GP twice
    attempt([])                                                           # B = 0
    assert "member 1" in attempt([a, big])                                # 49 observations
    # the constructor
    for bad, exc in (([], ValueError), ([a, object()], TypeError), ([a, b, a], ValueError),
                     ([a, safeopt_amd.SafeOpt(a.gps[0], a.parameter_set, 0.0)], ValueError)):
        with pytest.raises(exc):
            safeopt_amd.SafeOptFleet(bad)

    class TwoRanks(object):
        world, rank = 2, 0
    c = _maker(mods, 1, [64], 5, 34)()
    c._comm = TwoRanks()
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, c])
    d = _maker(mods, 1, [64], 5, 35)()
    d._backend.ctx = object()
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, d])
    # ... and the members still step
    X = safeopt_amd.SafeOptFleet([a, b]).optimize()
    assert len(X) == 2


def test_state_is_left_usable(mods):
    safeopt_amd = mods[0]
    makers = [_maker(mods, 1, [64], 5, 41), _maker(mods, 2, [9, 8], 8, 42)]
    fleet = safeopt_amd.SafeOptFleet([m() for m in makers])
    twins = [m() for m in makers]
    _step_both(mods, fleet, twins)
    for o, t in zip(fleet.opts, twins):
        np.random.seed(5)
        got = o.mes_point()
        np.random.seed(5)
        _same(got, t.mes_point())
        _same(o.ei_point(), t.ei_point())


def test_repeat_stability(mods):
    safeopt_amd = mods[0]
    makers = [_maker(mods, 1, [64], 5, 51), _maker(mods, 2, [9, 8], 8, 52),
              _maker(mods, 1, [64], 30, 53)]
    fleet = safeopt_amd.SafeOptFleet([m() for m in makers])
    ctx = fleet.opts[0]._backend.ctx
    first = [np.array(x) for x in fleet.optimize()]
    fleet.optimize()
    allocs = ctx.alloc_count()
    for _ in range(48):
        X = fleet.optimize()
        for x, x0 in zip(X, first):
            assert_array_equal(x, x0)
    assert ctx.alloc_count() == allocs
