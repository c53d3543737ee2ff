"""Hallucinated swarms (``sgp_swarm_fitness_hall`` / ``sgp_swarm_run_hall``, k_swarm_down in
csrc/swarm_batch.hip, ``SafeOptSwarm.optimize_batch``) against the NumPy statement of
tests/_swarm_batch_ref.py (needs an MI355X).  Cases, shapes and pending picks: that module's
docstring.  The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it: ``down`` is
never read before it is written.

Tolerances.  Variance: 2 VAR_TOL k(x, x) -- the real variance and the downdate are each held to
``_gpu_common.check_posterior``'s bound.  Whole formula: see ``test_the_whole_formula``.
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
import _swarm_batch_ref as ref
import _swarm_thompson_ref as tref
from _gpu_common import mods, _swarm_problem, _PretendWorld, MEAN_TOL, VAR_TOL  # noqa: F401

pytestmark = pytest.mark.gpu

_GPS = {}
OPEN = np.full(3, -np.inf)


def device_gps(case):
    """The G GPs of a case on the device (objective, constraints); built once."""
    import safeopt_amd.gpy as gpy
    if case not in _GPS:
        kind, d, n, b, P, G = case
        _, X, Y, _ = ref.problem(case)
        kerns = [tref.make_kernel(gpy.kern, kind, d)] + \
            [tref.constraint_kernel(gpy.kern, d) for _ in range(G - 1)]
        _GPS[case] = [gpy.models.GPRegression(X, Y[:, [g]], kerns[g], noise_var=ref.NOISE)
                      for g in range(G)]
    return _GPS[case]


def make_clones(case, pend):
    """Clones of the case's device GPs with ``pend`` appended; the caller destroys them."""
    clones = [g._fitted().clone() for g in device_gps(case)]
    for x in pend:
        for c in clones:
            assert c.append(x, 0.0)
    return clones


def hall(case, swarm_type, fmin, pend, particles=None, want_var=True, blb=None):
    from safeopt_amd import _hip
    G = case[5]
    devs = [g._fitted() for g in device_gps(case)]
    if particles is None:
        particles = ref.problem(case)[3]
    clones = make_clones(case, pend)
    try:
        return _hip.swarm_fitness_hall(
            devs[0].ctx, devs, clones, swarm_type, particles, ref.BETA, fmin[:G], ref.SCALING[:G],
            ref.best_lower_bound_of(case) if blb is None else blb, want_var=want_var)
    finally:
        for c in clones:
            c.destroy()


def plain(case, swarm_type, fmin, particles=None):
    from safeopt_amd import _hip
    G = case[5]
    devs = [g._fitted() for g in device_gps(case)]
    if particles is None:
        particles = ref.problem(case)[3]
    return _hip.swarm_fitness(devs[0].ctx, devs, swarm_type, particles, ref.BETA, fmin[:G],
                              ref.SCALING[:G], ref.best_lower_bound_of(case))


@functools.lru_cache(maxsize=None)
def open_expanders(case):
    """values, safe, var_h of the expanders swarm without constraints; computed once."""
    out = hall(case, "expanders", OPEN, ref.pending(case))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. the variance ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_variance_against_the_refit(mods, case):
    """var_h against the posterior refitted on X plus the pending picks."""
    kind, d, n, b, P, G = case
    kerns = ref.problem(case)[0]
    var_h = open_expanders(case)[2]
    assert var_h.shape == (G, P)
    slow = ref.refit_var_h(case, ref.pending(case))
    for g in range(G):
        kdiag = pn.prior_variance(kerns[g])
        err = float(np.max(np.abs(var_h[g] - slow[g]))) / kdiag
        print("GP %d: max |var_h - refit| / k(x, x) = %.3e (bound %.1e)" % (g, err, 2 * VAR_TOL))
        assert err <= 2 * VAR_TOL
    if G == 3:
        assert_array_equal(var_h[1], var_h[2])      # one factor: one downdate


# ---- 2. the width term, exactly ----------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_width_term_exactly(mods, case):
    """fmin = -inf for every GP, expanders: no penalty, interest = G, so values = G max_g
    sqrt(var_h_g) / scaling_g up to the roundings of a square root, a division and a product."""
    G, P = case[5], case[4]
    values, safe, var_h = open_expanders(case)
    assert values.shape == (P,) and safe.shape == (P,) and safe.dtype == np.bool_
    assert safe.all()
    want = G * np.max(np.sqrt(var_h) / ref.SCALING[:G, None], axis=0)
    err = float(np.max(np.abs(values - want) / want))
    print("width term: max relative difference %.3e" % err)
    assert err <= 4 * 2.0 ** -53


# ---- 3. nothing else moved, exactly ------------------------------------------------------------

@pytest.mark.parametrize("swarm_type", ["maximizers", "expanders"])
@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_a_far_pending_point_changes_no_bit(mods, case, swarm_type):
    """The clones carry only the far pending pick: down == 0, and values and safe are those of
    the plain ``sgp_swarm_fitness`` call bit for bit."""
    fmin = ref.fmin_of(case)
    v, s, var_h = hall(case, swarm_type, fmin, ref.pending(case, far_only=True))
    vp, sp = plain(case, swarm_type, fmin)
    assert_array_equal(v, vp)
    assert_array_equal(s, sp)
    assert np.all(np.isfinite(var_h)) and np.all(var_h > 0)


# ---- 4. the whole formula ----------------------------------------------------------------------

PDF_MAX = 1.0 / (0.2 * np.sqrt(2 * np.pi))             # norm.pdf(0, scale=0.2)
PDF_SLOPE = 1.0 / (0.2 ** 2 * np.sqrt(2 * np.pi * np.e))   # max |d/ds norm.pdf(s, scale=0.2)|


@pytest.mark.parametrize("swarm_type", ["maximizers", "expanders"])
@pytest.mark.parametrize("case", ref.FORMULA_CASES, ids=ref.FORMULA_IDS)
def test_the_whole_formula(mods, case, swarm_type):
    """Near pending picks, finite fmin: values against the restatement (_swarm_batch_ref.
    hall_fitness) evaluated on ``predict_noiseless`` of the same device GPs and on the returned
    var_h; safe equals the plain call's bits.

    Tolerance.  The width term W is formed from the returned var_h itself: roundings only.  The
    posterior behind the penalty and the interest (the fitness call's and predict_noiseless's)
    meets ``check_posterior``'s criterion against the truth, between the two twice that: per GP
    |d mean| <= 2 MEAN_TOL max|mean|, dv = 2 VAR_TOL k(x, x), |d sd| <= min(sqrt(dv), dv / sd),
    so e_g = (2 MEAN_TOL max|mean| + beta min(sqrt(dv), dv / sd)) / scaling_g bounds the error
    of the scaled slack of GP g and of the scaled upper bound of GP 0.  Every scaled slack lies
    above -1 (the CPU test holds the reference to it), where the slope of the penalty is at
    most 10: |d pen| <= 10 sum_g e_g.  Interest: maximizers expit(10 u), expit' <= 1/4: |d I| <=
    2.5 e_0; expanders G prod_g pdf(s_g), pdf = norm.pdf(., scale=0.2) with maximum PDF_MAX =
    1 / (0.2 sqrt(2 pi)) and largest slope PDF_SLOPE = 1 / (0.04 sqrt(2 pi e)): |d I| <= G
    (prod_g (PDF_MAX + PDF_SLOPE e_g) - PDF_MAX^k) over the k GPs with a constraint.  With value
    = (W + pen) I: |d value| <= |I| d_pen + |W + pen| d_I + d_pen d_I, plus the roundings of
    the three operations and of W, 8 x 2^-53 (|W| + |pen|) |I|.  A particle whose reference
    scaled slack lies within EDGE_GAP of a band edge may land in the other band and is left
    out; at most 1 % may be."""
    kind, d, n, b, P, G = case
    kerns, _, _, particles = ref.problem(case)
    gps = device_gps(case)
    fmin = ref.fmin_of(case)
    blb = ref.best_lower_bound_of(case)
    v, safe, var_h = hall(case, swarm_type, fmin, ref.pending(case))
    vp, sp = plain(case, swarm_type, fmin)
    assert_array_equal(safe, sp)
    assert 0 < safe.sum() < P

    mean, var = np.empty((G, P)), np.empty((G, P))
    e = np.empty((G, P))
    for g, gp in enumerate(gps):
        m_, v_ = gp.predict_noiseless(particles)
        mean[g], var[g] = m_[:, 0], v_[:, 0]
        dv = 2 * VAR_TOL * pn.prior_variance(kerns[g])
        sd = np.sqrt(var[g])
        e[g] = (2 * MEAN_TOL * np.abs(mean[g]).max() +
                ref.BETA * np.minimum(np.sqrt(dv), dv / sd)) / ref.SCALING[g]
    want, _, scaled, (W, pen, I) = ref.hall_fitness(swarm_type, mean, var, var_h, fmin,
                                                    ref.SCALING, blb)
    assert scaled.min() > -1.0
    d_pen = 10 * e.sum(axis=0)
    if swarm_type == "maximizers":
        d_I = 2.5 * e[0]
    else:
        d_I = G * (np.prod(PDF_MAX + PDF_SLOPE * e, axis=0) - PDF_MAX ** G)
    tol = np.abs(I) * d_pen + np.abs(W + pen) * d_I + d_pen * d_I + \
        8 * 2.0 ** -53 * (np.abs(W) + np.abs(pen)) * np.abs(I)
    keep = ~ref.near_band_edge(scaled)
    assert np.count_nonzero(~keep) <= 0.01 * P
    err = np.abs(v - want)
    print("%s: max |dev - ref| %.3e, max err / tol %.3e, left out %d of %d, "
          "max |hall - plain| %.3e" % (swarm_type, err[keep].max(), (err[keep] / tol[keep]).max(),
                                       np.count_nonzero(~keep), P, np.abs(v - vp).max()))
    assert np.all(err[keep] <= tol[keep])
    # the downdate is really there
    assert np.abs(v - vp).max() > 1e-3


# ---- 5. same bits ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[8], ref.CASES[3]], ids=[ref.IDS[8], ref.IDS[3]])
def test_same_bits_for_a_subset_and_a_repeat(mods, case):
    """37 particles against the rows 100..136 of the 5000 that hold them, a single particle, and
    a repeated call: var_h bit for bit.  down of a particle depends on its coordinates and the
    clones alone; the real variance under it is the one the plain call forms for that P and n
    (the far pending pick alone returns it: down == 0, var_h == var).  At n = 5 every P takes
    the same posterior kernel and all of it is compared.  At n = 300 the 37 particles take the
    few-points posterior and the 5000 the paired sweep: their real variances differ in the last
    bits (measured: 107 of 111 entries, at most 5.3e-15), so there var_h is compared bit for bit
    on the entries whose real variance has the same bits in both launches, and on the others
    through what was taken off, var - var_h, to the rounding of that difference; the single
    particle and the repeat are compared bit for bit at both n."""
    assert case[4] == 37 and case[2] in (5, 300)
    d, n = case[1], case[2]
    particles = ref.problem(case)[3]
    big = np.random.RandomState(77 + d).uniform(-3, 3, (5000, d))
    assert_array_equal(big[100:137], particles)
    pend = ref.pending(case)
    far = ref.pending(case, far_only=True)
    few = hall(case, "expanders", OPEN, pend)[2]
    many = hall(case, "expanders", OPEN, pend, particles=big)[2][:, 100:137]
    one = hall(case, "expanders", OPEN, pend, particles=big[100:101])[2]
    var_few = hall(case, "expanders", OPEN, far)[2]
    var_many = hall(case, "expanders", OPEN, far, particles=big)[2][:, 100:137]
    same = var_few == var_many
    print("real variance, 37 vs 5000: %d of %d entries with equal bits (max |d| %.3e); var_h: "
          "max |d| %.3e on those, %.3e on the others"
          % (same.sum(), same.size, np.abs(var_few - var_many).max(),
             np.abs(few - many)[same].max() if same.any() else 0.0,
             np.abs(few - many)[~same].max() if (~same).any() else 0.0))
    assert_array_equal(hall(case, "expanders", OPEN, pend)[2], few)              # a repeat
    assert_array_equal(one, few[:, :1])
    if n == 5:
        assert same.all()
    assert_array_equal(few[same], many[same])
    off = ~same & (few > 1e-15) & (many > 1e-15)
    taken_few, taken_many = (var_few - few)[off], (var_many - many)[off]
    assert np.all(np.abs(taken_few - taken_many) <=
                  4 * 2.0 ** -53 * np.maximum(var_few, var_many)[off])


# ---- 6. device loop == host loop ---------------------------------------------------------------

@pytest.mark.parametrize("swarm_type", ["maximizers", "expanders"])
@pytest.mark.parametrize("swarm_size", [40, 100])
def test_device_loop_bit_identical_to_host_loop(mods, swarm_size, swarm_type):
    """``sgp_swarm_run_hall`` against the reference loop over ``_compute_hall_fitness``, same
    np.random stream: every state array bit-identical, the generator left in the same state.
    40 particles lie below kSmallSwarm: a hallucinated run takes the general launches there
    too."""
    from functools import partial
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization
    opt = _swarm_problem(mods, "device", swarm_size=swarm_size)
    opt.best_lower_bound = 0.1
    start = np.random.default_rng(3).uniform(-0.5, 0.5, size=(swarm_size, 2))
    clones = [g._fitted().clone() for g in opt.gps]
    try:
        for x in ([0.1, -0.2], [0.3, 0.25], [0.1, -0.2]):
            for c in clones:
                assert c.append(np.array(x), 0.0)
        host = SwarmOptimization(swarm_size, opt.optimal_velocities,
                                 partial(opt._compute_hall_fitness, swarm_type, clones),
                                 bounds=opt.bounds)
        dev = DeviceSwarmOptimization(swarm_size, opt.optimal_velocities, opt, swarm_type,
                                      bounds=opt.bounds, rng='numpy')
        dev.set_clones(clones)
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
        # ... and it is not the plain swarm's fitness
        assert np.abs(dev.fitness(start)[0] -
                      opt._compute_particle_fitness(swarm_type, start)[0]).max() > 1e-6
    finally:
        for c in clones:
            c.destroy()


# ---- 7. end to end -----------------------------------------------------------------------------

def _oracle_sd(opt, X_pending, x):
    """sd of every GP at x from the NumPy posterior refitted on the data plus X_pending."""
    out = []
    for gp in opt.gps:
        kern = tref.kern_tuple(gp.kern, gp.input_dim)
        Xp = np.vstack([np.asarray(gp.X), X_pending]) if len(X_pending) else np.asarray(gp.X)
        noise = float(gp.noise_var)
        Ky = pn.kernel_matrix(kern, Xp, Xp) + (noise + 1e-8) * np.eye(Xp.shape[0])
        kx = pn.kernel_matrix(kern, x[None, :], Xp)
        var = pn.prior_variance(kern) - kx.dot(np.linalg.solve(Ky, kx.T)).item()
        out.append((max(var, 1e-15), pn.prior_variance(kern)))
    return out


def _state(opt):
    return (opt.S.copy(), opt.greedy_point.copy(), float(opt.best_lower_bound), opt.t,
            [g._fitted().factor() for g in opt.gps],
            {k: (s.positions.copy(), s.best_values.copy()) for k, s in opt.swarms.items()})


@pytest.mark.parametrize("pso", ["device", "device-rng"])
def test_optimize_batch_end_to_end(mods, pso):
    np.random.seed(2)
    opt = _swarm_problem(mods, pso)
    np.random.seed(2)
    twin = _swarm_problem(mods, pso)
    np.random.seed(5)
    X, sd_h = opt.optimize_batch(size=4, max_iters=8, return_state=True)
    np.random.seed(5)
    x_twin = twin.optimize()
    k, d, G = X.shape[0], opt.gp.input_dim, len(opt.gps)
    assert 1 <= k <= 4 and X.shape == (k, d) and sd_h.shape == (k, G)
    assert k == 4                                              # this problem has room for 4
    assert_array_equal(X[0], x_twin)
    bounds = np.asarray(opt.bounds)
    assert np.all(X >= bounds[:, 0]) and np.all(X <= bounds[:, 1])
    assert opt._compute_particle_fitness('safe_set', X)[1].all()
    assert len(np.unique(X, axis=0)) == k
    # the hallucinated standard deviations, teacher-forced: |d var| <= 2 VAR_TOL k(x, x), through
    # the square root min(sqrt(dv), dv / sd)
    for b in range(k):
        real = _oracle_sd(opt, X[:0], X[b])
        for g, (var, kdiag) in enumerate(_oracle_sd(opt, X[:b], X[b])):
            dv = 2 * VAR_TOL * kdiag
            sd = np.sqrt(var)
            tol = min(np.sqrt(dv), dv / sd)
            print("pick %d GP %d: sd_h %.6e oracle %.6e (tol %.1e), real sd %.6e"
                  % (b, g, sd_h[b, g], sd, tol, np.sqrt(real[g][0])))
            assert abs(sd_h[b, g] - sd) <= tol
            assert sd_h[b, g] <= np.sqrt(real[g][0]) + tol
    # the state is that after optimize(), bit for bit
    a, t = _state(opt), _state(twin)
    assert_array_equal(a[0], t[0])
    assert_array_equal(a[1], t[1])
    assert a[2] == t[2] and a[3] == t[3]
    for fa, ft in zip(a[4], t[4]):
        assert_array_equal(fa[0], ft[0])
        assert_array_equal(fa[1], ft[1])
    assert sorted(opt.swarms) == ['expanders', 'greedy', 'maximizers']
    for key in a[5]:
        assert_array_equal(a[5][key][0], t[5][key][0])
        assert_array_equal(a[5][key][1], t[5][key][1])
    # ... and the run goes on as if the batch had not been made
    y = [np.array([[0.3]]), np.array([[0.4]])]
    for o in (opt, twin):
        o.add_new_data_point(X[0], np.hstack(y))
    np.random.seed(9)
    after = opt.optimize()
    np.random.seed(9)
    assert_array_equal(twin.optimize(), after)
    assert_array_equal(twin.S, opt.S)
    # the same seed, the same batch
    np.random.seed(2)
    again = _swarm_problem(mods, pso)
    np.random.seed(5)
    assert_array_equal(again.optimize_batch(size=4, max_iters=8), X)


def test_ucb_batch_runs_the_maximizers_only(mods):
    np.random.seed(2)
    opt = _swarm_problem(mods, "device")
    np.random.seed(2)
    twin = _swarm_problem(mods, "device")
    np.random.seed(5)
    X = opt.optimize_batch(size=3, ucb=True, max_iters=5)
    np.random.seed(5)
    assert_array_equal(X[0], twin.optimize(ucb=True))
    assert X.shape == (3, 2) and len(np.unique(X, axis=0)) == 3
    assert opt._compute_particle_fitness('safe_set', X)[1].all()


def test_host_loop_matches_device(mods):
    """pso='host' (the reference loop, one fitness call per iteration) picks what pso='device'
    picks under the same seed."""
    res = []
    for pso in ("host", "device"):
        np.random.seed(2)
        opt = _swarm_problem(mods, pso, swarm_size=20)
        opt.max_iters = 6
        np.random.seed(8)
        res.append(opt.optimize_batch(size=3, max_iters=6, return_state=True))
    assert_array_equal(res[0][0], res[1][0])
    assert_array_equal(res[0][1], res[1][1])


# ---- 8. refusals -------------------------------------------------------------------------------

def test_refusals(mods):
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd import _hip
    case = ref.CASES[8]
    kind, d, n, b, P, G = case
    devs = [g._fitted() for g in device_gps(case)]
    ctx = devs[0].ctx
    particles = ref.problem(case)[3]
    fmin = ref.fmin_of(case)
    args = (particles, ref.BETA, fmin, ref.SCALING[:G], 0.0)
    pend = ref.pending(case)
    clones = make_clones(case, pend)
    fresh = [g.clone() for g in devs]
    other_ctx = _hip.Context(ctx.device)
    try:
        for st in ("greedy", "safe_set"):
            with pytest.raises(_hip.HipError, match="maximizers or an expanders"):
                _hip.swarm_fitness_hall(ctx, devs, clones, st, *args)
        # no pending pick at all; one more on one clone than on the other
        with pytest.raises(_hip.HipError, match="pending picks"):
            _hip.swarm_fitness_hall(ctx, devs, fresh, "expanders", *args)
        assert fresh[1].append(pend[0], 0.0)
        with pytest.raises(_hip.HipError, match="pending picks"):
            _hip.swarm_fitness_hall(ctx, devs, fresh, "expanders", *args)
        assert clones[1].append(np.full(d, 0.5), 0.0)
        with pytest.raises(_hip.HipError, match="pending picks"):
            _hip.swarm_fitness_hall(ctx, devs, clones, "maximizers", *args)
        # a clone of the other GP: another kernel
        assert fresh[0].append(pend[0], 0.0)
        with pytest.raises(_hip.HipError, match="kernel"):
            _hip.swarm_fitness_hall(ctx, devs, [fresh[1], fresh[0]], "expanders", *args)
        # a clone in another context
        X, Y = ref.problem(case)[1:3]
        k0 = tref.make_kernel(gpy.kern, kind, d)
        foreign = _hip.DeviceGP(other_ctx, k0._desc(d), ref.NOISE)
        foreign.set_data(np.vstack([X, pend[:1]]), np.append(Y[:, 0], 0.0))
        with pytest.raises(_hip.HipError, match="another context"):
            _hip.swarm_fitness_hall(ctx, devs, [foreign, fresh[1]], "expanders", *args)
        # the run entry point makes the same checks
        st = [particles.copy(), np.zeros((P, d)), np.zeros((P, d)), np.zeros(P), np.zeros(d)]
        with pytest.raises(_hip.HipError, match="maximizers or an expanders"):
            _hip.swarm_run_hall(ctx, devs, fresh, "greedy", ref.BETA, fmin, ref.SCALING[:G], 0.0,
                                *st, np.full(d, 0.1), None, True, 0, 1.0, 0.0, None)
        with pytest.raises(_hip.HipError, match="pending picks"):
            _hip.swarm_run_hall(ctx, devs, clones, "expanders", ref.BETA, fmin, ref.SCALING[:G],
                                0.0, *st, np.full(d, 0.1), None, True, 0, 1.0, 0.0, None)
        # P = 0 returns 0 and writes nothing
        dp, lib = _hip.dptr, _hip.lib()
        values, safe, vh = np.full(3, 7.0), np.full(3, 9, dtype=np.uint8), np.full((G, 3), 5.0)
        rc = lib.sgp_swarm_fitness_hall(
            ctx.h, _hip._gp_array(devs), _hip._gp_array(fresh), G, 2, dp(particles), 0, ref.BETA,
            dp(fmin), dp(ref.SCALING[:G].copy()), 0.0, dp(values),
            safe.ctypes.data_as(_hip.c_u8_p), dp(vh))
        assert rc == 0 and np.all(values == 7.0) and np.all(safe == 9) and np.all(vh == 5.0)
        state = [np.full((1, d), 3.0), np.full((1, d), 4.0), np.full((1, d), 5.0),
                 np.full(1, 6.0), np.full(d, 8.0)]
        vs = np.full(d, 0.1)
        rc = lib.sgp_swarm_run_hall(
            ctx.h, _hip._gp_array(devs), _hip._gp_array(fresh), G, 2, ref.BETA, dp(fmin),
            dp(ref.SCALING[:G].copy()), 0.0, 0, dp(state[0]), dp(state[1]), dp(state[2]),
            dp(state[3]), dp(state[4]), dp(vs), None, 1, 3, 1.0, -0.3, None, 5)
        assert rc == 0
        for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)):
            assert np.all(a == val)
    finally:
        for c in clones + fresh:
            c.destroy()

    opt = _swarm_problem(mods, "device")
    with pytest.raises(ValueError, match="SGP_MAX_BATCH"):
        opt.optimize_batch(size=65)
    with pytest.raises(ValueError, match="SGP_MAX_BATCH"):
        opt.optimize_batch(size=0)
    state = np.random.get_state()[1].copy()
    before = opt.S.copy()
    opt._comm = _PretendWorld(None, 2)
    with pytest.raises(NotImplementedError, match="one rank"):
        opt.optimize_batch(size=2)
    assert_array_equal(np.random.get_state()[1], state)     # refused before any draw
    assert_array_equal(opt.S, before)
    # only a maximizers or an expanders swarm takes clones
    from safeopt_amd.swarm import DeviceSwarmOptimization
    sw = DeviceSwarmOptimization(20, opt.optimal_velocities, opt, 'greedy', bounds=opt.bounds)
    with pytest.raises(ValueError, match="takes clones"):
        sw.set_clones([])
