"""Information-theoretic safe exploration swarms (``sgp_swarm_fitness_ise`` /
``sgp_swarm_run_ise``, k_swarm_ise in csrc/swarm_ise.hip, ``SafeOptSwarm.ise_point``) against
tests/_swarm_ise_ref.py and ``sgp_ise_eval`` (needs an MI355X).  Cases and shapes: that module's
docstring.

Tolerances.  pairs, alpha, target: none -- ``pairs`` must have the BITS of the in-order sum of
``sgp_ise_eval`` on the call's own ``post``, ``cov``, ``zmean - fmin`` and ``zvar``
(tests/test_gpu_ise.py holds ``sgp_ise_eval`` to the 80-digit reference), alpha / target are the
host's max / first arg-max of them.  ``cov``: ``VAR_TOL k(x, x)`` against the long-double
covariance, the bound the posterior variance -- the same contraction -- is held to.  ``post``:
``_gpu_common.check_posterior``.  Penalty: see ``test_penalty_and_safety``.
The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import functools
from functools import partial

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _incremental_ref as inc
import _swarm_ise_ref as ref
from _gpu_common import mods, _swarm_problem, check_posterior, MEAN_TOL, VAR_TOL  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = ("alpha", "target", "post", "pairs", "cov")
_GPS = {}


def device_gps(case):
    """The GPs of a case on the device; built once."""
    import safeopt_amd.gpy as gpy
    if case not in _GPS:
        X, Y = ref.problem(case)[:2]
        _GPS[case] = [gpy.models.GPRegression(X, Y[:, [g]], inc.make_kernel(gpy.kern, spec),
                                              noise_var=ref.NOISE)
                      for g, spec in enumerate(ref.specs(case))]
    return _GPS[case]


@functools.lru_cache(maxsize=None)
def target_posterior(case):
    """``(zmean, zvar)`` (G, T) as the Python layer forms them: one ``predict_noiseless`` per GP."""
    targets = ref.problem(case)[3]
    post = [g.predict_noiseless(targets) for g in device_gps(case)]
    zm = np.stack([m[:, 0] for m, _ in post])
    zv = np.stack([v[:, 0] for _, v in post])
    zm.setflags(write=False)
    zv.setflags(write=False)
    return zm, zv


def fitness(case, fmin, want=ALL, particles=None, targets=None, zmean=None, zvar=None):
    """``(values, safe, out)`` of the C call on a case."""
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)]
    G = len(devs)
    if particles is None:
        particles = ref.problem(case)[2]
    if targets is None:
        targets = ref.problem(case)[3]
        zmean, zvar = target_posterior(case)
    return _hip.swarm_fitness_ise(devs[0].ctx, devs, particles, ref.BETA, np.asarray(fmin),
                                  ref.SCALING[:G], targets, zmean, zvar, want=want)


@functools.lru_cache(maxsize=None)
def open_call(case):
    values, safe, out = fitness(case, ref.fmin_open(case))
    for a in (values, safe) + tuple(out.values()):
        a.setflags(write=False)
    return values, safe, out


def noise_s(case):
    return np.full(len(ref.specs(case)), ref.NOISE + 1e-8)


# ---- 1. pairs are eval's terms, alpha / target their row maximum -------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_pairs_alpha_target_and_covariance(mods, case):
    kind, d, n, P, T, variant = case
    G = len(ref.specs(case))
    fmin = ref.fmin_open(case)
    values, safe, out = open_call(case)
    assert values.shape == (P,) and safe.shape == (P,) and safe.dtype == np.bool_
    assert out["alpha"].shape == (P,) and out["target"].shape == (P,)
    assert out["target"].dtype == np.int64
    assert out["post"].shape == (G, 2, P) and out["pairs"].shape == (P, T)
    assert out["cov"].shape == (G, P, T)
    zmean, zvar = target_posterior(case)
    ctx = device_gps(case)[0]._fitted().ctx
    host = ref.host_pairs(ctx.ise_eval, out["post"], out["cov"], zmean, zvar, fmin, noise_s(case))
    assert_array_equal(out["pairs"], host)
    assert_array_equal(out["alpha"], host.max(axis=1))
    assert_array_equal(out["target"], host.argmax(axis=1))
    assert np.all(np.isfinite(out["pairs"])) and np.all(out["pairs"] >= 0.0)
    if variant == "mid":
        # (a literal fmin: unsafe particles carry a penalty; a safe one none -- total_pen is 0)
        assert_array_equal(out["cov"][1], np.zeros((P, T)))
        assert_array_equal(values[safe], out["alpha"][safe])
    else:
        assert safe.all()
        assert_array_equal(values, out["alpha"])
    r = ref.reference(case)
    ec = max(np.max(np.abs(out["cov"][g] - r["cov"][g])) / r["kdiag"][g]
             for g in range(G) if np.isfinite(fmin[g]))
    rp = ref.pairs(case, fmin)
    print("cov: max |d cov| / k(x,x) %.3e (allowed %.0e); max |pairs - reference pairs| %.3e, "
          "targets that differ from the reference's %d of %d (neither asserted: the reference "
          "pairs come from the reference posterior)"
          % (ec, VAR_TOL, np.max(np.abs(out["pairs"] - rp[0])),
             np.count_nonzero(out["target"] != rp[2]), P))
    assert ec < VAR_TOL
    for g in range(G):
        check_posterior(out["post"][g, 0], out["post"][g, 1], r["mean"][g], r["var"][g],
                        r["kdiag"][g])


# ---- 2. independence ---------------------------------------------------------------------------

IND = [ref.CASES[5], ref.CASES[9]]
IND_IDS = [ref.IDS[5], ref.IDS[9]]


@pytest.mark.parametrize("case", IND, ids=IND_IDS)
def test_a_particle_does_not_depend_on_the_swarm(mods, case):
    """The first P' particles alone (63 / 64 / 65: both sides of the tile edge) and a
    permutation of the particles give every particle the bits of the whole call."""
    fmin = ref.fmin_open(case)
    particles = ref.problem(case)[2]
    values, safe, out = open_call(case)
    assert particles.shape[0] == 65
    for Pp in (63, 64, 65):
        v, s, o = fitness(case, fmin, particles=particles[:Pp], targets=ref.problem(case)[3],
                          zmean=target_posterior(case)[0], zvar=target_posterior(case)[1])
        assert_array_equal(v, values[:Pp])
        assert_array_equal(s, safe[:Pp])
        for k in ("alpha", "target", "pairs"):
            assert_array_equal(o[k], out[k][:Pp])
        assert_array_equal(o["cov"], out["cov"][:, :Pp])
        assert_array_equal(o["post"], out["post"][:, :, :Pp])
    perm = np.random.RandomState(5).permutation(65)
    v, s, o = fitness(case, fmin, particles=particles[perm], targets=ref.problem(case)[3],
                      zmean=target_posterior(case)[0], zvar=target_posterior(case)[1])
    assert_array_equal(v, values[perm])
    for k in ("alpha", "target", "pairs"):
        assert_array_equal(o[k], out[k][perm])
    assert_array_equal(o["cov"], out["cov"][:, perm])


@pytest.mark.parametrize("case", IND, ids=IND_IDS)
def test_a_pair_does_not_depend_on_the_target_set(mods, case):
    """A permutation of the targets permutes pairs and cov and maps ``target`` (the maxima are
    unique: tests/test_swarm_ise_cpu.py); a prefix of the targets gives the same cov columns."""
    fmin = ref.fmin_open(case)
    targets = ref.problem(case)[3]
    zmean, zvar = target_posterior(case)
    T = targets.shape[0]
    values, safe, out = open_call(case)
    srt = np.sort(out["pairs"], axis=1)
    assert T == 1 or np.all(srt[:, -1] > srt[:, -2])         # no ties at the maximum
    perm = np.random.RandomState(6).permutation(T)
    v, s, o = fitness(case, fmin, targets=targets[perm], zmean=zmean[:, perm],
                      zvar=zvar[:, perm])
    assert_array_equal(o["pairs"], out["pairs"][:, perm])
    assert_array_equal(o["cov"], out["cov"][:, :, perm])
    assert_array_equal(o["alpha"], out["alpha"])
    assert_array_equal(perm[o["target"]], out["target"])
    assert_array_equal(v, values)
    for Tp in (1, 16, 17, 64):
        o = fitness(case, fmin, want=("cov", "pairs"), targets=targets[:Tp],
                    zmean=zmean[:, :Tp], zvar=zvar[:, :Tp])[2]
        assert_array_equal(o["cov"], out["cov"][:, :, :Tp])
        assert_array_equal(o["pairs"], out["pairs"][:, :Tp])


@pytest.mark.parametrize("T", [17, 65])
def test_padding_columns_never_win(mods, T):
    """Exclusion by index, where only it can hold.  Every real pair but the last column's is 0
    (``zmean - fmin`` so large that ``e^-t = 0``); the last column keeps its own posterior.  A
    padding column repeats the last column's target, ``zmean`` and ``zvar`` but meets a zero
    column of W: its covariance would be the PRIOR covariance k(x, z), and its pair -- formed
    here on the host from the call's own outputs -- is larger than the real one at some particles (asserted).  So a
    padding column that took part would win there; it must not: alpha is the last real column's pair, the target is T - 1, or 0 where
    that pair is 0 too."""
    case = ref.CASES[9]
    fmin = ref.fmin_open(case)
    targets = ref.problem(case)[3][:T]
    particles = ref.problem(case)[2]
    gps = device_gps(case)
    G = len(gps)
    zmean = np.full((G, T), 1e6)
    zmean[:, T - 1] = target_posterior(case)[0][:, T - 1]
    zvar = np.array(target_posterior(case)[1][:, :T])
    values, safe, out = fitness(case, fmin, targets=targets, zmean=zmean, zvar=zvar)
    real = out["pairs"][:, T - 1]
    assert_array_equal(out["pairs"][:, :T - 1], np.zeros((particles.shape[0], T - 1)))
    assert_array_equal(out["alpha"], real)
    assert_array_equal(out["target"], np.where(real > 0.0, T - 1, 0))
    # what a padding column would hold: the same term on the prior covariance
    ctx = gps[0]._fitted().ctx
    s = noise_s(case)
    padded = np.zeros_like(real)
    for g in range(G):
        if np.isfinite(fmin[g]):
            prior = np.asarray(gps[g].kern.K(particles, targets[T - 1:T]))[:, 0]
            P = particles.shape[0]
            padded = padded + ctx.ise_eval(np.full(P, zmean[g, T - 1] - fmin[g]),
                                           np.full(P, zvar[g, T - 1]), out["post"][g, 1], prior,
                                           s[g])
    beaten = np.count_nonzero(padded > real)
    print("T = %d: a padding column would beat the real maximum at %d of %d particles"
          % (T, beaten, real.size))
    assert beaten >= 1


# ---- 3. penalty and safety ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.PENALTY_CASES, ids=ref.PENALTY_IDS)
def test_penalty_and_safety(mods, case):
    """Finite fmin that splits the particles: the safety flags are those of the maximizers swarm
    (same posterior, same rule), and ``values - alpha`` -- alpha the call's own -- is the
    penalty of the slacks that ``predict_noiseless`` gives on the same device GPs.

    Tolerance: the derivation of ``test_penalty_and_safety`` in tests/test_gpu_swarm_mes.py --
    the two posteriors (the fitness call's and predict_noiseless's) lie within twice MEAN_TOL
    max|mean| and VAR_TOL k(x, x) of each other, |d slack_g| <= 2 MEAN_TOL max|mean| + beta
    min(sqrt(dv), dv / sd) with dv = 2 VAR_TOL k(x, x), the slope of the penalty at most 10 above
    a scaled slack of -1, and the roundings of alpha + pen: 4 x 2^-53 (|values| + |alpha|).  A
    particle whose scaled slack lies within 1e-9 of a band edge may land in the other band and
    is left out; at most 1 % may be."""
    safeopt_amd = mods[0]
    kind, d, n, P, T, variant = case
    particles = ref.problem(case)[2]
    gps = device_gps(case)
    G = len(gps)
    fmin = ref.fmin_split(case)
    opt = safeopt_amd.SafeOptSwarm(gps, list(fmin), bounds=[(-3.0, 3.0)] * d, beta=ref.BETA,
                                   scaling=ref.SCALING[:G], swarm_size=20)
    _, safe_max = opt._compute_particle_fitness('maximizers', particles)
    pen, slack_tol, scaled = np.zeros(P), np.zeros(P), np.empty((G, P))
    r = ref.reference(case)
    for g, gp in enumerate(gps):
        mean, var = gp.predict_noiseless(particles)
        mean, var = mean[:, 0], var[:, 0]
        sd = np.sqrt(var)
        scaled[g] = (mean - ref.BETA * sd - fmin[g]) / ref.SCALING[g]
        pen += opt._compute_penalty(scaled[g])
        dv = 2 * VAR_TOL * r["kdiag"][g]
        d_slack = 2 * MEAN_TOL * np.abs(mean).max() + ref.BETA * np.minimum(np.sqrt(dv), dv / sd)
        slack_tol += 10 * d_slack / ref.SCALING[g]
    assert scaled.min() > -1.0
    keep = ~ref.near_band_edge(scaled)
    assert np.count_nonzero(~keep) <= 0.01 * P
    assert np.abs(pen).max() > 1e-3                          # the penalty is really there
    ise = (ref.problem(case)[3],) + target_posterior(case)
    vc, safe, out = opt._compute_ise_fitness(ise, particles, want=("alpha",))
    assert_array_equal(fitness(case, fmin, want=())[0], vc)          # the method is the C call
    assert_array_equal(safe, safe_max)
    assert 0 < safe.sum() < P
    tol = slack_tol + 4 * 2.0 ** -53 * (np.abs(vc) + np.abs(out["alpha"]))
    err = np.abs((vc - out["alpha"]) - pen)
    print("max |(values - alpha) - pen| %.3e, max err / tol %.3e, left out %d of %d"
          % (err[keep].max(), (err[keep] / tol[keep]).max(), np.count_nonzero(~keep), P))
    assert np.all(err[keep] <= tol[keep])


# ---- 4. device loop == host loop ---------------------------------------------------------------

@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2]], ids=[ref.IDS[1], ref.IDS[2]])
def test_device_loop_bit_identical_to_host_loop(mods, case):
    """``sgp_swarm_run_ise`` with the host's random numbers against the reference loop over
    ``sgp_swarm_fitness_ise``, 3 iterations, 37 particles (the few-points posterior; below
    kSmallSwarm, where an 'ise' run still takes the general launches) and 5000 (the sweep):
    every state array bit-identical, the generator left in the same state."""
    safeopt_amd = mods[0]
    from safeopt_amd.swarm import SwarmOptimization, DeviceSwarmOptimization
    kind, d, n, P, T, variant = case
    assert P in (37, 5000)
    gps = device_gps(case)
    opt = safeopt_amd.SafeOptSwarm(gps, list(ref.fmin_split(case)), bounds=[(-3.0, 3.0)] * d,
                                   beta=ref.BETA, scaling=ref.SCALING[:len(gps)], swarm_size=P)
    ise = (ref.problem(case)[3],) + target_posterior(case)
    start = np.array(ref.problem(case)[2])
    host = SwarmOptimization(P, opt.optimal_velocities, partial(opt._compute_ise_fitness, ise),
                             bounds=opt.bounds)
    dev = DeviceSwarmOptimization(P, opt.optimal_velocities, opt, 'ise', bounds=opt.bounds,
                                  rng='numpy')
    dev.set_targets(*ise)
    res = []
    for sw in (host, dev):
        np.random.seed(11)
        sw.init_swarm(start.copy())
        sw.run_swarm(3)
        res.append((sw.positions.copy(), sw.velocities.copy(), sw.best_positions.copy(),
                    np.array(sw.best_values), np.array(sw.global_best), np.random.rand()))
    for a, b in zip(res[0], res[1]):
        assert_array_equal(a, b)
    assert not np.array_equal(res[1][0], start)              # the swarm really moved
    assert_array_equal(dev.fitness(start)[0], host.fitness(start)[0])


# ---- 5. end to end -----------------------------------------------------------------------------

def test_ise_point_end_to_end(mods):
    res = {}
    for pso in ("host", "device", "device-rng"):
        opt = _swarm_problem(mods, pso, swarm_size=20)
        before = (opt.S.copy(), opt.greedy_point.copy(), opt.best_lower_bound, opt.t)
        np.random.seed(8)
        x, alpha, st = opt.ise_point(targets=40, about='all', max_iters=6, return_state=True)
        d, G = opt.gp.input_dim, len(opt.gps)
        assert x.shape == (d,) and isinstance(alpha, float) and alpha >= 0.0
        assert sorted(st) == ['target', 'targets', 'zmean', 'zvar']
        assert st['targets'].shape == (40, d) and st['target'].shape == (d,)
        assert st['zmean'].shape == (G, 40) and st['zvar'].shape == (G, 40)
        bounds = np.asarray(opt.bounds)
        assert np.all(x >= bounds[:, 0]) and np.all(x <= bounds[:, 1])
        assert np.all(st['targets'] >= bounds[:, 0]) and np.all(st['targets'] <= bounds[:, 1])
        assert opt._compute_particle_fitness('safe_set', x[None, :])[1].all()
        ise = (st['targets'], st['zmean'], st['zvar'])
        v, s, o = opt._compute_ise_fitness(ise, x[None, :], want=("alpha", "target"))
        assert alpha == o["alpha"][0]
        assert_array_equal(st['target'], st['targets'][o["target"][0]])
        assert_array_equal(opt.S, before[0])
        assert_array_equal(opt.greedy_point, before[1])
        assert opt.best_lower_bound == before[2] and opt.t == before[3]
        res[pso] = (x, alpha, st)
        # about='unsafe' keeps the targets that are not certified safe, and only those
        np.random.seed(8)
        xu, au, su = opt.ise_point(targets=40, max_iters=2, return_state=True)
        beta = opt.beta(opt.t)
        low = st['zmean'] - beta * np.sqrt(st['zvar'])
        unsafe = ~np.all(low >= np.asarray(opt.fmin)[:, None], axis=0)
        assert 0 < unsafe.sum() < 40
        assert_array_equal(su['targets'], st['targets'][unsafe])
        # rows given: nothing is drawn for the targets
        np.random.seed(8)
        xr, ar = opt.ise_point(targets=st['targets'], about='all', max_iters=6)
        if pso != "device-rng":
            np.random.seed(8)
            np.random.rand(40, d)
            x2, a2 = opt.ise_point(targets=st['targets'], about='all', max_iters=6)
            assert_array_equal(x2, x)
            assert a2 == alpha
    assert_array_equal(res["host"][0], res["device"][0])
    assert res["host"][1] == res["device"][1]
    assert_array_equal(res["host"][2]['targets'], res["device"][2]['targets'])


def test_info_point_returns_the_larger_acquisition(mods):
    opt = _swarm_problem(mods, "device", swarm_size=20)
    opt.max_iters = 5
    np.random.seed(4)
    x, alpha, which = opt.info_point(paths=2, features=64, targets=30, about='all')
    np.random.seed(4)
    xm, am = opt.mes_point(paths=2, features=64)
    xi, ai = opt.ise_point(targets=30, about='all')
    assert which == ('ise' if ai > am else 'mes')
    assert alpha == max(am, ai)
    assert_array_equal(x, xi if which == 'ise' else xm)


def test_info_point_without_a_target_left_is_the_mes_pick(mods):
    """Every target certified safe: ``info_point`` returns the MES pick -- that outcome alone;
    an empty safe set is still an error."""
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd.gp_opt import NoIseTarget
    gp = gpy.models.GPRegression(np.array([[0.], [0.5]]), np.array([[1.], [1.2]]),
                                 noise_var=0.01 ** 2)
    sure = safeopt_amd.SafeOptSwarm(gp, fmin=[-100.], bounds=[[-1., 1.]])
    sure.max_iters = 3
    with pytest.raises(NoIseTarget, match="no target is left"):
        sure.ise_point(targets=4)
    np.random.seed(4)
    x, alpha, which = sure.info_point(paths=2, features=16, targets=4)
    np.random.seed(4)
    xm, am = sure.mes_point(paths=2, features=16)
    assert which == 'mes' and alpha == am
    assert_array_equal(x, xm)
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[-1.]]), noise_var=0.01 ** 2)
    empty = safeopt_amd.SafeOptSwarm(gp, fmin=[0.], bounds=[[-1., 1.]])
    with pytest.raises(RuntimeError, match="The safe set is empty."):
        empty.info_point(paths=2, features=16, targets=4)


# ---- 6. refusals -------------------------------------------------------------------------------

def _raw(case):
    from safeopt_amd import _hip
    devs = [g._fitted() for g in device_gps(case)]
    return _hip, devs, devs[0].ctx, _hip.lib(), _hip.dptr


class _Out(object):
    def __init__(self, P, G, T):
        self.values, self.safe = np.full(P, 7.0), np.full(P, 9, dtype=np.uint8)
        self.alpha, self.target = np.full(P, -3.0), np.full(P, -4, dtype=np.int64)
        self.post, self.pairs = np.full((G, 2, P), -5.0), np.full((P, max(T, 1)), -6.0)
        self.cov = np.full((G, P, max(T, 1)), -8.0)

    def untouched(self):
        return (np.all(self.values == 7.0) and np.all(self.safe == 9) and
                np.all(self.alpha == -3.0) and np.all(self.target == -4) and
                np.all(self.post == -5.0) and np.all(self.pairs == -6.0) and
                np.all(self.cov == -8.0))


def _call_fitness(case, x, P, fmin, targets, zmean, zvar, T, o, diag=True):
    _hip, devs, ctx, lib, dp = _raw(case)
    G = len(devs)
    scaling = ref.SCALING[:G].copy()
    fmin = np.ascontiguousarray(fmin, dtype=np.float64)
    return ctx, lib.sgp_swarm_fitness_ise(
        ctx.h, _hip._gp_array(devs) if G else None, G, dp(x), P, 2.0, dp(fmin), dp(scaling),
        None if targets is None else dp(targets), dp(zmean), dp(zvar), T, dp(o.values),
        o.safe.ctypes.data_as(_hip.c_u8_p), dp(o.alpha), o.target.ctypes.data_as(_hip.c_i64_p),
        dp(o.post), dp(o.pairs) if diag else None, dp(o.cov) if diag else None)


def _call_run(case, state, P, fmin, targets, zmean, zvar, T, shard=None):
    _hip, devs, ctx, lib, dp = _raw(case)
    G = len(devs)
    scaling = ref.SCALING[:G].copy()
    fmin = np.ascontiguousarray(fmin, dtype=np.float64)
    vs = np.full(case[1], 0.1)
    args = (ctx.h, _hip._gp_array(devs), G, 2.0, dp(fmin), dp(scaling), P, dp(state[0]),
            dp(state[1]), dp(state[2]), dp(state[3]), dp(state[4]), dp(vs), None, 1, 3, 1.0,
            -0.3, None, 5, dp(targets), dp(zmean), dp(zvar), T)
    if shard is not None:
        return ctx, lib.sgp_swarm_run_ise_shard(*(args + shard))
    return ctx, lib.sgp_swarm_run_ise(*args)


def _bad_inputs(case):
    """(name, fmin, targets, zmean, zvar, T, message), in the order of the checks: an input
    with TWO faults is refused for the earlier one."""
    d, G = case[1], len(ref.specs(case))
    T = 5
    tg = np.array(ref.problem(case)[3][:T])
    zm, zv = (np.array(a[:, :T]) for a in target_posterior(case))
    fmin = ref.fmin_open(case)
    nan_tg = tg.copy()
    nan_tg[3, d - 1] = np.nan
    neg = zv.copy()
    neg[G - 1, 2] = -1e-3
    dead = np.full(G, -np.inf)
    big = np.zeros((ref_max() + 1, d))
    bigz = np.zeros((G, ref_max() + 1))
    return [("T=0", fmin, tg, zm, zv, 0, "SGP_MAX_ISE"),
            ("T>max", fmin, big, bigz, bigz, ref_max() + 1, "SGP_MAX_ISE"),
            ("nan-target", fmin, nan_tg, zm, zv, T, "not finite"),
            ("negative-zvar", fmin, tg, zm, neg, T, "not a variance"),
            ("no-active-GP", dead, tg, zm, zv, T, "no GP is active"),
            # two faults: the earlier check speaks
            ("T=0+dead", dead, tg, zm, zv, 0, "SGP_MAX_ISE"),
            ("nan-target+negative-zvar", fmin, nan_tg, zm, neg, T, "not finite"),
            ("negative-zvar+dead", dead, tg, zm, neg, T, "not a variance")]


def ref_max():
    from safeopt_amd import _hip
    return _hip.MAX_ISE


def test_bad_targets_are_refused_in_order_with_nothing_written(mods):
    from safeopt_amd import _hip
    case = ref.CASES[9]
    d, G = case[1], len(ref.specs(case))
    x = np.zeros((3, d))
    for name, fmin, tg, zm, zv, T, msg in _bad_inputs(case):
        o = _Out(3, G, min(T, 8))
        for P in (3, 0):                       # (refused even for an empty call)
            ctx, rc = _call_fitness(case, x, P, fmin, tg, zm, zv, T, o, diag=T <= 8)
            assert rc != 0, name
            with pytest.raises(_hip.HipError, match=msg):
                ctx.check(rc)
            assert o.untouched(), name
        state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0),
                 np.full(3, 6.0), np.full(d, 8.0)]
        for shard in (None, (0, 3)):
            ctx, rc = _call_run(case, state, 3, fmin, tg, zm, zv, T, shard=shard)
            with pytest.raises(_hip.HipError, match=msg):
                ctx.check(rc)
            for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)):
                assert np.all(a == val), name
    # no GP comes first
    tg = np.array(ref.problem(case)[3][:5])
    zm, zv = (np.array(a[:, :5]) for a in target_posterior(case))
    o = _Out(3, G, 5)
    _hip_, devs, ctx, lib, dp = _raw(case)
    fmin, scaling = ref.fmin_open(case).copy(), ref.SCALING[:G].copy()
    rc = lib.sgp_swarm_fitness_ise(ctx.h, _hip._gp_array(devs), 0, dp(x), 3, 2.0, dp(fmin),
                                   dp(scaling), dp(tg), dp(zm), dp(zv), 0, dp(o.values),
                                   o.safe.ctypes.data_as(_hip.c_u8_p), None, None, None, None, None)
    with pytest.raises(_hip.HipError, match="no GP"):
        ctx.check(rc)
    assert o.untouched()


def test_empty_calls_oversize_outputs_and_empty_blocks(mods):
    """P <= 0 returns 0 and writes nothing; test outputs above G P T = 2^24 are refused with
    nothing written, behind the empty return; an empty block of a sharded swarm is refused."""
    from safeopt_amd import _hip
    case = ref.CASES[9]
    d, G = case[1], len(ref.specs(case))
    fmin = ref.fmin_open(case)
    tg = np.array(ref.problem(case)[3][:5])
    zm, zv = (np.array(a[:, :5]) for a in target_posterior(case))
    x = np.zeros((3, d))
    o = _Out(3, G, 5)
    for P in (0, -2):
        ctx, rc = _call_fitness(case, x, P, fmin, tg, zm, zv, 5, o)
        assert rc == 0 and o.untouched()
    # an oversize diagnostic request: G P T > 2^24 (the arrays are never touched)
    Pbig = (1 << 24) // (G * 5) + 1
    xbig = np.zeros((Pbig, d))
    ob = _Out(Pbig, G, 1)
    ctx, rc = _call_fitness(case, xbig, Pbig, fmin, tg, zm, zv, 5, ob)
    with pytest.raises(_hip.HipError, match="test outputs"):
        ctx.check(rc)
    assert ob.untouched()
    ctx, rc = _call_fitness(case, xbig, 0, fmin, tg, zm, zv, 5, ob)      # the empty return first
    assert rc == 0
    state = [np.full((3, d), 3.0), np.full((3, d), 4.0), np.full((3, d), 5.0), np.full(3, 6.0),
             np.full(d, 8.0)]

    def untouched():
        return all(np.all(a == val) for a, val in zip(state, (3.0, 4.0, 5.0, 6.0, 8.0)))
    ctx, rc = _call_run(case, state, 0, fmin, tg, zm, zv, 5)
    assert rc == 0 and untouched()
    ctx, rc = _call_run(case, state, 0, fmin, tg, zm, zv, 5, shard=(0, 0))
    assert rc == 0 and untouched()
    ctx, rc = _call_run(case, state, 0, fmin, tg, zm, zv, 5, shard=(0, 6))
    with pytest.raises(_hip.HipError, match="bad swarm size"):
        ctx.check(rc)
    assert untouched()
    # sgp_swarm_fitness knows the types 0..3 only
    devs = _raw(case)[1]
    scaling = ref.SCALING[:G].copy()
    with pytest.raises(_hip.HipError, match="Invalid swarm type"):
        ctx.check(_hip.lib().sgp_swarm_fitness(
            ctx.h, _hip._gp_array(devs), G, 6, _hip.dptr(x), 1, 2.0, _hip.dptr(fmin.copy()),
            _hip.dptr(scaling), 0.0, _hip.dptr(o.values), o.safe.ctypes.data_as(_hip.c_u8_p)))
    assert "ise" not in _hip.SWARM_TYPES


def test_ise_point_errors(mods):
    safeopt_amd, gpy, _, _ = mods
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[-1.]]), noise_var=0.01 ** 2)
    empty = safeopt_amd.SafeOptSwarm(gp, fmin=[0.], bounds=[[-1., 1.]])
    with pytest.raises(RuntimeError, match="The safe set is empty."):
        empty.ise_point(targets=4)
    # every target certified safe: none is left
    gp = gpy.models.GPRegression(np.array([[0.]]), np.array([[1.]]), noise_var=0.01 ** 2)
    sure = safeopt_amd.SafeOptSwarm(gp, fmin=[-100.], bounds=[[-1., 1.]])
    with pytest.raises(RuntimeError, match="no target is left"):
        sure.ise_point(targets=4)
