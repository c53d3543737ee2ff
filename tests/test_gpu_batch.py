"""``SafeOpt.optimize_batch`` on the device (csrc/batch.hip, ``sgp_gp_clone``,
``sgp_grid_batch_next``) against the NumPy restatement tests/_batch_ref.py -- the oracle GPs
refitted on the hallucinated inputs -- with teacher forcing: every pick of the device is judged
on the device's own earlier picks.

Bounds.  Hallucinated intervals ``mean -+ beta sqrt(var_h)``: ``rtol=0, atol=1e-8``, what the
project holds chained rank-1 refreshes to against a refit.  Picks: equal rows, after the oracle
alone has shown a margin above 1e-6 between the best and the second-best eligible value at
every pick (the seeds below were chosen for that on the CPU).  One downdate against
``sgp_grid_rank1_update``: ``atol = 1e-11 k(x, x)``, the bound between two device paths for one
quantity.  Everything the real step left behind: equal bits.

The file also runs with ``SGP_POISON=1`` and ``=2`` in front of it: ``var_h`` is never read
before it is written."""
import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _batch_ref as ref
from _gpu_common import mods  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BETA = 2.0
MARGIN = 1e-6
INTERVAL_ATOL = 1e-8


# ---- the cases ----------------------------------------------------------------------------
def _objective(X, g=0):
    return 1.0 + np.exp(-(X ** 2).sum(1) / X.shape[1]) * (1.0 + 0.2 * g)


def case(name):
    """``dict``: grid (parameters only), per GP (X, Y, kernel kind / columns, noise), fmin,
    scaling, size, ucb, context.  Kernels are built per namespace by ``_kern``."""
    c = dict(fmin=[0.0], scaling='auto', size=6, ucb=False, context=None, threshold=0.2,
             extra=None)
    if name.startswith(('A', 'E', 'F')):
        kind = name.split('-')[1]
        rng = np.random.default_rng(11)
        c['grid'] = _lin([(-2.0, 2.0)] * 2, [37, 41])
        X = rng.uniform(-1.5, 1.5, size=(12, 2))
        noise = 0.05 ** 2
        if name[0] == 'F':
            noise, c['fmin'] = 100 * 1.7, [-10.0]
        c['gps'] = [(X, (_objective(X) + 0.05 * rng.normal(size=12))[:, None],
                     [(kind, [0, 1], 1.7, [0.8, 1.6])], noise)]
        c['ucb'] = name[0] == 'E'
    elif name == 'B':
        rng = np.random.default_rng(5)
        c['grid'] = _lin([(-1.0, 1.0)] * 2, [5, 3])
        X = rng.uniform(-0.8, 0.8, size=(5, 2))
        c['gps'] = [(X, (_objective(X) + 0.05 * rng.normal(size=5))[:, None],
                     [('RBF', [0, 1], 1.7, [0.8, 1.6])], 0.05 ** 2)]
        c['size'] = 4
    elif name == 'C':
        rng = np.random.default_rng(21)
        c['grid'] = _lin([(-2.0, 2.0)] * 2, [37, 41])
        c['context'] = [0.3]
        X = np.hstack([rng.uniform(-1.5, 1.5, size=(99, 2)), np.full((99, 1), 0.3)])
        kern01 = [('Matern52', [0, 1, 2], 1.4, [0.9, 1.3, 2.0])]
        kern2 = [('RBF', [0, 1, 2], 0.8, [1.2, 0.9, 1.5])]
        c['gps'] = [(X, (_objective(X[:, :2], g) + 0.05 * rng.normal(size=99))[:, None], k, 0.05 ** 2)
                    for g, k in enumerate((kern01, kern01, kern2))]
        # one more observation that GP 2 does not see: GPs 0 and 1 share inputs (n = 100), kernel
        # and history -- one factor --, GP 2 has other inputs (n = 99) and another kernel
        x = np.array([0.4, -0.7])
        c['extra'] = (x, np.array([[_objective(x[None])[0], 1.1 * _objective(x[None])[0], np.nan]]))
        c['fmin'] = [0.0, -np.inf, 0.0]
        c['scaling'] = [1.3, 0.7, 2.0]
        c['size'] = 5
    elif name == 'D':
        # n_pad (d + 1) = 800 * 8 = 6400 > 6144 staged doubles: training rows and w are read
        # from global memory
        rng = np.random.default_rng(33)
        c['grid'] = rng.uniform(-1.0, 1.0, size=(200, 7))
        X = rng.uniform(-1.0, 1.0, size=(800, 7))
        c['gps'] = [(X, (_objective(X) + 0.05 * rng.normal(size=800))[:, None],
                     [('RBF', [0, 1, 2, 3], 1.3, [1.1, 1.4, 0.9, 1.6]),
                      ('Matern52', [4, 5, 6], 1.2, [1.5, 1.2, 1.8])], 0.05 ** 2)]
        c['size'] = 3
    else:
        raise KeyError(name)
    return c


def _lin(bounds, num):
    import safeopt_amd
    return safeopt_amd.linearly_spaced_combinations(bounds, num)


def _kern(ns, parts, d):
    k = None
    for kind, cols, var, ls in parts:
        whole = len(parts) == 1 and len(cols) == d
        part = getattr(ns, kind)(len(cols), variance=var, lengthscale=np.array(ls), ARD=True,
                                 **({} if whole else dict(active_dims=list(cols))))
        k = part if k is None else k * part
    return k


def build(mods, c, which='device'):
    """``SafeOpt`` on the device (``which='device'``), or the oracle GPs of the same problem
    with the extra observation appended."""
    safeopt_amd, gpy, gpn, _son = mods
    ns, model = (gpy.kern, gpy.models.GPRegression) if which == 'device' else (gpn, gpn.GPRegression)
    d = c['gps'][0][0].shape[1]
    gps = [model(X, Y, _kern(ns, parts, d), noise_var=noise) for X, Y, parts, noise in c['gps']]
    if which != 'device':
        if c['extra'] is not None:
            x, y = c['extra']
            row = np.hstack([x, c['context']])[None, :]
            for i, gp in enumerate(gps):
                if not np.isnan(y[0, i]):
                    gp.set_XY(np.vstack([gp.X, row]), np.vstack([gp.Y, y[:, [i]]]))
        return gps
    nc = 0 if c['context'] is None else len(c['context'])
    opt = safeopt_amd.SafeOpt(gps if len(gps) > 1 else gps[0], c['grid'],
                              c['fmin'] if len(gps) > 1 else c['fmin'][0], threshold=c['threshold'],
                              scaling=c['scaling'], num_contexts=nc, beta=BETA)
    if c['extra'] is not None:
        opt.add_new_data_point(c['extra'][0], c['extra'][1], context=c['context'])
    return opt


def full_rows(c):
    g = c['grid']
    if c['context'] is None:
        return g
    return np.hstack([g, np.tile(np.asarray(c['context'], dtype=float), (g.shape[0], 1))])


def resident(opt):
    from safeopt_amd import _hip
    be = opt._backend
    return {k: be.download(getattr(_hip, k)) for k in ('Q', 'S', 'M', 'G', 'MEAN', 'VAR')}


def factors(opt):
    return [gp._fitted().factor() for gp in opt.gps]


def check_against_oracle(mods, c, opt, X, rows, var_h):
    """Intervals and picks of a finished batch against the teacher-forced restatement."""
    from safeopt_amd import _hip
    gos = build(mods, c, 'oracle')
    grid = full_rows(c)
    mean = opt._backend.download(_hip.MEAN)
    S, M, G = (np.array(getattr(opt, k)) for k in 'SMG')
    mode = ref.UCB if c['ucb'] else ref.MG_WIDTH
    erows, edown, evar, _vals, margins = ref.batch(
        gos, grid, mean, S, M, G, rows[0], c['size'], BETA, opt.scaling, mode, forced=rows)
    # the resident means are the oracle's to the bound of the posterior tests
    omean = np.array([g.predict_noiseless(grid)[0].ravel() for g in gos])
    assert_allclose(mean, omean, rtol=0, atol=1e-8)
    # intervals of every GP and row after the last downdate
    assert var_h.shape == evar.shape
    lo, up = ref.intervals(mean, var_h, BETA)
    elo, eup = ref.intervals(omean, evar, BETA)
    print("max interval error", max(np.abs(lo - elo).max(), np.abs(up - eup).max()),
          "min margin", min(margins) if margins else None)
    assert_allclose(lo, elo, rtol=0, atol=INTERVAL_ATOL)
    assert_allclose(up, eup, rtol=0, atol=INTERVAL_ATOL)
    # picks: a bad margin is a bad input, not a kernel bug
    assert all(m > MARGIN for m in margins), margins
    assert_array_equal(rows, erows)
    assert len(set(rows.tolist())) == len(rows)
    assert_array_equal(X, c['grid'][rows])
    return margins


CASES = ['A-RBF', 'A-Matern32', 'A-Matern52', 'B', 'C', 'D', 'E-RBF', 'F-RBF']


@pytest.mark.parametrize('name', CASES)
def test_batch_against_refitted_oracle(mods, name):
    c = case(name)
    opt, twin = build(mods, c), build(mods, c)
    x_twin = twin.optimize(context=c['context'], ucb=c['ucb'])
    if name == 'B':
        from safeopt_amd import _hip
        assert _hip.Context.default().last_sweep() == 'step-small'
    before, fac = resident(twin), factors(twin)
    X, rows, var_h = opt.optimize_batch(size=c['size'], context=c['context'], ucb=c['ucb'],
                                        return_state=True)
    assert_array_equal(X[0], x_twin)
    assert X.shape == (c['size'], c['grid'].shape[1]), (X.shape, rows)
    check_against_oracle(mods, c, opt, X, rows, var_h)
    # nothing real changed: the resident state and the GPs are the twin's, bit for bit
    after = resident(opt)
    for k in before:
        assert_array_equal(after[k], before[k], err_msg=k)
    for (Li, al), (Lt, at), gp, gt in zip(factors(opt), fac, opt.gps, twin.gps):
        assert_array_equal(Li, Lt)
        assert_array_equal(al, at)
        assert gp.X.shape == gt.X.shape
    # ... and so is the step after the next measurement
    y = np.array([[1.3 + 0.1 * i for i in range(len(opt.gps))]])
    for o in (opt, twin):
        o.add_new_data_point(X[0], y, context=c['context'])
    xa = opt.optimize(context=c['context'], ucb=c['ucb'])
    xb = twin.optimize(context=c['context'], ucb=c['ucb'])
    assert_array_equal(xa, xb)
    for k in 'QSMG':
        assert_array_equal(getattr(opt, k), getattr(twin, k), err_msg=k)


def test_batch_ends_when_the_sets_run_out(mods):
    """Case G: |M u G| = 3 and size = 8: exactly three rows, no error."""
    from safeopt_amd import _hip
    c = case('A-RBF')
    opt = build(mods, c)
    opt.optimize()
    keep = np.flatnonzero(np.array(opt.M) | np.array(opt.G))[[0, 7, 19]]
    m = np.zeros(opt.inputs.shape[0], dtype=bool)
    m[keep[:2]] = True
    g = np.zeros_like(m)
    g[keep[2]] = True
    opt.M[:] = m
    opt.G[:] = g
    x0 = opt.get_new_query_point()                 # (uploads the masks)
    row0 = int(np.flatnonzero((opt.inputs == x0).all(1))[0])
    assert row0 in keep
    rows, downdates, var_h = opt._backend.batch(opt.inputs, row0, 8, _hip.ARGMAX_MG_WIDTH, BETA,
                                                opt.scaling, want_var=True)
    assert sorted(rows.tolist()) == sorted(keep.tolist()) and downdates == 3
    gos = build(mods, c, 'oracle')
    evar = ref.refit_variances(gos, opt.inputs, opt.inputs[rows])
    mean = opt._backend.download(_hip.MEAN)
    assert_allclose(ref.intervals(mean, var_h, BETA)[1], ref.intervals(mean, evar, BETA)[1],
                    rtol=0, atol=INTERVAL_ATOL)


def test_tie_goes_to_the_lower_row(mods):
    """Two symmetric observations on a symmetric 1-d grid, the centre row hallucinated: rows i
    and 128 - i have the same variance by symmetry (in different workgroups).  Equal device
    values: the lower row wins; values that differ in their last bits: either row, and the two
    values agree to 1e-8."""
    safeopt_amd, gpy, gpn, _son = mods
    from safeopt_amd import _hip
    grid = np.linspace(-2.0, 2.0, 129)[:, None]
    X = np.array([[-0.5], [0.5]])
    Y = np.array([[1.2], [1.2]])
    gp = gpy.models.GPRegression(X, Y, gpy.kern.RBF(1, variance=1.5, lengthscale=0.7),
                                 noise_var=1e-3)
    go = gpn.GPRegression(X, Y, gpn.RBF(1, variance=1.5, lengthscale=0.7), noise_var=1e-3)
    opt = safeopt_amd.SafeOpt(gp, grid, -50.0, threshold=0.0, beta=BETA)
    opt.optimize()
    opt.M[:] = True
    opt.get_new_query_point()
    val = ref.rule_values(go.predict_noiseless(grid)[0].T, ref.refit_variances([go], grid, grid[[64]]),
                          BETA, opt.scaling, ref.MG_WIDTH)
    lo_row, margin = ref.pick(val, np.ones(129, bool), [64])
    pair = {lo_row, 128 - lo_row}
    assert len(pair) == 2 and lo_row // 64 != (128 - lo_row) // 64
    third = val[np.setdiff1d(np.arange(129), [64] + sorted(pair))].max()
    assert val[lo_row] - third > MARGIN
    be = opt._backend
    clones = [dv.clone() for dv in be._dev()]
    try:
        assert all(cl.append(grid[64], 0.0) for cl in clones)
        v1, r1 = be.grid.batch_next(clones, True, _hip.ARGMAX_MG_WIDTH, BETA, opt.scaling, [64])
        v2, r2 = be.grid.batch_next(clones, True, _hip.ARGMAX_MG_WIDTH, BETA, opt.scaling, [64, r1])
    finally:
        for cl in clones:
            cl.destroy()
    assert {r1, r2} == pair
    if v1 == v2:
        assert r1 == min(pair)
    else:
        assert abs(v1 - v2) <= 1e-8
    assert abs(v1 - val[lo_row]) <= 1e-8


def test_one_downdate_equals_the_rank1_refresh(mods):
    """``var_h`` after the first downdate against a twin that really appends ``x_0`` and takes
    ``sgp_grid_rank1_update``: two device paths for one quantity."""
    from safeopt_amd import _hip
    for name in ('A-Matern52', 'C'):
        c = case(name)
        opt, twin = build(mods, c), build(mods, c)
        X, rows, var_h = opt.optimize_batch(size=2, context=c['context'], return_state=True)
        assert len(rows) == 2
        twin.optimize(context=c['context'])
        twin.add_new_data_point(X[0], np.zeros((1, len(twin.gps))), context=c['context'])
        # (the backend directly: setting a context again would ask for a full sweep)
        twin._backend.confidence(BETA, twin.fmin)
        assert twin._backend._rank1_streak == 1            # (the closed-form refresh ran)
        var = twin._backend.download(_hip.VAR)
        for i, gp in enumerate(opt.gps):
            kdiag = float(gp.kern.Kdiag(np.zeros((1, gp.input_dim)))[0])
            err = np.abs(var_h[i] - var[i]).max()
            print(name, "GP", i, "max |var_h - var| / kdiag", err / kdiag,
                  "equal bits" if np.array_equal(var_h[i], var[i]) else "")
            assert err <= 1e-11 * kdiag


def test_clone(mods):
    safeopt_amd, gpy, gpn, _son = mods
    rng = np.random.default_rng(2)
    X = rng.uniform(-1.5, 1.5, size=(12, 2))
    Y = _objective(X)[:, None]
    pts = rng.uniform(-2, 2, size=(300, 2))
    gp = gpy.models.GPRegression(X, Y, gpy.kern.Matern32(2, 1.3, [0.8, 1.1], ARD=True), noise_var=1e-3)
    # (60 one-row appends behind a fit at n = 12: the source has no room for 64 more rows, the
    # clone gets a wider pitch)
    for k in range(60):
        x = rng.uniform(-1.5, 1.5, size=(1, 2))
        gp.set_XY(np.vstack([gp.X, x]), np.vstack([gp.Y, _objective(x)[:, None]]))
    for n_expect in (72,):
        dev = gp._fitted()
        assert dev.n == n_expect and dev.appended
        m0, v0 = dev.predict(pts)
        L0, a0 = dev.factor()
        twin = dev.clone()
        assert twin.n == dev.n and twin.serial != dev.serial
        m1, v1 = twin.predict(pts)
        assert_array_equal(m1, m0)
        assert_array_equal(v1, v0)
        L1, a1 = twin.factor()
        assert_array_equal(L1, L0)
        assert_array_equal(a1, a0)
        # appending to the clone leaves the source alone
        for k in range(64):
            assert twin.append(rng.uniform(-1.5, 1.5, size=2), 0.5)
        assert twin.n == n_expect + 64 and dev.n == n_expect
        L2, a2 = dev.factor()
        assert_array_equal(L2, L0)
        assert_array_equal(a2, a0)
        m2, v2 = dev.predict(pts)
        assert_array_equal(m2, m0)
        assert_array_equal(v2, v0)
        # the clone after its appends is the GP fitted on all rows, to the bound of append
        Lt, _ = twin.factor()
        assert_array_equal(Lt[:n_expect, :n_expect], L0)
        # the source goes first: the clone stays usable
        second = dev.clone()
        gp._dev.destroy()
        m3, v3 = second.predict(pts)
        assert_array_equal(m3, m0)
        assert_array_equal(v3, v0)
        assert second.append(np.array([0.1, 0.2]), 1.0)
        assert np.isfinite(second.predict(pts)[1]).all()
        second.destroy()
        twin.destroy()
        gp._dev = None
        gp._dev_fitted = False


def test_argument_errors(mods):
    safeopt_amd, gpy, gpn, _son = mods
    from safeopt_amd import _hip
    c = case('B')
    opt = build(mods, c)
    with pytest.raises(ValueError):
        opt.optimize_batch(size=65)
    opt.optimize()
    be = opt._backend
    devs = be._dev()
    # the user's GPs carry no append record: refused like a rank-1 update without one
    with pytest.raises(_hip.HipError):
        be.grid.batch_next(devs, True, _hip.ARGMAX_MG_WIDTH, BETA, opt.scaling, [0])
    clones = [dv.clone() for dv in devs]
    try:
        assert all(cl.append(opt.inputs[0], 0.0) for cl in clones)
        with pytest.raises(_hip.HipError):
            be.grid.batch_next(clones, True, _hip.ARGMAX_LCB, BETA, opt.scaling, [0])
        with pytest.raises(_hip.HipError):
            be.grid.batch_next(clones, True, _hip.ARGMAX_UCB, BETA, opt.scaling, list(range(65)))
    finally:
        for cl in clones:
            cl.destroy()
