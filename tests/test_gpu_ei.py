"""Log expected improvement on the device (csrc/ei.hip; needs an MI355X): ``sgp_ei_eval``,
``sgp_grid_ei`` and ``SafeOpt.ei_point`` against tests/_ei_ref.py -- the definitions in 50-digit
mpmath and the float64 restatement of the device's stable forms.

Tolerance of ``ln h`` and ``ln Phi``, per point, in units of ``EPS (1 + z^2 / 2)`` (both are
``-z^2 / 2`` to leading order for very negative z): the restatement's own maximum over the points
of the test is measured against mpmath IN the test, and the device is allowed 4 times that --
the factor and the yardstick of tests/test_gpu_mes.py; the device differs from the restatement
only through the math library's erfcx / erfc, exp and log.  Both maxima are printed, and
written to the file ``SAFEOPT_EI_PARITY_OUT`` names when it is set (profiles/ei/parity.txt was
taken that way).  Everything else is equality: bits of a row against the same row elsewhere,
arg-max, incumbent.

The grids: ``line`` (1000 rows: four workgroups, the last ragged) and ``plane`` (70 x 70: twenty)
of tests/_mes_problems.py, three GPs on the first 1500 rows of ``plane``, and the converged run
of tests/_ei_problems.py.  The file also passes with ``SGP_POISON=1`` in front of it.
"""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _ei_problems as EP
import _ei_ref as ref
import _mes_problems as P
from _gpu_common import build_opt, mods                                     # noqa: F401

pytestmark = pytest.mark.gpu

FACTOR = 4.0
KINDS = (("ei", ref.EI), ("pi", ref.PI))


@pytest.fixture(scope="module")
def ctx(hip_device):
    from safeopt_amd import _hip
    return _hip.Context.default()


def _record(line):
    print(line)
    out = os.environ.get("SAFEOPT_EI_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


# ---- 1. term by term ---------------------------------------------------------------------------

def test_terms_against_mpmath(ctx):
    """G = 1, var = 1, tau = 0, xi = 0, mean = z: alpha = ln h(z) (EI: ln(1) / 2 = 0 is added,
    exactly) and ln Phi(z) (PI)."""
    z, eh, en, host_h, host_n = ref.reference()
    one = np.ones(1)
    for name, kind, exact, host_u in (("log_h", ref.EI, eh, host_h), ("log_ndtr", ref.PI, en, host_n)):
        got = ctx.ei_eval(z, np.ones_like(z), 0.0, 0.0, kind)
        dev_u = ref.units(got, z, exact)
        _record("var = 1, %s: %d points; max error in units of EPS (1 + z^2 / 2): host restatement "
                "%.3f, device %.3f at z = %r (allowed %.3f)"
                % (name, z.size, host_u.max(), dev_u.max(), float(z[np.argmax(dev_u)]),
                   FACTOR * host_u.max()))
        assert np.all(np.isfinite(got))
        assert dev_u.max() <= FACTOR * host_u.max()
        # one call per point: the same bits
        single = np.array([ctx.ei_eval(z[i:i + 1], one, 0.0, 0.0, kind)[0] for i in range(z.size)])
        assert_array_equal(single, got)


@pytest.mark.parametrize("var", [1e-15, 1e-30, 1e6])
def test_terms_at_other_variances(ctx, var):
    """alpha = ln(v) / 2 + ln h(z) (EI) and ln Phi(z) (PI) against the same sums in mpmath; the
    yardstick is the restatement's error on the same points, the rounding of ln(v) / 2 and of
    the sum included."""
    import mpmath as mp
    v = max(var, 1e-15)                                               # 1e-30 is clipped
    sigma = np.sqrt(v)
    means = np.concatenate([np.linspace(-40.0, 40.0, 321), [0.0, -0.0]]) * sigma
    z = means / sigma                                                 # as the device forms it
    vars_ = np.full(means.size, var)
    for name, kind in KINDS:
        if kind == ref.EI:
            with mp.workdps(50):
                exact = [e + mp.log(mp.mpf(float(v))) / 2 for e in ref.log_h_mp(z)]
        else:
            exact = ref.log_ndtr_mp(z)
        host_u = ref.units(ref.alpha(means, vars_, 0.0, 0.0, kind), z, exact)
        got = ctx.ei_eval(means, vars_, 0.0, 0.0, kind)
        dev_u = ref.units(got, z, exact)
        _record("var = %g, %s: %d points; host restatement %.3f, device %.3f (allowed %.3f)"
                % (var, name, z.size, host_u.max(), dev_u.max(), FACTOR * host_u.max()))
        assert np.all(np.isfinite(got))
        assert dev_u.max() <= FACTOR * host_u.max()
        single = np.array([ctx.ei_eval(means[i:i + 1], vars_[:1], 0.0, 0.0, kind)[0]
                           for i in range(means.size)])
        assert_array_equal(single, got)


# ---- 2. launch independence --------------------------------------------------------------------

NS = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("G", [1, 3])
def test_rows_do_not_depend_on_launch(ctx, G):
    rng = np.random.default_rng(200 + G)
    mean = rng.normal(size=(G, 1000))
    var = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), size=(G, 1000)))
    one_inf = np.array([0.2, -np.inf, -0.4])[:G] if G == 3 else np.array([-np.inf])
    tau, xi = 0.4, 0.01
    host_max = max(ref.reference()[3].max(), ref.reference()[4].max())
    sig = np.sqrt(var)
    for name, kind in KINDS:
        for f in (None, one_inf, np.full(G, -0.3)):
            full = ctx.ei_eval(mean, var, tau, xi, kind, f)
            # against the restatement: every logarithm within the tolerance of test 1 in its
            # own unit, ln(v) / 2 and each of the at most G + 1 additions within an EPS of
            # the size of the sum
            want = ref.alpha(mean, var, tau, xi, kind, f)
            z = (mean[0] - tau - xi) / sig[0]
            unit = 1.0 + 0.5 * z * z
            for g in range(G):
                if f is not None and np.isfinite(f[g]):
                    unit = unit + 1.0 + 0.5 * ((mean[g] - f[g]) / sig[g]) ** 2
            tol = ref.EPS * (FACTOR * host_max * unit +
                             (G + 2) * (np.abs(want) + np.abs(0.5 * np.log(var[0]))))
            assert np.all(np.abs(full - want) <= tol)
            for N in NS:
                assert_array_equal(ctx.ei_eval(mean[:, :N], var[:, :N], tau, xi, kind, f), full[:N])
                perm = rng.permutation(1000)[:N]
                assert_array_equal(ctx.ei_eval(mean[:, perm], var[:, perm], tau, xi, kind, f),
                                   full[perm])
        # no weights: NULL and all -inf
        assert_array_equal(ctx.ei_eval(mean, var, tau, xi, kind, None),
                           ctx.ei_eval(mean, var, tau, xi, kind, np.full(G, -np.inf)))
        # an entry of -inf: the GP adds nothing, whatever its posterior
        if G == 3:
            other = mean.copy()
            other[1] = -other[1]
            assert_array_equal(ctx.ei_eval(other, var, tau, xi, kind, one_inf),
                               ctx.ei_eval(mean, var, tau, xi, kind, one_inf))


def test_a_call_in_several_launches(ctx):
    """More rows than one launch of ``sgp_ei_eval`` takes (2^18): the chunks' rows have the bits
    of the same rows alone."""
    rng = np.random.default_rng(7)
    N = (1 << 18) + 1000
    mean, var = rng.normal(size=(2, N)), np.exp(rng.uniform(-8.0, 1.0, size=(2, N)))
    got = ctx.ei_eval(mean, var, 0.5, 0.0, ref.EI, [-np.inf, 0.1])
    tail = slice((1 << 18) - 300, N)
    assert_array_equal(got[tail], ctx.ei_eval(mean[:, tail], var[:, tail], 0.5, 0.0, ref.EI,
                                              [-np.inf, 0.1]))
    assert_array_equal(got[:500], ctx.ei_eval(mean[:, :500], var[:, :500], 0.5, 0.0, ref.EI,
                                              [-np.inf, 0.1]))


# ---- 3. refusals, with nothing written ---------------------------------------------------------

@pytest.mark.parametrize("G, kind, tau, xi", [
    (0, 0, 0.0, 0.0), (9, 0, 0.0, 0.0), (1, 2, 0.0, 0.0), (1, 0, float("nan"), 0.0),
    (1, 0, float("inf"), 0.0), (1, 0, 0.0, -1.0), (1, 0, 0.0, float("nan"))],
    ids=["G=0", "G=9", "kind=2", "tau=nan", "tau=inf", "xi=-1", "xi=nan"])
def test_bad_arguments_are_refused_with_nothing_written(ctx, G, kind, tau, xi):
    from safeopt_amd import _hip
    mean, var = np.zeros((9, 5)), np.ones((9, 5))
    out = np.full(5, -7.0)
    rc = _hip.lib().sgp_ei_eval(ctx.h, _hip.dptr(mean), _hip.dptr(var), 5, G, None, kind, tau,
                                xi, _hip.dptr(out))
    assert rc != 0 and np.all(out == -7.0)
    # N = 0: nothing to do, nothing written
    assert _hip.lib().sgp_ei_eval(ctx.h, _hip.dptr(mean), _hip.dptr(var), 0, 1, None, 0, 0.0,
                                  0.0, _hip.dptr(out)) == 0
    assert np.all(out == -7.0)


def test_grid_without_a_posterior_is_refused(ctx):
    import ctypes as C
    from safeopt_amd import _hip
    g = _hip.DeviceGrid(ctx, np.linspace(0.0, 1.0, 10)[:, None], 1)
    al = np.full(10, -7.0)
    v, i, tu = C.c_double(-7.0), C.c_int64(-7), C.c_double(-7.0)
    rc = _hip.lib().sgp_grid_ei(g.h, 0, _hip.MES_ALL, _hip.EI_TAU_MEAN, 0.0, 0.0, None,
                                _hip.dptr(al), C.byref(v), C.byref(i), C.byref(tu))
    assert rc != 0 and np.all(al == -7.0) and (v.value, i.value, tu.value) == (-7.0, -7, -7.0)
    with pytest.raises(_hip.HipError, match="no current posterior"):
        g.ei(rows=_hip.MES_ALL)


def test_new_context_columns_void_the_posterior(mods, ctx):
    from safeopt_amd import _hip
    _, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("plane")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    dev = [gp._fitted()]
    g = _hip.DeviceGrid(ctx, z["parameter_set"][:300], 1)
    g.posterior(dev)
    assert g.ei(rows=_hip.MES_ALL)[2] >= 0
    g.set_context([0.25])
    with pytest.raises(_hip.HipError, match="no current posterior"):
        g.ei(rows=_hip.MES_ALL)
    g.posterior(dev)
    assert g.ei(rows=_hip.MES_ALL)[2] >= 0


def test_grid_refuses_bad_arguments(ctx, mods):
    from safeopt_amd import _hip
    g = _three_gps(mods, ctx)["grid"]
    for kw in (dict(kind=2), dict(rows=3), dict(tau=float("nan")), dict(tau=float("inf")),
               dict(tau=-float("inf")), dict(xi=-1.0), dict(xi=float("nan")),
               dict(fmin=[0.0, float("nan"), 0.0]), dict(fmin=[0.0, float("inf"), 0.0])):
        with pytest.raises(_hip.HipError):
            g.ei(**dict(dict(rows=_hip.MES_ALL), **kw))
    with pytest.raises(ValueError):
        g.ei(tau="max")
    with pytest.raises(ValueError):
        g.ei(fmin=[0.0])


# ---- 4. the grid -------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["line", "plane"])
def grid(request, mods, ctx):
    """An optimiser after ``optimize()``, with what the device holds: posterior and masks.  The
    tests of this module leave ``S`` on the device as they found it."""
    from safeopt_amd import _hip
    z, meta = P.problem(request.param)
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    be = opt._backend
    state = dict(name=request.param, opt=opt, be=be, N=z["parameter_set"].shape[0],
                 mean=be.download(_hip.MEAN).copy(), var=be.download(_hip.VAR).copy(),
                 S=np.array(be.download(_hip.S)), M=np.array(be.download(_hip.M)),
                 G=np.array(be.download(_hip.G)))
    assert state["S"].any() and not state["S"].all() and (state["M"] | state["G"]).any()
    return state


_THREE = {}


def _three_gps(mods, ctx):
    """Three GPs (the objective of ``plane`` and two constraints on other data) over the first
    1500 rows of its grid, masks uploaded from a generator: ``mean[g][i]`` with g > 0."""
    cache = _THREE
    if cache:
        return cache
    from safeopt_amd import _hip
    _, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("plane")
    X, Y = z["it0_X0"], z["it0_Y0"]
    ys = [Y, 0.4 * np.cos(2.0 * X[:, :1]) + 0.1, Y[::-1] - 1.0]
    gps = [gpy.models.GPRegression(X, y, make_kernel(gpy.kern, meta["kernels"][0]),
                                   noise_var=P.NOISE * (g + 1)) for g, y in enumerate(ys)]
    N = 1500
    g = _hip.DeviceGrid(ctx, z["parameter_set"][:N], 3)
    g.posterior([gp._fitted() for gp in gps])
    rng = np.random.default_rng(31)
    S = rng.random(N) < 0.4
    M = S & (rng.random(N) < 0.2)
    G = S & ~M & (rng.random(N) < 0.1)
    for what, mask in ((_hip.S, S), (_hip.M, M), (_hip.G, G)):
        g.upload_mask(what, mask)
    cache.update(grid=g, gps=gps, N=N, S=S, M=M, G=G, mean=g.download(_hip.MEAN).copy(),
                 var=g.download(_hip.VAR).copy())
    return cache


FMIN3 = np.array([-np.inf, 0.05, -1.2])


def test_grid_alpha_is_eval_alpha(grid, ctx):
    from safeopt_amd import _hip
    g = grid["be"].grid
    for name, kind in KINDS:
        for fmin in (None, [P.FMIN]):
            al, v, i, tu = g.ei(kind=kind, rows=_hip.MES_S, tau='mean', xi=0.01, fmin=fmin,
                                alpha=True)
            assert tu == grid["mean"][0][grid["S"]].max()
            assert_array_equal(al, ctx.ei_eval(grid["mean"], grid["var"], tu, 0.01, kind, fmin))
            # alpha = False (rows outside the mask are skipped): the same pick
            assert g.ei(kind=kind, rows=_hip.MES_S, tau='mean', xi=0.01, fmin=fmin)[1:] == (v, i, tu)


def test_three_gps_alpha_is_eval_alpha(mods, ctx):
    from safeopt_amd import _hip
    t = _three_gps(mods, ctx)
    for name, kind in KINDS:
        for fmin in (None, FMIN3, np.array([0.3, 0.05, -1.2])):
            al, v, i, tu = t["grid"].ei(kind=kind, rows=_hip.MES_S, tau='mean', fmin=fmin,
                                        alpha=True)
            assert tu == t["mean"][0][t["S"]].max()
            assert_array_equal(al, ctx.ei_eval(t["mean"], t["var"], tu, 0.0, kind, fmin))
            want = int(np.flatnonzero(t["S"])[np.argmax(al[t["S"]])])
            assert (v, i) == (al[want], want)
            assert t["grid"].ei(kind=kind, rows=_hip.MES_S, tau='mean', fmin=fmin)[1:] == (v, i, tu)
    # the weights change alpha: the constraints are felt
    a0 = t["grid"].ei(rows=_hip.MES_ALL, alpha=True)[0]
    a1 = t["grid"].ei(rows=_hip.MES_ALL, fmin=FMIN3, alpha=True)[0]
    assert np.all(a1 < a0)


def _check_pick(state, g, rows, tau, kind, fmin):
    from safeopt_amd import _hip
    N = state["N"]
    mask = {"ALL": np.ones(N, dtype=bool), "S": state["S"], "MG": state["M"] | state["G"]}[rows]
    al, v, i, tu = g.ei(kind=kind, rows=getattr(_hip, "MES_" + rows), tau=tau, fmin=fmin,
                        alpha=True)
    if tau == "mean":
        m0 = state["mean"][0]
        assert tu == (m0.max() if rows == "ALL" else m0[state["S"]].max())
    else:
        assert tu == tau
    assert np.all(np.isfinite(al))
    want = int(np.flatnonzero(mask)[np.argmax(al[mask])])
    assert (v, i) == (al[want], want)
    assert g.ei(kind=kind, rows=getattr(_hip, "MES_" + rows), tau=tau, fmin=fmin)[1:] == (v, i, tu)


@pytest.mark.parametrize("rows", ["ALL", "S", "MG"])
@pytest.mark.parametrize("tau", ["mean", 2.25])
def test_grid_pick_is_first_maximum_over_the_mask(grid, rows, tau):
    for name, kind in KINDS:
        for fmin in (None, [P.FMIN]):
            _check_pick(grid, grid["be"].grid, rows, tau, kind, fmin)


@pytest.mark.parametrize("rows", ["ALL", "S", "MG"])
def test_three_gps_pick_is_first_maximum_over_the_mask(mods, ctx, rows):
    t = _three_gps(mods, ctx)
    for tau in ("mean", 0.7):
        for name, kind in KINDS:
            for fmin in (None, FMIN3):
                _check_pick(t, t["grid"], rows, tau, kind, fmin)


def test_empty_mask_has_no_pick(grid):
    from safeopt_amd import _hip
    be = grid["be"]
    try:
        be.upload_mask(_hip.S, np.zeros(grid["N"], dtype=bool))
        al, v, i, tu = be.grid.ei(rows=_hip.MES_S, tau='mean', alpha=True)
        assert (v, i, tu) == (-np.inf, -1, -np.inf) and np.all(al == -np.inf)
        assert be.grid.ei(rows=_hip.MES_S, tau='mean')[1:] == (-np.inf, -1, -np.inf)
        # an incumbent by value: alpha as ever, still no pick
        al, v, i, tu = be.grid.ei(rows=_hip.MES_S, tau=1.0, alpha=True)
        assert (v, i, tu) == (-np.inf, -1, 1.0) and np.all(np.isfinite(al))
    finally:
        be.upload_mask(_hip.S, grid["S"])


# ---- 5. ties -----------------------------------------------------------------------------------

def test_lowest_row_wins_a_tie_from_a_late_workgroup(grid):
    """ln Phi is exactly 0 far above the incumbent: every row ties, the mask plants the rows."""
    from safeopt_amd import _hip
    be, N = grid["be"], grid["N"]
    first = 256 * ((N - 1) // 256 - 1)               # first row of the last full workgroup
    mask = np.zeros(N, dtype=bool)
    mask[[first, first + 1, first + 300 if first + 300 < N else N - 1, N - 1]] = True
    try:
        be.upload_mask(_hip.S, mask)
        al, v, i, _ = be.grid.ei(kind=_hip.EI_PI, rows=_hip.MES_S, tau=-1e6, alpha=True)
        assert np.all(al == 0.0) and (v, i) == (0.0, first)
        assert be.grid.ei(kind=_hip.EI_PI, rows=_hip.MES_ALL, tau=-1e6)[1:3] == (0.0, 0)
    finally:
        be.upload_mask(_hip.S, grid["S"])


def _planted(grid, ctx, lo, hi, kind):
    """A grid of rows [lo, hi) of the problem whose LAST row is a copy of the row with the
    largest alpha among its first 256: equal (mean, var), hence two equal maxima, one in the
    first workgroup and one in the last; candidates: the first 256 rows and the last."""
    from safeopt_amd import _hip
    opt = grid["opt"]
    dev = [g._fitted() for g in opt.gps]
    pts = np.array(opt.inputs[lo:hi])
    tau = float(grid["mean"][0].max()) + 0.3
    a = ref.alpha(grid["mean"][0][lo:hi], grid["var"][0][lo:hi], tau, kind=kind)
    early = int(np.argmax(a[:256]))
    keep = np.zeros(hi - lo, dtype=bool)
    keep[:256] = True
    keep[-1] = True
    pts[-1] = pts[early]
    shard = _hip.DeviceGrid(ctx, pts, len(dev), global_offset=lo)
    shard.posterior(dev)
    shard.upload_mask(_hip.S, keep)
    return shard, early, tau


@pytest.mark.parametrize("lo", [0, 333])
def test_planted_equal_maxima(grid, ctx, lo):
    """Two rows with the same posterior and the largest alpha, at least three workgroups apart;
    on a shard with ``global_offset > 0`` the global row comes back."""
    from safeopt_amd import _hip
    hi = grid["N"] - 7
    n = hi - lo
    assert (n + 255) // 256 >= 3
    for name, kind in KINDS:
        shard, early, tau = _planted(grid, ctx, lo, hi, kind)
        mean, var = shard.download(_hip.MEAN)[0], shard.download(_hip.VAR)[0]
        assert (mean[n - 1], var[n - 1]) == (mean[early], var[early])
        al, v, i, tu = shard.ei(kind=kind, rows=_hip.MES_S, tau=tau, alpha=True)
        assert al[n - 1] == al[early] == al[:256].max() and tu == tau
        assert np.count_nonzero(al[:256] == al[early]) == 1
        assert (v, i) == (al[early], lo + early)
        assert shard.ei(kind=kind, rows=_hip.MES_S, tau=tau)[1:3] == (v, i)
        # the shard's rows have the bits of the whole grid's rows
        whole = grid["be"].grid.ei(kind=kind, rows=_hip.MES_ALL, tau=tau, alpha=True)[0]
        assert_array_equal(al[:-1], whole[lo:hi - 1])


# ---- 6. ei_point end to end --------------------------------------------------------------------

def _state(opt):
    from safeopt_amd import _hip
    be = opt._backend
    out = [np.array(be.download(w)) for w in (_hip.Q, _hip.S, _hip.M, _hip.G, _hip.MEAN,
                                              _hip.VAR)]
    out.extend([np.array(opt.x), np.array(opt.y)])
    out.extend(np.array(a) for a in opt.gp._fitted().factor())
    return out


def test_ei_point_end_to_end(grid):
    opt, S = grid["opt"], grid["S"]
    mean, var = grid["mean"], grid["var"]
    before = _state(opt)
    x, a, values, tau = opt.ei_point(return_values=True)
    assert tau == mean[0][S].max() and values.shape == (grid["N"],)
    row = int(np.flatnonzero(S)[np.argmax(values[S])])
    assert S[row] and a == values[row] == values[S].max()
    assert_array_equal(x, opt.inputs[row])
    x2, a2 = opt.ei_point()
    assert_array_equal(x2, x)
    assert a2 == a
    # the restatement on the downloaded posterior: within the tolerance of test 1, row by row
    want = ref.alpha(mean[0], var[0], tau)
    z = (mean[0] - tau) / np.sqrt(np.maximum(var[0], 1e-15))
    host_max = ref.reference()[3].max()
    assert np.all(np.abs(values - want) <=
                  (FACTOR * host_max + 4.0) * ref.EPS * (1.0 + 0.5 * z * z + np.abs(want)))
    # candidates M | G: a row of M | G, the same alpha array
    x3, a3, values3, tau3 = opt.ei_point(within='MG', return_values=True)
    mg = grid["M"] | grid["G"]
    assert_array_equal(values3, values)
    assert tau3 == tau
    r3 = int(np.flatnonzero(mg)[np.argmax(values[mg])])
    assert_array_equal(x3, opt.inputs[r3])
    assert mg[r3] and a3 == values[r3]
    # the incumbent as passed
    best = float(opt.y[:, 0].max())
    assert opt.ei_point(incumbent='data', return_values=True)[3] == best
    x5, a5, values5, tau5 = opt.ei_point(incumbent=1.75, xi=0.25, kind='pi', return_values=True)
    assert tau5 == 1.75
    assert_array_equal(values5, opt._backend.grid.ctx.ei_eval(mean, var, 1.75, 0.25, ref.PI))
    # feasibility: the weights of the finite fmin
    values6 = opt.ei_point(feasibility=True, return_values=True)[2]
    assert_array_equal(values6, opt._backend.grid.ctx.ei_eval(mean, var, tau, 0.0, ref.EI,
                                                              [P.FMIN]))
    # no mask at all
    x4, a4, values4, tau4 = opt.ei_point(within='all', return_values=True)
    assert tau4 == mean[0].max() and a4 == values4.max()
    for u, w in zip(before, _state(opt)):
        assert_array_equal(u, w)


def test_ei_point_without_a_safe_row(mods):
    z, meta = P.problem("line")
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    opt.S[:] = False
    with pytest.raises(RuntimeError, match="no safe points"):
        opt.ei_point()


def test_converged_run_where_ei_underflows(mods):
    """tests/_ei_problems.py: sigma small on every row, the improvement asked for hundreds of
    sigma away.  EI is exactly 0 on every safe row -- asserted, so that the test checks what it
    claims -- and the pick is still one row: the arg-max of the restatement on the downloaded
    posterior (tests/test_ei_cpu.py: on the oracle's posterior its two largest values differ
    by 6.6e3, the tolerance of test 1 is below 3e-8 on every row)."""
    from safeopt_amd import _hip
    z, meta = EP.converged()
    opt = build_opt(mods, z, meta, 0)
    opt.update_confidence_intervals()
    opt.compute_safe_set()
    be = opt._backend
    x, a, values, tau = opt.ei_point(xi=EP.XI, return_values=True)
    S = np.array(be.download(_hip.S))
    mean, var = be.download(_hip.MEAN)[0], be.download(_hip.VAR)[0]
    assert S.sum() > 500 and tau == mean[S].max()
    assert np.all(np.isfinite(values)) and np.exp(values[S]).max() == 0.0
    want = ref.alpha(mean, var, tau, EP.XI)
    zrow = (mean - tau - EP.XI) / np.sqrt(np.maximum(var, 1e-15))
    tol = FACTOR * ref.reference()[3].max() * ref.EPS * (1.0 + 0.5 * zrow * zrow)
    assert EP.top_two_gap(want, S) > 2.0 * tol.max()
    row = int(np.flatnonzero(S)[np.argmax(want[S])])
    assert np.count_nonzero(values[S] == values[S].max()) == 1
    assert_array_equal(x, opt.inputs[row])
    assert a == values[row]


# ---- 7. the GP's own method --------------------------------------------------------------------

def test_log_expected_improvement_of_a_gp(mods, ctx):
    """``GPRegression.log_expected_improvement``: predict_noiseless, then sgp_ei_eval."""
    _, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("plane")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    X = z["parameter_set"][::37]
    a = gp.log_expected_improvement(X, 1.5, xi=0.02)
    mean, var = gp.predict_noiseless(X)
    assert a.shape == (X.shape[0], 1)
    assert_array_equal(a[:, 0], ctx.ei_eval(mean[:, 0], var[:, 0], 1.5, 0.02))
    assert_array_equal(gp.log_expected_improvement(X, 1.5)[:, 0],
                       ctx.ei_eval(mean[:, 0], var[:, 0], 1.5))
