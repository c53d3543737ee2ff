"""GPU parity of the removal of any observation -- ``sgp_gp_remove`` (factor.hip: the downdate
of L^-1 and alpha) and ``sgp_grid_rank1_remove`` (k_rank1<.., true>, expander.hip: the resident
posterior corrected in closed form) -- against long-double refits of the reduced data
(tests/_remove_ref.py), through the C ABI and through SafeOpt.

Tolerances: the project's, as tests/test_gpu_incremental.py has them -- 1e-8 on L^-1
(absolute), alpha (relative to max |alpha|) and Q, ``check_posterior`` (1e-9, 1e-5 relative) on
mean and variance, equality of S outside the rows within 1e-8 of fmin.  What a float64
implementation gives on the factor cases is in tests/test_remove_cpu.py and
profiles/remove/SUMMARY.txt: at most 2e-11."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _remove_ref as R
from _golden import load
from _gpu_common import (  # noqa: F401
    MEAN_TOL, VAR_TOL, mods, build_opt, check_posterior)

pytestmark = pytest.mark.gpu

LINV_TOL = ALPHA_TOL = Q_TOL = RET_TOL = LL_TOL = 1e-8


def _gp(gpy, spec, X, Y):
    return gpy.models.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpy.kern, spec),
                                   noise_var=R.NOISE)


def _check_snapshot(gp, snap, Xs, kd, what):
    """alpha, L^-1 and the posterior at Xs against the refit."""
    dev = gp._fitted() if hasattr(gp, "_fitted") else gp
    assert dev.n == snap["n"], what
    Linv, alpha = dev.factor()
    ea = np.max(np.abs(alpha - snap["alpha"])) / np.max(np.abs(snap["alpha"]))
    el = np.max(np.abs(Linv - snap["Linv"]))
    m, v = dev.predict(Xs)
    m, v = m[:, 0], v[:, 0]
    em = np.max(np.abs(m - snap["mean"])) / np.max(np.abs(snap["mean"]))
    ev = np.max(np.abs(v - snap["var"])) / kd
    print("%s: alpha %.2e  L^-1 %.2e  mean %.2e  var %.2e" % (what, ea, el, em, ev))
    assert np.all(Linv[np.triu_indices(dev.n, 1)] == 0.0), what
    assert np.all(np.diag(Linv) > 0.0), what
    assert ea < ALPHA_TOL, what
    assert el < LINV_TOL, what
    check_posterior(m, v, snap["mean"], snap["var"], kd)


# ---- the factor ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FACTOR_CASES))
def test_remove_against_long_double(mods, name):
    """Fit n rows, ``remove(i)``: L^-1, alpha and the posterior at 200 rows against the
    long-double refit without row i."""
    _, gpy, _, _ = mods
    spec, d, n, i = R.FACTOR_CASES[name]
    X, Y, Xs, t = R.factor_reference(name)
    gp = _gp(gpy, spec, X, Y)
    dev = gp._fitted()
    v0 = dev.version
    assert dev.remove(i), "remove refused"
    assert dev.removed and not dev.appended and dev.version == v0 + 1 and dev.n == n - 1
    _check_snapshot(dev, t, Xs, R.kdiag(spec), name)


def test_remove_refuses(mods):
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    spec = R.single("RBF", 1)
    X = np.array([[0.0], [1.0], [2.5]])
    dev = _gp(gpy, spec, X, np.array([0.1, 0.2, 0.3]))._fitted()
    before = dev.factor()
    for bad in (-1, 3, 2 ** 40):
        with pytest.raises(_hip.HipError):
            dev.remove(bad)
    assert dev.n == 3 and not dev.removed
    for a, b in zip(before, dev.factor()):
        assert_array_equal(a, b)
    assert dev.remove(1) and dev.remove(0) and dev.n == 1
    with pytest.raises(_hip.HipError):          # the only observation
        dev.remove(0)


# ---- chains -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CHAINS))
def test_chain(mods, name):
    """remove -> append -> pop, and two removals: the refit of the same data after every call;
    exactly one of ``appended`` / ``removed`` after a one-row change, none after a pop."""
    _, gpy, _, _ = mods
    X, Y, Xs, E, YE, snaps = R.chain_reference(name)
    dev = _gp(gpy, R.CHAIN_SPEC, X, Y)._fitted()
    e = 0
    for (what, row), snap in zip(R.CHAINS[name], snaps):
        if what == "remove":
            assert dev.remove(row) and dev.removed and not dev.appended
        elif what == "append":
            assert dev.append(E[e], YE[e]) and dev.appended and not dev.removed
            e += 1
        else:
            dev.pop()
            assert not dev.appended and not dev.removed
        _check_snapshot(dev, snap, Xs, R.kdiag(R.CHAIN_SPEC), "%s after %s" % (name, what))


def test_append_past_the_old_n_after_a_removal(mods):
    """12 rows, one removed, then ``set_XY`` with one more row three times: bordered appends
    (the capacity of the fit is kept), past the 12 rows the GP once had."""
    _, gpy, _, _ = mods
    spec, d, n, row, more = R.GROW
    X, Y, Xs, E, YE, snaps = R.grow_reference()
    gp = _gp(gpy, spec, X, Y)
    gp.remove_data(row)
    assert gp._dev.removed and gp.X.shape[0] == n - 1
    _check_snapshot(gp, snaps[0], Xs, R.kdiag(spec), "grow: removed")
    for e in range(more):
        gp.set_XY(np.vstack([gp.X, E[e]]), np.vstack([gp.Y, [[YE[e]]]]))
        assert gp._dev.appended and not gp._dev.removed
        _check_snapshot(gp, snaps[1 + e], Xs, R.kdiag(spec), "grow: n = %d" % gp._dev.n)


def test_remove_on_a_clone_leaves_the_source(mods):
    _, gpy, _, _ = mods
    name = "rbf_d3_n130_i64"
    spec, d, n, i = R.FACTOR_CASES[name]
    X, Y, Xs, t = R.factor_reference(name)
    src = _gp(gpy, spec, X, Y)._fitted()
    before = src.factor() + src.predict(Xs)
    twin = src.clone()
    try:
        assert not twin.removed and twin.remove(i) and twin.removed
        _check_snapshot(twin, t, Xs, R.kdiag(spec), "clone")
        assert src.n == n and not src.removed
        for a, b in zip(before, src.factor() + src.predict(Xs)):
            assert_array_equal(a, b)
    finally:
        twin.destroy()


def test_log_likelihood_after_a_removal(mods):
    """The likelihood factorises the resident data again: X and Y were compacted on the device."""
    _, gpy, _, _ = mods
    X, Y, _, _, _, _ = R.chain_reference("remove_twice")
    gp = _gp(gpy, R.CHAIN_SPEC, X, Y)
    gp.remove_data(5)
    keep = np.arange(len(X)) != 5
    want = R.log_likelihood_ld(R.CHAIN_SPEC, X[keep], Y[keep])
    got = gp.log_likelihood()
    print("log likelihood %.12g, long double %.12g" % (got, want))
    assert abs(got - want) < LL_TOL * max(abs(want), 1.0)
    assert_array_equal(gp.X, X[keep])


# ---- the grid -----------------------------------------------------------------------------
def _compare_grid(grid, G, exp, fmin, kd, ret, what):
    from safeopt_amd import _hip
    mean, var = grid.download(_hip.MEAN), grid.download(_hip.VAR)
    Q, S = grid.download(_hip.Q), grid.download(_hip.S)
    for g in range(G):
        em = np.max(np.abs(mean[g] - exp["mean"][g])) / np.max(np.abs(exp["mean"][g]))
        ev = np.max(np.abs(var[g] - exp["var"][g])) / kd[g]
        eq = np.max(np.abs(Q[:, 2 * g:2 * g + 2] - exp["Q"][:, 2 * g:2 * g + 2]))
        print("%s GP %d: mean %.2e  var %.2e  Q %.2e" % (what, g, em, ev, eq))
    for g in range(G):
        check_posterior(mean[g], var[g], exp["mean"][g], exp["var"][g], kd[g])
    assert np.max(np.abs(Q - exp["Q"])) < Q_TOL, what
    keep = ~exp["excluded"]
    assert np.array_equal(S[keep], exp["S"][keep]), what
    if ret is not None:
        want = exp["ret"]
        assert ret[1] == want[1], what
        if want[1]:
            assert abs(ret[0] - want[0]) < RET_TOL, what
        else:
            assert ret[0] == -np.inf, what


def _setup_grid(mods, name):
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case, ref = R.GRID_CASES[name], R.grid_reference(name)
    G = len(case["gps"])
    gps = [_gp(gpy, c[0], ref["X"][g], ref["Y"][g]) for g, c in enumerate(case["gps"])]
    devs = [gp._fitted() for gp in gps]
    pts = ref["pts"]
    if case["ctx_col"] is not None:
        pts = pts.copy()                    # made with another context and told the case's one
        pts[:, -1] = 9.0
    grid = _hip.DeviceGrid(devs[0].ctx, pts, G)
    if case["tensor"]:
        assert grid.set_axes(_hip.tensor_grid_axes(pts))
    if case["ctx_col"] is not None:
        grid.set_context([case["ctx_col"]])
    return case, ref, G, devs, grid


def _run_grid(mods, name, defer=False):
    """Sweep, then per step: ``remove`` on the GPs with a row to lose, ``rank1_remove`` with
    another beta, and mean, var, Q, S and the returned maximum against the refits."""
    case, ref, G, devs, grid = _setup_grid(mods, name)
    ctx = devs[0].ctx
    which = [int(c[3] is not None) for c in case["gps"]]
    old = ctx.set_share(case["share"]) if case["share"] is not None else None
    try:
        grid.confidence(devs, ref["beta0"], ref["fmin"])
        for t, st in enumerate(ref["steps"]):
            for g, c in enumerate(case["gps"]):
                if which[g]:
                    assert devs[g].remove(c[3])
            ret = grid.rank1_remove(devs, which, st["beta"], ref["fmin"], defer=defer)
            if defer:
                assert ret == (None, None)
                # the maximum stays on the device and comes back with the set pass
                out = grid.sets_fused(devs, st["beta"], ref["fmin"], None, np.ones(G),
                                      np.full(G, 0.05), 0.5)
                ret = (out[7], bool(st["S"].any()))
            _compare_grid(grid, G, st, ref["fmin"], ref["kdiag"], ret, "%s step %d" % (name, t))
    finally:
        if old is not None:
            ctx.set_share(old)
    return devs, grid


@pytest.mark.parametrize("name", sorted(set(R.GRID_CASES) - {"streak_mat52_d2"}))
def test_rank1_remove_against_long_double(mods, name):
    """1000 rows, tensor and scattered; one GP, one of three, all three; n = 17, 200 and 700
    (699 rows of d = 8 do not fit the LDS stage); followers of a shared factor; a context
    column: the GPs that lost a row against the refit of n - 1 rows, the others against
    their n rows with the new beta.  On the scattered grids the row that left, a row that
    stays and a row 60 units away are grid rows."""
    _run_grid(mods, name)


def test_rank1_remove_deferred(mods):
    """``out2 == NULL``: nothing comes back; the next set pass returns max l0[S]."""
    _run_grid(mods, "g3_one_d3_n200", defer=True)


def test_rank1_remove_streak(mods):
    """A sliding window: the oldest of 40 rows leaves, 8 times in a row, two GPs with one
    factor; every refresh, the 8th included, within the bounds of a single one."""
    _run_grid(mods, "streak_mat52_d2")


def test_rank1_remove_refused_without_a_removal_record(mods):
    """A fresh fit, an append, a pop and a hyper-parameter edit leave no removal record:
    ``rank1_remove`` raises and leaves mean, var, Q and S alone.  The other way round:
    ``rank1_update`` refuses the record of a removal."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    name = "g1_rbf_d1_tensor_n17"
    case, ref = R.GRID_CASES[name], R.grid_reference(name)
    spec = case["gps"][0][0]

    def fresh_fit(dev):
        return dev

    def after_append(dev):
        assert dev.remove(2) and dev.append([0.3], 0.7)
        return dev

    def after_pop(dev):
        assert dev.remove(2)
        dev.pop()
        return dev

    def after_hyper_edit(dev):
        assert dev.remove(2)
        dev.set_hyper([1.3], [[1.0]], 0.01)
        return dev

    def removal(dev):
        assert dev.remove(2)
        return dev

    for change in (fresh_fit, after_append, after_pop, after_hyper_edit, removal):
        dev = _gp(gpy, spec, ref["X"][0], ref["Y"][0])._fitted()
        grid = _hip.DeviceGrid(dev.ctx, ref["pts"], 1)
        grid.confidence([dev], ref["beta0"], ref["fmin"])
        before = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        dev = change(dev)
        refresh = grid.rank1_update if change is removal else grid.rank1_remove
        with pytest.raises(_hip.HipError):
            refresh([dev], [1], 2.0, ref["fmin"])
        after = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b), change.__name__


# ---- sharing ------------------------------------------------------------------------------
def test_different_removals_unshare(mods):
    """Two GPs with one set of inputs under ``set_share``: the same removal on both is the
    case ``shared_aa_d2`` above (the second takes the first's c(x)) and leaves them one L^-1
    bit for bit; DIFFERENT removals leave different inputs -- each then has a c(x) of its
    own, in the refresh and in the sweep after it."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case, ref = R.GRID_CASES["shared_aa_d2"], R.grid_reference("shared_aa_d2")
    spec, fmin, pts = case["gps"][0][0], ref["fmin"], ref["pts"]
    ctx = _hip.Context.default()
    old = ctx.set_share(True)
    try:
        devs = [_gp(gpy, spec, ref["X"][g], ref["Y"][g])._fitted() for g in range(2)]
        for dv in devs:
            assert dv.remove(20)
        assert_array_equal(devs[0].factor()[0], devs[1].factor()[0])

        devs = [_gp(gpy, spec, ref["X"][g], ref["Y"][g])._fitted() for g in range(2)]
        grid = _hip.DeviceGrid(ctx, pts, 2)
        grid.confidence(devs, 2.0, fmin)
        rows = (20, 33)
        mean, var = [], []
        for g in range(2):
            assert devs[g].remove(rows[g])
            keep = np.arange(len(ref["X"][g])) != rows[g]
            m, v = R.RefGP(spec, ref["X"][g][keep], ref["Y"][g][keep]).predict(pts)
            mean.append(R.f64(m))
            var.append(R.clip_var(v))
        beta = 2.5
        lo = np.array(mean) - beta * np.sqrt(var)
        up = np.array(mean) + beta * np.sqrt(var)
        exp = {"mean": mean, "var": var,
               "Q": np.stack([lo, up], axis=2).transpose(1, 0, 2).reshape(-1, 4),
               "S": np.all(lo > fmin[:, None], axis=0),
               "excluded": np.any(np.abs(lo - fmin[:, None]) < R.S_EXCLUDE, axis=0)}
        grid.rank1_remove(devs, [1, 1], beta, fmin)
        _compare_grid(grid, 2, exp, fmin, ref["kdiag"], None, "different removals: refresh")
        grid.confidence(devs, beta, fmin)
        _compare_grid(grid, 2, exp, fmin, ref["kdiag"], None, "different removals: sweep")
    finally:
        ctx.set_share(old)


# ---- end to end ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "large_grid"])
def test_safeopt_forgets_a_measurement(mods, path):
    """The 1-d problem of the golden BO-loop replay on its 1000-point grid: ten iterations,
    ``remove_data_point(3)``, ``optimize()`` -- the same x, S, M, G as a twin built from the
    reduced data with ``set_XY``, Q within 1e-8.  ``large_grid``: the one-launch step of small
    grids is switched off, so the posterior behind the removal comes from the refresh."""
    safeopt_amd, gpy, _, _ = mods
    z, meta = load("safeopt_1d_rbf")

    def f(x):
        return 1.0 + 0.5 * np.sin(1.3 * np.atleast_2d(x))

    def make():
        opt = build_opt(mods, z, meta, 0)
        if path == "large_grid":
            opt._backend.SMALL_STEP_BUDGET = 0
        return opt

    opt = make()
    for _ in range(10):
        x = opt.optimize()
        opt.add_new_data_point(x, f(x))
    opt.optimize()                                   # the posterior of all 11 is resident
    t = opt.t
    opt.remove_data_point(3)
    assert opt.t == t - 1 and opt.gp._dev.removed and opt.gp._dev.n == t - 1
    streak = opt._backend._rank1_streak
    x = opt.optimize()
    if path == "large_grid":
        assert opt._backend._rank1_streak == streak + 1          # a refresh, not a sweep

    twin = make()
    twin.gp.set_XY(opt.gp.X.copy(), opt.gp.Y.copy())
    twin._x, twin._y = opt.x.copy(), opt.y.copy()
    assert not twin.gp._dev.removed and twin.t == opt.t
    xt = twin.optimize()
    assert_array_equal(x, xt)
    for a, b in ((opt.S, twin.S), (opt.M, twin.M), (opt.G, twin.G)):
        assert_array_equal(a, b)
    print("Q: %.2e" % np.max(np.abs(opt.Q - twin.Q)))
    assert np.max(np.abs(opt.Q - twin.Q)) < Q_TOL
