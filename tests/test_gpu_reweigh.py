"""GPU parity of per-observation noise scales -- the scaled fits (``sgp_gp_set_data_w``,
``sgp_gp_append_w``, ``sgp_gp_append_block_w`` and what ``sgp_gp_remove`` / ``sgp_gp_pop`` /
``sgp_gp_clone`` carry along), the re-weighting of one observation in place (``sgp_gp_reweigh``,
factor.hip) and the refresh of the resident posterior behind it (``sgp_grid_rank1_reweigh``,
k_rank1<.., kRank1Reweigh>, expander.hip) -- against long-double refits of the same data
(tests/_reweigh_ref.py), through the C ABI and through SafeOpt.

Tolerances: the project's, as tests/test_gpu_incremental.py and tests/test_gpu_remove.py have
them -- 1e-8 on L^-1 (absolute), alpha (relative to max |alpha|) and Q, ``check_posterior``
(1e-9, 1e-5 relative) on mean and variance, equality of S outside the rows within 1e-8 of fmin.
What a float64 statement of the formulas gives is in tests/test_reweigh_cpu.py: 4e-13."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _reweigh_ref as R
from _gpu_common import mods, check_posterior, smooth  # noqa: F401

pytestmark = pytest.mark.gpu

LINV_TOL = ALPHA_TOL = Q_TOL = 1e-8


def _gp(gpy, spec, X, Y, r=None):
    return gpy.models.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpy.kern, spec),
                                   noise_var=R.NOISE, noise_scale=r)


def _check_snapshot(dev, snap, Xs, kd, what):
    """alpha, L^-1, the scales and the posterior at Xs against the refit."""
    assert dev.n == snap["n"], what
    Linv, alpha = dev.factor()
    ea = np.max(np.abs(alpha - snap["alpha"])) / np.max(np.abs(snap["alpha"]))
    el = np.max(np.abs(Linv - snap["Linv"]))
    m, v = dev.predict(Xs)
    m, v = m[:, 0], v[:, 0]
    em = np.max(np.abs(m - snap["mean"])) / max(np.max(np.abs(snap["mean"])), 1e-300)
    ev = np.max(np.abs(v - snap["var"])) / kd
    print("%s: alpha %.2e  L^-1 %.2e  mean %.2e  var %.2e" % (what, ea, el, em, ev))
    assert_array_equal(dev.noise_scale(), snap["r"], what)
    assert np.all(Linv[np.triu_indices(dev.n, 1)] == 0.0), what
    assert np.all(np.diag(Linv) > 0.0), what
    assert ea < ALPHA_TOL, what
    assert el < LINV_TOL, what
    check_posterior(m, v, snap["mean"], snap["var"], kd)


# ---- scaled fits ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FIT_CASES))
def test_scaled_chain_against_long_double(mods, name):
    """set_data_w -> append_w -> append_block_w -> remove -> pop with scales from 1/16 .. 4:
    the refit of the same data after every call; then a clone has the same bits and scales."""
    _, gpy, _, _ = mods
    spec, d, n = R.FIT_CASES[name]
    X, Y, r, Xs, E, YE, rE, snaps = R.fit_reference(name)
    kd = R.kdiag(spec)
    dev = _gp(gpy, spec, X, Y, r)._fitted()
    for (what, row), snap in zip(R.fit_script(n), snaps):
        if what == "append":
            assert dev.append(E[0], YE[0], rE[0]) and dev.appended
        elif what == "block":
            assert dev.append_block(E[1:], YE[1:], rE[1:]) and dev.block == R.FIT_BLOCK
        elif what == "remove":
            assert dev.remove(row) and dev.removed
        elif what == "pop":
            dev.pop()
        assert not dev.reweighed
        _check_snapshot(dev, snap, Xs, kd, "%s after %s" % (name, what))
    twin = dev.clone()
    try:
        for a, b in zip(dev.factor() + dev.predict(Xs) + (dev.noise_scale(),),
                        twin.factor() + twin.predict(Xs) + (twin.noise_scale(),)):
            assert_array_equal(a, b)
        # the clone's scales are its own
        assert twin.append(E[0], YE[0], 0.5)
        assert_array_equal(twin.noise_scale(), np.append(snaps[-1]["r"], 0.5))
        assert_array_equal(dev.noise_scale(), snaps[-1]["r"])
    finally:
        twin.destroy()


@pytest.mark.parametrize("name", ["rbf_d1_n33", "mat52_d2_n130", "prodctx_d3_n300"])
def test_no_scales_equal_ones_bit_for_bit(mods, name):
    """``noise_scale=None`` against ``np.ones(n)``: fit, append, block append, removal and
    re-weighting give the same factor and the same predictions, bit for bit."""
    _, gpy, _, _ = mods
    spec, d, n = R.FIT_CASES[name]
    X, Y, _, Xs, E, YE, _, _ = R.fit_reference(name)
    a = _gp(gpy, spec, X, Y)._fitted()
    b = _gp(gpy, spec, X, Y, np.ones(n))._fitted()

    def same(what):
        for u, v in zip(a.factor() + a.predict(Xs), b.factor() + b.predict(Xs)):
            assert_array_equal(u, v, what)

    same("fit")
    assert a.append(E[0], YE[0]) and b.append(E[0], YE[0], 1.0)
    same("append")
    assert a.append_block(E[1:], YE[1:]) and b.append_block(E[1:], YE[1:], np.ones(len(E) - 1))
    same("block")
    assert a.remove(n // 2) and b.remove(n // 2)
    same("remove")
    assert a.reweigh(3, 0.25, 0.5) and b.reweigh(3, 0.25, 0.5)
    same("reweigh")
    assert_array_equal(a.noise_scale(), b.noise_scale())


def test_scaled_refusals(mods):
    """A scale that is not finite or not positive is refused with nothing written."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    spec = R.single("RBF", 1)
    X = np.array([[0.0], [1.0], [2.5]])
    dev = _gp(gpy, spec, X, np.array([0.1, 0.2, 0.3]), [1.0, 0.5, 2.0])._fitted()
    before = dev.factor() + (dev.noise_scale(),)
    lib, C = _hip.lib(), _hip.C
    info, jit = C.c_int(0), C.c_double(0)
    x, y = np.array([0.7]), np.array([0.1])
    for bad in (0.0, -1.0, np.nan, np.inf):
        r = np.array([bad])
        with pytest.raises(ValueError):
            dev.append(x, 0.1, bad)
        assert lib.sgp_gp_append_w(dev.h, _hip.dptr(x), 0.1, _hip.dptr(r), C.byref(info)) != 0
        assert lib.sgp_gp_append_block_w(dev.h, _hip.dptr(x), _hip.dptr(y), _hip.dptr(r), 1,
                                         C.byref(info)) != 0
        assert lib.sgp_gp_reweigh(dev.h, 1, 0.3, bad, C.byref(info)) != 0
    for index in (-1, 3, 2 ** 40):
        assert lib.sgp_gp_reweigh(dev.h, index, 0.3, 1.0, C.byref(info)) != 0
        with pytest.raises(IndexError):
            dev.reweigh(index, 0.3, 1.0)
    for bad in (np.nan, np.inf):
        assert lib.sgp_gp_reweigh(dev.h, 1, bad, 1.0, C.byref(info)) != 0
        with pytest.raises(ValueError):
            dev.reweigh(1, bad, 1.0)
    assert dev.n == 3 and not dev.reweighed and not dev.appended
    for a, b in zip(before, dev.factor() + (dev.noise_scale(),)):
        assert_array_equal(a, b)


# ---- reweigh --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.REWEIGH_CASES))
def test_reweigh_against_long_double(mods, name):
    """i first / middle / last at n = 2 .. 300, less and more noise, scale only, value only:
    L^-1, alpha and the posterior at 200 rows against the refit; the flags; the same call from
    the same state gives the same bits."""
    _, gpy, _, _ = mods
    spec = R.REWEIGH_CASES[name][0]
    X, Y, r, Xs, i, y_new, r_new, before, after = R.reweigh_reference(name)
    kd = R.kdiag(spec)
    out = []
    for _ in range(2):
        dev = _gp(gpy, spec, X, Y, r)._fitted()
        v0 = dev.version
        assert dev.reweigh(i, y_new, r_new), "reweigh refused"
        assert dev.reweighed and not dev.appended and not dev.removed and not dev.block
        assert dev.version == v0 + 1 and dev.n == len(Y)
        out.append(dev.factor() + dev.predict(Xs))
    _check_snapshot(dev, after, Xs, kd, name)
    for a, b in zip(*out):
        assert_array_equal(a, b)


def test_reweigh_chain(mods):
    """reweigh -> append -> reweigh (the appended row) -> remove -> pop: the refit after every
    call, exactly one of the flags after a one-row change."""
    _, gpy, _, _ = mods
    X, Y, r, Xs, E, YE, snaps = R.chain_reference()
    dev = _gp(gpy, R.CHAIN_SPEC, X, Y, r)._fitted()
    for (what, row, scale, dy), snap in zip(R.CHAIN, snaps):
        if what == "reweigh":
            assert dev.reweigh(row, snap["Y"][row], scale)
            assert dev.reweighed and not dev.appended and not dev.removed
        elif what == "append":
            assert dev.append(E[0], YE[0], scale) and dev.appended and not dev.reweighed
        elif what == "remove":
            assert dev.remove(row) and dev.removed and not dev.reweighed
        else:
            dev.pop()
            assert not (dev.appended or dev.removed or dev.reweighed)
        _check_snapshot(dev, snap, Xs, R.kdiag(R.CHAIN_SPEC), "chain after %s" % what)


def test_reweigh_on_a_clone_leaves_the_source(mods):
    _, gpy, _, _ = mods
    name = sorted(n for n, c in R.REWEIGH_CASES.items() if c[2] == 130)[0]
    spec = R.REWEIGH_CASES[name][0]
    X, Y, r, Xs, i, y_new, r_new, _, after = R.reweigh_reference(name)
    src = _gp(gpy, spec, X, Y, r)._fitted()
    before = src.factor() + src.predict(Xs) + (src.noise_scale(),)
    twin = src.clone()
    try:
        assert not twin.reweighed and twin.reweigh(i, y_new, r_new) and twin.reweighed
        _check_snapshot(twin, after, Xs, R.kdiag(spec), "clone")
        assert not src.reweighed
        for a, b in zip(before, src.factor() + src.predict(Xs) + (src.noise_scale(),)):
            assert_array_equal(a, b)
    finally:
        twin.destroy()


def test_model_reweigh_and_likelihood(mods):
    """``GPRegression.reweigh_data``: the model's arrays follow, and the likelihood -- a fresh
    factorisation of the resident data with their scales -- is the long-double one; its noise
    slot is the central difference of the long-double likelihood in ``noise_var``."""
    _, gpy, _, _ = mods
    name = sorted(n for n, c in R.REWEIGH_CASES.items() if c[2] == 65)[0]
    spec = R.REWEIGH_CASES[name][0]
    X, Y, r, Xs, i, y_new, r_new, _, after = R.reweigh_reference(name)
    gp = _gp(gpy, spec, X, Y, r)
    gp.reweigh_data(i, y=y_new, noise_scale=r_new)
    assert gp._dev.reweighed and gp.Y[i, 0] == y_new
    assert_array_equal(gp.noise_scale, after["r"])
    _check_snapshot(gp._fitted(), after, Xs, R.kdiag(spec), "model")
    want = float(R.ScaledGP(spec, after["X"], after["Y"], after["r"]).log_likelihood())
    got = gp.log_likelihood()
    print("log likelihood %.12g, long double %.12g" % (got, want))
    assert abs(got - want) < 1e-8 * max(abs(want), 1.0)
    h = 1e-6
    up = R.ScaledGP(spec, after["X"], after["Y"], after["r"], noise=R.NOISE + h)
    dn = R.ScaledGP(spec, after["X"], after["Y"], after["r"], noise=R.NOISE - h)
    fd = float((up.log_likelihood() - dn.log_likelihood()) / (2 * R.LD(h)))
    desc = gp.kern._desc(gp.input_dim)
    g_noise = gp._evaluate(desc[2], desc[3], gp.noise_var)[1]
    gp._settle()
    print("d/dnoise_var %.10g, central difference %.10g" % (g_noise, fd))
    assert abs(g_noise - fd) < 1e-6 * max(abs(fd), 1.0)


# ---- the grid -------------------------------------------------------------------------------
#: name -> (d, N, [(spec, data key, n, reweigh (row, scale) or None)], share, context column)
_M2 = R.single("Matern52", 2)
GRID_CASES = {
    "g3_mixed_d3_N197": (3, 197, [(R.single("RBF", 3), "a", 100, (50, 1 / 8)),
                                  (R.single("Matern52", 3), "b", 20, None),
                                  (R.PROD3, "c", 300, (299, 4.0))], None, None),
    "shared_pair_d2_N64": (2, 64, [(_M2, "a", 20, (0, 0.25)), (_M2, "a", 20, (0, 0.25))], True, None),
    "ctx_prod_d3_N1000": (3, 1000, [(R.PROD_CTX, "a", 300, (150, 1 / 16)),
                                    (R.PROD_CTX, "a", 100, (99, 2.0))], None, 0.4),
    "tiny_rbf_d1_N1000": (1, 1000, [(R.single("RBF", 1), "a", 20, (7, 4.0))], None, None),
}


def _grid_problem(mods, name):
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    d, N, gps, share, ctx_col = GRID_CASES[name]
    rng = np.random.default_rng(R.I._seed(name))
    dp = d - (1 if ctx_col is not None else 0)

    def with_ctx(a, value):
        return a if ctx_col is None else np.hstack([a, np.full((a.shape[0], 1), value)])

    Xd = {}
    for _, key, n, _ in gps:
        if key not in Xd or Xd[key].shape[0] < n:
            Xd[key] = with_ctx(np.random.default_rng(R.I._seed(name + key)).uniform(-2, 2, (n, dp)),
                               ctx_col)
    rs = rng.choice(R.SCALES, size=max(g[2] for g in gps))
    models = []
    for g, (spec, key, n, _) in enumerate(gps):
        X = Xd[key][:n]
        models.append(_gp(gpy, spec, X, smooth(X, 11 + g)[:, 0] + 0.3, rs[:n]))
    devs = [m._fitted() for m in models]
    pts = with_ctx(rng.uniform(-3, 3, size=(N, dp)), 9.0)
    pts[N // 2, :dp] = Xd[gps[0][1]][gps[0][3][0], :dp]        # the re-weighted row itself
    pts[1, :dp] = 60.0                                          # the covariance underflows
    grid = _hip.DeviceGrid(devs[0].ctx, pts, len(gps))
    if ctx_col is not None:
        grid.set_context([ctx_col])
    return models, devs, grid, share


def _download(grid):
    from safeopt_amd import _hip
    return [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]


@pytest.mark.parametrize("name", sorted(GRID_CASES))
def test_rank1_reweigh_against_the_sweep(mods, name):
    """N = 64, 197 and 1000; three GPs with mixed ``which``; a pair that shares a factor; a
    context column; n = 20, 100 and 300: ``rank1_reweigh`` after one ``reweigh`` on the flagged
    GPs against a full ``confidence`` sweep of the same GPs -- mean, var, Q within tolerance, S
    equal outside the rows within 1e-8 of fmin, the returned maximum."""
    models, devs, grid, share = _grid_problem(mods, name)
    gps = GRID_CASES[name][2]
    G = len(gps)
    ctx = devs[0].ctx
    old = ctx.set_share(share) if share is not None else None
    try:
        grid.confidence(devs, 2.0, np.full(G, -np.inf))
        before = _download(grid)
        lo = before[2][:, 0::2]
        fmin = np.array([np.quantile(lo[:, g], 0.3) for g in range(G)])
        which = [int(c[3] is not None) for c in gps]
        for g, c in enumerate(gps):
            if which[g]:
                row, scale = c[3]
                y_new = models[g].Y[row, 0] + (0.4 if g % 2 == 0 else 0.0)
                assert devs[g].reweigh(row, y_new, scale)
        beta = 2.5
        ret = grid.rank1_reweigh(devs, which, beta, fmin)
        mean, var, Q, S = _download(grid)
        ret_s = grid.confidence(devs, beta, fmin)
        mean_s, var_s, Q_s, S_s = _download(grid)
    finally:
        if old is not None:
            ctx.set_share(old)
    for g in range(G):
        kd = R.kdiag(gps[g][0])
        em = np.max(np.abs(mean[g] - mean_s[g])) / np.max(np.abs(mean_s[g]))
        ev = np.max(np.abs(var[g] - var_s[g])) / kd
        print("%s GP %d: mean %.2e  var %.2e  Q %.2e" % (
            name, g, em, ev, np.max(np.abs(Q[:, 2 * g:2 * g + 2] - Q_s[:, 2 * g:2 * g + 2]))))
    for g in range(G):
        check_posterior(mean[g], var[g], mean_s[g], var_s[g], R.kdiag(gps[g][0]))
    assert np.max(np.abs(Q - Q_s)) < Q_TOL
    keep = ~np.any(np.abs(Q_s[:, 0::2] - fmin[None, :]) < R.S_EXCLUDE, axis=1)
    assert keep.sum() > 0.9 * len(keep)
    assert_array_equal(S[keep], S_s[keep])
    assert 0 < S_s.sum() < len(S_s)
    assert ret[1] == ret_s[1] and abs(ret[0] - ret_s[0]) < Q_TOL
    # the refresh moved GP 0 (its re-weighted row is a grid row) and no GP that is not flagged
    for g in range(G):
        moved = np.max(np.abs(mean[g] - before[0][g])) + np.max(np.abs(var[g] - before[1][g]))
        assert moved > 1e-6 if g == 0 else (which[g] or moved == 0.0), (g, moved)


def test_each_refresh_refuses_the_other_records(mods):
    """After a reweigh ``rank1_update`` and ``rank1_remove`` raise; after an append, a removal,
    a pop or a fresh fit ``rank1_reweigh`` raises; mean, var, Q and S stay as they were."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    spec = R.single("RBF", 1)
    X = np.linspace(-2, 2, 17)[:, None]
    Y = smooth(X, 3)[:, 0]
    pts = np.linspace(-3, 3, 197)[:, None]
    fmin = np.array([-0.2])

    def reweighed(dev):
        assert dev.reweigh(2, 0.3, 0.5)
        return dev, ("rank1_update", "rank1_remove")

    def appended(dev):
        assert dev.reweigh(2, 0.3, 0.5) and dev.append([0.3], 0.7)
        return dev, ("rank1_reweigh", "rank1_remove")

    def removed(dev):
        assert dev.reweigh(2, 0.3, 0.5) and dev.remove(4)
        return dev, ("rank1_reweigh", "rank1_update")

    def popped(dev):
        assert dev.reweigh(2, 0.3, 0.5)
        dev.pop()
        return dev, ("rank1_reweigh",)

    def fresh(dev):
        return dev, ("rank1_reweigh",)

    for change in (reweighed, appended, removed, popped, fresh):
        dev = _gp(gpy, spec, X, Y)._fitted()
        grid = _hip.DeviceGrid(dev.ctx, pts, 1)
        grid.confidence([dev], 2.0, fmin)
        before = _download(grid)
        dev, refused = change(dev)
        for refresh in refused:
            with pytest.raises(_hip.HipError):
                getattr(grid, refresh)([dev], [1], 2.0, fmin)
        for a, b in zip(before, _download(grid)):
            assert_array_equal(a, b, change.__name__)


def test_different_reweighs_unshare(mods):
    """Two GPs with one set of inputs under ``set_share``: the same re-weighting on both leaves
    them one L^-1 bit for bit (and sharing); different scales give each its own factor, in the
    refresh and in the sweep after it."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    rng = np.random.default_rng(5)
    X = rng.uniform(-2, 2, (40, 2))
    Ys = [smooth(X, 11 + g)[:, 0] + 0.3 for g in range(2)]
    pts = rng.uniform(-3, 3, (197, 2))
    fmin = np.array([-0.1, -0.1])
    ctx = _hip.Context.default()
    old = ctx.set_share(True)
    try:
        devs = [_gp(gpy, _M2, X, Ys[g])._fitted() for g in range(2)]
        for dv in devs:
            assert dv.reweigh(20, 0.5, 0.25)
        assert_array_equal(devs[0].factor()[0], devs[1].factor()[0])

        devs = [_gp(gpy, _M2, X, Ys[g])._fitted() for g in range(2)]
        grid = _hip.DeviceGrid(ctx, pts, 2)
        grid.confidence(devs, 2.0, fmin)
        scales = (0.25, 4.0)
        exp = []
        for g in range(2):
            assert devs[g].reweigh(20, Ys[g][20], scales[g])
            r = np.ones(40)
            r[20] = scales[g]
            m, v = R.ScaledGP(_M2, X, Ys[g], r).predict(pts)
            exp.append((R.f64(m), R.clip_var(v)))
        for what in ("refresh", "sweep"):
            if what == "refresh":
                grid.rank1_reweigh(devs, [1, 1], 2.5, fmin)
            else:
                grid.confidence(devs, 2.5, fmin)
            mean, var = grid.download(_hip.MEAN), grid.download(_hip.VAR)
            for g in range(2):
                check_posterior(mean[g], var[g], exp[g][0], exp[g][1], R.kdiag(_M2))
    finally:
        ctx.set_share(old)


def test_confidence_takes_the_refresh_for_one_reweigh(mods):
    """``SafeOpt``: one ``reweigh_data`` behind the resident posterior is absorbed by the
    refresh (``last_sweep`` unchanged, the streak counts it); a reweigh on one GP and an append
    on the other is a sweep.  Both give the intervals of a twin fitted to the same data."""
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd import _hip
    rng = np.random.default_rng(9)
    X = rng.uniform(-2, 2, (30, 2))
    grid = safeopt_amd.linearly_spaced_combinations([(-3., 3.)] * 2, 40)

    def make(Ys, rs):
        gps = [_gp(gpy, _M2, X, Ys[g], rs[g]) for g in range(2)]
        opt = safeopt_amd.SafeOpt(gps, grid, [-0.5, -0.5], threshold=0.0)
        opt._backend.SMALL_STEP_BUDGET = 0
        return opt

    Ys = [smooth(X, 11 + g)[:, 0] + 0.3 for g in range(2)]
    opt = make(Ys, [None, None])
    opt.update_confidence_intervals()
    ctx = _hip.Context.default()
    opt.gps[0].reweigh_data(5, noise_scale=1 / 8)
    marker = ctx.last_sweep()
    streak = opt._backend._rank1_streak
    opt.update_confidence_intervals()
    assert opt._backend._rank1_streak == streak + 1 and ctx.last_sweep() == marker
    r0 = np.ones(30)
    r0[5] = 1 / 8
    twin = make(Ys, [r0, None])
    twin.update_confidence_intervals()
    print("refresh: Q %.2e" % np.max(np.abs(opt.Q - twin.Q)))
    assert np.max(np.abs(opt.Q - twin.Q)) < Q_TOL

    opt.gps[0].reweigh_data(6, y=Ys[0][6] + 0.2)
    opt.gps[1].set_XY(np.vstack([X, [[0.1, 0.2]]]), np.vstack([Ys[1][:, None], [[0.4]]]))
    opt.update_confidence_intervals()
    assert opt._backend._rank1_streak == 0                      # a mix of kinds: a sweep
