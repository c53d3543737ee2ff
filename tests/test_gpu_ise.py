"""Information-theoretic safe exploration on the device (csrc/ise.hip; needs an MI355X):
``sgp_ise_eval``, ``sgp_grid_ise`` and ``SafeOpt.ise_point`` / ``info_point`` against
tests/_ise_ref.py -- the closed form at 80 digits, its float64 restatement, a long-double GP.

Tolerance of a term, per point, in the unit ``u = EPS (1 + t) sqrt(kappa) ln2 e^-t``
(tests/_ise_ref.py): the restatement's own maximum over the points is measured against mpmath IN
the test, and the device is allowed 4 times that -- the factor and its reason are
tests/test_gpu_mes.py's: the device's exp / expm1 / log1p are a few ulp each where NumPy's are at
most one; the factor covers three such calls and the divisions.  Both maxima are printed, and
appended to the file ``SAFEOPT_ISE_PARITY_OUT`` names when it is set (profiles/ise/parity.txt
was taken that way).  The covariances stay within the project's ``VAR_TOL kdiag`` of the
long-double GP.  Everything else is equality: pairs against ``sgp_ise_eval`` on the device's own
downloaded inputs, the reductions against the host's over those pairs, bits of a candidate
against the same candidate elsewhere.

The grid cases straddle tile and padding edges (64 rows, 64 candidates, 16 and 64 training
rows), not workload size.  The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _incremental_ref as R
import _ise_ref as ref
import _mes_problems as P
from _gpu_common import VAR_TOL, build_opt, mods, smooth                    # noqa: F401

pytestmark = pytest.mark.gpu

FACTOR = 4.0


@pytest.fixture(scope="module")
def ctx(hip_device):
    from safeopt_amd import _hip
    return _hip.Context.default()


def _record(line):
    print(line)
    out = os.environ.get("SAFEOPT_ISE_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


# ---- 1. term by term ---------------------------------------------------------------------------

def _eval_by_s(ctx, mu, vz, vx, c, s):
    """``sgp_ise_eval`` takes one s per call: the points grouped by launch."""
    return np.array([ctx.ise_eval(mu[i:i + 1], vz[i:i + 1], vx[i:i + 1], c[i:i + 1], s[i])[0]
                     for i in range(mu.size)])


def test_term_against_mpmath(ctx):
    mu, vz, vx, c, s = ref.point_set()
    exact, unit, host_u = ref.point_reference()
    got = _eval_by_s(ctx, mu, vz, vx, c, s)
    dev_u = ref.units(got, exact, unit)
    _record("%d points, t in [0, 650], 1 - |rho| down to 1e-12; max error in units of EPS (1 + t) "
            "sqrt(kappa) ln2 e^-t: host restatement %.3f, device %.3f (allowed %.3f)"
            % (mu.size, host_u.max(), dev_u.max(), FACTOR * host_u.max()))
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    assert dev_u.max() <= FACTOR * host_u.max()


def test_term_at_the_corners(ctx):
    big = np.sqrt(800.0 / ref.C1)                                  # t = 800 at vz = 1
    #            mu   vz     vx     c      s
    corners = [(0.3, 1.0, 1.0, 1.5, 0.1),                          # r2 > 1
               (0.3, 1.0, 1.0, 1.0, 0.0),                          # s = 0, r2 = 1
               (0.3, 1.0, 1.0, -1.0 - 1e-12, 0.0),
               (0.0, 1e-30, 1e-30, 1e-15, 1e-3),                   # variances below the clip
               (1e-9, 1e-30, 2.0, 1e-9, 0.0),
               (big, 1.0, 1.0, 0.7, 0.1),                          # t > 745: e^-t = 0
               (-big, 1.0, 1.0, 1.0, 0.0),
               (0.3, 1.0, 1.0, 0.0, 0.1),                          # c = 0
               (0.3, 1.0, 1.0, -0.0, 0.0)]
    mu, vz, vx, c, s = (np.array(a) for a in zip(*corners))
    got = _eval_by_s(ctx, mu, vz, vx, c, s)
    # (the bound ln2 e^-t with NumPy's exponential: the device's may differ from it by a few ulp)
    cap = ref.LN2 * np.exp(-ref.C1 * mu * mu / np.maximum(vz, 1e-15))
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    assert np.all(got <= cap * (1.0 + 4 * ref.EPS))
    assert np.all(np.abs(got[[1, 2]] - cap[[1, 2]]) <= 4 * ref.EPS * cap[[1, 2]])   # the whole entropy
    assert_array_equal(got[[5, 6, 7, 8]], np.zeros(4))


NS = (1, 63, 64, 65, 255, 256, 257, 1000)


def test_rows_do_not_depend_on_launch(ctx):
    mu, vz, vx, c, _ = (a[:1000] for a in ref.point_set())
    s = 0.0025
    full = ctx.ise_eval(mu, vz, vx, c, s)
    rng = np.random.default_rng(5)
    for N in NS:
        assert_array_equal(ctx.ise_eval(mu[:N], vz[:N], vx[:N], c[:N], s), full[:N])
        p = rng.permutation(1000)[:N]
        assert_array_equal(ctx.ise_eval(mu[p], vz[p], vx[p], c[p], s), full[p])


@pytest.mark.parametrize("s", [float("nan"), -1e-3, -np.inf])
def test_bad_noise_is_refused_with_nothing_written(ctx, s):
    from safeopt_amd import _hip
    a = np.ones(5)
    out = np.full(5, -7.0)
    d = _hip.dptr
    rc = _hip.lib().sgp_ise_eval(ctx.h, d(a), d(a), d(a), d(a), 5, s, d(out))
    assert rc != 0 and np.all(out == -7.0)
    with pytest.raises(_hip.HipError):
        ctx.ise_eval(a, a, a, a, s)
    # N = 0: nothing to do, nothing written
    assert _hip.lib().sgp_ise_eval(ctx.h, d(a), d(a), d(a), d(a), 0, 0.1, d(out)) == 0
    assert np.all(out == -7.0)


# ---- 2. the grid -------------------------------------------------------------------------------

def _plane(n_side, lim=2.0):
    ax = np.linspace(-lim, lim, n_side)
    return np.array([[a, b] for a in ax for b in ax])


def _case(name):
    """``(gps = [(spec, n)], pts (N, d), fmin, K, safe rows or None)``"""
    rng = np.random.default_rng(R._seed("ise_" + name))
    if name == "a":
        return [(R.single("RBF", 1), 5)], np.linspace(-3.0, 3.0, 1000)[:, None], [0.1], 1, None
    if name in ("b48", "b49"):
        return [(R.single("Matern52", 2), int(name[1:]))], _plane(70), [0.0], 17, None
    if name == "c":
        return [(R.single("Matern32", 3), 130)], rng.uniform(-2.5, 2.5, (1000, 3)), [-0.2], 64, None
    if name == "d":
        spec = R.single("RBF", 2)
        return ([(spec, 257), (spec, 40), (spec, 130)], rng.uniform(-2.5, 2.5, (1000, 2)),
                [0.2, -np.inf, -0.3], 65, None)
    if name == "e":
        p = _plane(30)
        return ([(R.PROD_CTX, 60)], np.hstack([p, np.full((900, 1), 0.4)]), [0.0], 16, None)
    if name == "f":
        return [(R.single("Matern52", 2), 1)], _plane(20), [-0.5], 3, np.array([7, 200, 399])
    raise KeyError(name)


CASES = ("a", "b48", "b49", "c", "d", "e", "f")


@functools.lru_cache(maxsize=None)
def _case_data(name):
    """The data of a case and its long-double covariances, once: ``X``, ``Y`` per GP, ``cand``,
    ``S`` and ``cov`` (G, K, N) (zeros for an inactive GP)."""
    gps, pts, fmin, K, safe = _case(name)
    rng = np.random.default_rng(R._seed("ise_data_" + name))
    d = pts.shape[1]
    X, Y = [], []
    for g, (_spec, n) in enumerate(gps):
        x = rng.uniform(-2.0, 2.0, (n, d))
        if name == "e":
            x[:, 2] = rng.choice([0.0, 0.4, 0.8], n)
        X.append(x)
        Y.append(smooth(x, 31 + g)[:, 0])
    N = pts.shape[0]
    if safe is None:
        # a "safe" region around the data of GP 0, cut so that both sides are populated
        dist = np.min(((pts[:, None, :] - X[0][None, :, :]) ** 2).sum(-1), axis=1)
        S = dist <= np.quantile(dist, 0.3)
        cand = np.sort(rng.choice(np.flatnonzero(S), size=K, replace=False))
        rng.shuffle(cand)
    else:
        S = np.zeros(N, dtype=bool)
        S[safe] = True
        cand = safe.copy()
    cov = np.zeros((len(gps), K, N))
    for g, (spec, _n) in enumerate(gps):
        if np.isfinite(fmin[g]):
            cov[g] = np.asarray(ref.ref_cov(R.RefGP(spec, X[g], Y[g]), pts, pts[cand]).T,
                                dtype=np.float64)
    return X, Y, cand.astype(np.int64), S, cov


def _device_case(mods, ctx, name):
    from safeopt_amd import _hip
    _, gpy, _, _ = mods
    gps, pts, fmin, K, _ = _case(name)
    X, Y, cand, S, cov = _case_data(name)
    models = [gpy.models.GPRegression(X[g], Y[g][:, None], R.make_kernel(gpy.kern, spec),
                                      noise_var=R.NOISE) for g, (spec, _n) in enumerate(gps)]
    devs = [m._fitted() for m in models]
    grid = _hip.DeviceGrid(ctx, pts, len(devs))
    grid.posterior(devs)
    grid.upload_mask(_hip.S, S)
    return models, devs, grid, np.array(fmin, dtype=float), cand, S, cov


def _host_pairs(ctx, grid, fmin, cand, cov):
    """The in-order sum over the active GPs of ``sgp_ise_eval`` on what the device holds."""
    from safeopt_amd import _hip
    mean, var = np.array(grid.download(_hip.MEAN)), np.array(grid.download(_hip.VAR))
    K, N = cand.size, mean.shape[1]
    out = np.zeros((K, N))
    for g in range(fmin.size):
        if np.isfinite(fmin[g]):
            out = out + ctx.ise_eval(np.broadcast_to(mean[g] - fmin[g], (K, N)),
                                     np.broadcast_to(var[g], (K, N)),
                                     np.broadcast_to(var[g][cand][:, None], (K, N)), cov[g],
                                     R.NOISE + 1e-8)
    return out


@pytest.mark.parametrize("name", CASES)
def test_grid_case(mods, ctx, name):
    from safeopt_amd import _hip
    _models, devs, grid, fmin, cand, S, cov_ref = _device_case(mods, ctx, name)
    specs = [g[0] for g in _case(name)[0]]
    first = None
    for about, zmask in ((_hip.ISE_UNSAFE, ~S), (_hip.ISE_ALL, np.ones(S.size, dtype=bool))):
        al, tg, v, i, pr, cv = grid.ise(devs, fmin, cand, about=about, pairs=True, cov=True)
        for g, spec in enumerate(specs):
            if not np.isfinite(fmin[g]):
                assert not cv[g].any()
                continue
            err = np.max(np.abs(cv[g] - cov_ref[g])) / R.kdiag(spec)
            print("case %s, GP %d: max |cov - long double| = %.2e kdiag" % (name, g, err))
            assert err < VAR_TOL
        assert_array_equal(pr, _host_pairs(ctx, grid, fmin, cand, cv))
        want_al, want_tg = ref.alpha(pr, zmask)
        assert_array_equal(al, want_al)
        assert_array_equal(tg, want_tg)
        assert (v, i) == ref.pick(want_al, want_tg, cand)
        assert np.all(np.isfinite(pr)) and np.all(pr >= 0.0) and v > 0.0
        if about == _hip.ISE_UNSAFE:
            assert not np.any(S[tg])
        # without the test outputs: the same results
        al2, tg2, v2, i2, pr2, cv2 = grid.ise(devs, fmin, cand, about=about)
        assert pr2 is None and cv2 is None and (v2, i2) == (v, i)
        assert_array_equal(al2, al)
        assert_array_equal(tg2, tg)
        # the rows z do not change a pair
        if first is None:
            first = pr
        assert_array_equal(pr, first)
    # S, mean and var are only read
    assert_array_equal(np.array(grid.download(_hip.S), dtype=bool), S)


def test_every_row_safe_has_no_target(mods, ctx):
    from safeopt_amd import _hip
    _m, devs, grid, fmin, cand, S, _ = _device_case(mods, ctx, "a")
    grid.upload_mask(_hip.S, np.ones(S.size, dtype=bool))
    al, tg, v, i, _, _ = grid.ise(devs, fmin, cand)
    assert np.all(al == -np.inf) and np.all(tg == -1) and (v, i) == (-np.inf, -1)
    assert grid.ise(devs, fmin, cand, about=_hip.ISE_ALL)[3] == cand[0]


def test_shard_returns_global_rows(mods, ctx):
    from safeopt_amd import _hip
    _m, devs, _grid, fmin, cand, S, _ = _device_case(mods, ctx, "c")
    lo, hi = 133, 901                                   # a shard that starts inside a tile
    pts = _case("c")[1]
    keep = cand[(cand >= lo) & (cand < hi)]
    shard = _hip.DeviceGrid(ctx, pts[lo:hi], len(devs), global_offset=lo)
    shard.posterior(devs)
    shard.upload_mask(_hip.S, S[lo:hi])
    al, tg, v, i, pr, cv = shard.ise(devs, fmin, keep, pairs=True, cov=True)
    assert_array_equal(pr, _host_pairs(ctx, shard, fmin, keep - lo, cv))
    want_al, want_tg = ref.alpha(pr, ~S[lo:hi])
    assert_array_equal(al, want_al)
    assert_array_equal(tg, want_tg + lo)
    assert (v, i) == ref.pick(want_al, want_tg, keep)


# ---- 3. position independence ------------------------------------------------------------------

def test_a_candidate_does_not_depend_on_its_position_or_on_K(mods, ctx):
    _m, devs, grid, fmin, cand, S, _ = _device_case(mods, ctx, "d")
    assert cand.size == 65
    al, tg, _, _, pr, _ = grid.ise(devs, fmin, cand, pairs=True)
    rng = np.random.default_rng(12)
    for K in (1, 16, 17, 64, 65):
        sel = rng.permutation(65)[:K]
        al2, tg2, v2, i2, pr2, _ = grid.ise(devs, fmin, cand[sel], pairs=True)
        assert_array_equal(pr2, pr[sel])
        assert_array_equal(al2, al[sel])
        assert_array_equal(tg2, tg[sel])
        assert (v2, i2) == ref.pick(al[sel], tg[sel], cand[sel])
    # duplicates are allowed: the same bits twice, the pick unchanged
    dup = np.array([cand[3], cand[9], cand[3]])
    al3, tg3, _, _, pr3, _ = grid.ise(devs, fmin, dup, pairs=True)
    assert_array_equal(pr3, pr[[3, 9, 3]])
    assert_array_equal(al3, al[[3, 9, 3]])


# ---- 4. refusals -------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(mods, ctx):
    import ctypes as C
    from safeopt_amd import _hip
    _, gpy, _, _ = mods
    _m, devs, grid, fmin, cand, S, _ = _device_case(mods, ctx, "a")
    pts = _case("a")[1]
    shard = _hip.DeviceGrid(ctx, pts[100:400], 1, global_offset=100)
    shard.posterior(devs)
    fresh = _hip.DeviceGrid(ctx, pts[:50], 1)            # no pass has swept it
    other_ctx = _hip.Context(ctx.device)
    spec = R.single("RBF", 1)
    X, Y = _case_data("a")[:2]
    k = R.make_kernel(gpy.kern, spec)
    foreign = _hip.DeviceGP(other_ctx, k._desc(1), R.NOISE)
    foreign.set_data(X[0], Y[0])
    # not fitted: an evaluation at infeasible hyper-parameters voids the factor
    Xd = np.vstack([X[0], X[0]])
    bad_gp = gpy.models.GPRegression(Xd, np.concatenate([Y[0], Y[0] + 0.01])[:, None],
                                     R.make_kernel(gpy.kern, spec), noise_var=R.NOISE)
    bad = bad_gp._fitted()
    desc = bad_gp.kern._desc(1)
    assert bad_gp._evaluate(desc[2], desc[3], -1.9e-8)[4] != 0
    two = _hip.DeviceGrid(ctx, pts[:50], 2)
    d, lib = _hip.dptr, _hip.lib()
    i64 = lambda a: a.ctypes.data_as(_hip.c_i64_p)                       # noqa: E731

    def call(g, gps, fm, cd, K, about=_hip.ISE_UNSAFE, extra=False):
        cd = np.ascontiguousarray(cd, dtype=np.int64)
        fm = np.ascontiguousarray(fm, dtype=np.float64)
        n_out = max(K, 1)
        al, tg = np.full(n_out, -7.0), np.full(n_out, -7, dtype=np.int64)
        pr, cv = np.full((n_out, g.N), -7.0), np.full((len(gps), n_out, g.N), -7.0)
        v, i = C.c_double(-7.0), C.c_int64(-7)
        rc = lib.sgp_grid_ise(g.h, _hip._gp_array(gps), len(gps), d(fm), i64(cd), K, about, d(al),
                              i64(tg), C.byref(v), C.byref(i), d(pr) if extra else None,
                              d(cv) if extra else None)
        clean = (np.all(al == -7.0) and np.all(tg == -7) and v.value == -7.0 and i.value == -7
                 and np.all(pr == -7.0) and np.all(cv == -7.0))
        return rc, clean

    try:
        refused = [
            ("K = 0", call(grid, devs, fmin, cand, 0)),
            ("K = 4097", call(grid, devs, fmin, np.zeros(4097), 4097)),
            ("about", call(grid, devs, fmin, cand, 1, about=2)),
            ("row below the shard", call(shard, devs, fmin, [99], 1)),
            ("row behind the shard", call(shard, devs, fmin, [150, 400], 2)),
            ("negative row", call(grid, devs, fmin, [-1], 1)),
            ("no active GP", call(grid, devs, [-np.inf], cand, 1)),
            ("fmin NaN only", call(grid, devs, [np.nan], cand, 1)),
            ("no posterior", call(fresh, devs, fmin, [3], 1)),
            ("another context", call(grid, [foreign], fmin, cand, 1)),
            ("not fitted", call(grid, [bad], fmin, cand, 1)),
            ("G of the grid", call(two, devs, fmin, [3], 1)),
        ]
        for what, (rc, clean) in refused:
            assert rc != 0, what
            assert clean, what
        # the wrappers raise
        with pytest.raises(_hip.HipError, match="SGP_MAX_ISE"):
            grid.ise(devs, fmin, [])
        with pytest.raises(_hip.HipError, match="outside the shard"):
            shard.ise(devs, fmin, [99])
        with pytest.raises(_hip.HipError, match="no current posterior"):
            fresh.ise(devs, fmin, [3])
        with pytest.raises(_hip.HipError, match="another context"):
            grid.ise([foreign], fmin, cand)
        with pytest.raises(_hip.HipError, match="not fitted"):
            grid.ise([bad], fmin, cand)
        # ... and the grid still answers
        rc, clean = call(grid, devs, fmin, cand, 1)
        assert rc == 0 and not clean
    finally:
        foreign.destroy()


def test_test_outputs_are_refused_above_their_bound(mods, ctx):
    """``pairs`` / ``cov`` are for tests and diagnostics: G K N_local > 2^24 is refused."""
    from safeopt_amd import _hip
    _m, devs, grid, fmin, cand, S, _ = _device_case(mods, ctx, "b48")
    rows = np.resize(np.flatnonzero(S), 4096)
    assert rows.size * S.size > 2 ** 24
    with pytest.raises(_hip.HipError, match="2\\^24"):
        grid.ise(devs, fmin, rows, pairs=True)
    # ... and without them the call goes through: the partials are bounded, not K x N
    al, tg, v, i, _, _ = grid.ise(devs, fmin, rows)
    small = grid.ise(devs, fmin, rows[:20])
    assert_array_equal(al[:20], small[0])
    assert_array_equal(tg[:20], small[1])
    assert v == al.max() and i == rows[al == v].min()


def test_new_context_columns_void_the_posterior(mods, ctx):
    from safeopt_amd import _hip
    _m, devs, grid, fmin, cand, S, _ = _device_case(mods, ctx, "e")
    assert grid.ise(devs, fmin, cand)[3] >= 0
    grid.set_context([0.25])
    with pytest.raises(_hip.HipError, match="no current posterior"):
        grid.ise(devs, fmin, cand)
    grid.posterior(devs)
    assert grid.ise(devs, fmin, cand)[3] >= 0


# ---- 5. ise_point / info_point end to end ------------------------------------------------------

def _state(opt):
    from safeopt_amd import _hip
    be = opt._backend
    out = [np.array(be.download(w)) for w in (_hip.Q, _hip.S, _hip.M, _hip.G, _hip.MEAN,
                                              _hip.VAR)]
    out.extend(np.array(a) for a in opt.gp._fitted().factor())
    out.extend([np.array(opt.x), np.array(opt.y)])
    return out


def _check_point(opt, K, about):
    """``ise_point`` against the reference selection and the reductions of the device pairs."""
    from safeopt_amd import _hip
    be = opt._backend
    x, a, rows, values, targets = opt.ise_point(candidates=K, about=about, return_values=True)
    var, S = np.array(be.download(_hip.VAR)), np.array(be.download(_hip.S), dtype=bool)
    fmin = np.asarray(opt.fmin, dtype=float)
    s = np.array([g.noise_var + 1e-8 for g in opt.gps])
    assert_array_equal(rows, ref.select(var, S, s, np.isfinite(fmin), K))
    code = _hip.ISE_UNSAFE if about == 'unsafe' else _hip.ISE_ALL
    pr = be.grid.ise(be._dev(), fmin, rows, about=code, pairs=True)[4]
    al, tg = ref.alpha(pr, ~S if about == 'unsafe' else np.ones(S.size, dtype=bool))
    assert_array_equal(values, al)
    assert_array_equal(targets, tg)
    v, i = ref.pick(al, tg, rows)
    assert a == v and S[i]
    assert_array_equal(x, opt.inputs[i, :opt.inputs.shape[1] - opt.num_contexts])
    x2, a2 = opt.ise_point(candidates=K, about=about)
    assert_array_equal(x2, x)
    assert a2 == a
    return x, a


@pytest.mark.parametrize("name", ["line", "plane"])
def test_ise_point_end_to_end(mods, name):
    z, meta = P.problem(name)
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    S = np.array(opt.S)
    assert S.any() and not S.all()
    before = _state(opt)
    rs = np.random.get_state()
    for K, about in ((40, 'unsafe'), (7, 'all')):
        _check_point(opt, K, about)
    ids = np.flatnonzero(S)[::5][:9]
    x, a, rows, values, targets = opt.ise_point(candidates=ids, return_values=True)
    assert_array_equal(rows, ids)
    assert a == values.max() and not np.any(S[targets])
    with pytest.raises(ValueError, match="outside the safe set"):
        opt.ise_point(candidates=np.flatnonzero(~S)[:2])
    for u, w in zip(before, _state(opt)):
        assert_array_equal(u, w)
    now = np.random.get_state()
    assert rs[0] == now[0] and np.array_equal(rs[1], now[1]) and rs[2:] == now[2:]
    # one more observation: the resident posterior is refreshed before it is read
    x_new = opt.inputs[np.flatnonzero(S)[0]]
    opt.add_new_data_point(x_new, 1.3)
    assert not opt._backend.posterior_is_current()
    _check_point(opt, 40, 'unsafe')
    assert opt._backend.posterior_is_current()
    assert opt.gp._fitted().n == z["it0_X0"].shape[0] + 1


@pytest.mark.parametrize("name", ["line", "plane"])
def test_info_point_takes_the_larger_acquisition(mods, name):
    z, meta = P.problem(name)
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    seed = P.SEEDS[name][0]
    np.random.seed(seed)
    xm, am = opt.mes_point(paths=P.PATHS, features=P.FEATURES)
    xi, ai = opt.ise_point(candidates=40)
    np.random.seed(seed)
    x, a, which = opt.info_point(paths=P.PATHS, features=P.FEATURES, candidates=40)
    assert which == ('ise' if ai > am else 'mes')
    assert a == max(am, ai)
    assert_array_equal(x, xi if which == 'ise' else xm)
    # every row safe: no row qualifies for ISE, the MES pick
    opt.S[:] = True
    np.random.seed(seed)
    xm2, am2 = opt.mes_point(paths=P.PATHS, features=P.FEATURES)
    np.random.seed(seed)
    x, a, which = opt.info_point(paths=P.PATHS, features=P.FEATURES, candidates=40)
    assert which == 'mes' and a == am2
    assert_array_equal(x, xm2)
    with pytest.raises(RuntimeError, match="no row qualifies"):
        opt.ise_point(candidates=40)


def test_ise_point_without_a_safe_row(mods):
    z, meta = P.problem("line")
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    opt.S[:] = False
    with pytest.raises(RuntimeError, match="no safe points"):
        opt.ise_point()
