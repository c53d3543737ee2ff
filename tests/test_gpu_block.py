"""GPU parity of the block path -- ``sgp_gp_append_block`` (factor.hip), the rank-b refresh of the
resident posterior ``sgp_grid_rankb_update`` (k_rankb, block.hip), ``GPRegression.append_XY`` and
``add_new_data_points`` -- against a long-double GP (tests/_block_ref.py on ``RefGP``).

The expected state after a block is ``RefGP.append`` applied b times.  Tolerances are the
project's: ``check_posterior`` (1e-9 relative on mean and var), 1e-8 on L^-1, alpha (relative to
max |alpha|), Q and the returned maximum; S is compared outside the rows with
``|lo - fmin| < 1e-8`` (tests/test_block_ref_cpu.py counts them: none)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _block_ref as B
import _incremental_ref as R
from _gpu_common import (  # noqa: F401
    MEAN_TOL, VAR_TOL, mods, check_posterior, _swarm_problem)

pytestmark = pytest.mark.gpu

LINV_TOL = ALPHA_TOL = Q_TOL = RET_TOL = 1e-8


def _gp(gpy, spec, X, Y):
    return gpy.models.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpy.kern, spec),
                                   noise_var=R.NOISE)


def _check_snapshot(gp, snap, Xs, kd, what):
    """alpha, L^-1 (where the reference has it), the posterior at Xs and the data against a refit."""
    dev = gp._fitted()
    assert dev.n == snap["n"], what
    Linv, alpha = dev.factor()
    ea = np.max(np.abs(alpha - snap["alpha"])) / np.max(np.abs(snap["alpha"]))
    el = np.max(np.abs(Linv - snap["Linv"])) if "Linv" in snap else 0.0
    m, v = gp.predict_noiseless(Xs)
    m, v = m[:, 0], v[:, 0]
    em = np.max(np.abs(m - snap["mean"])) / np.max(np.abs(snap["mean"]))
    ev = np.max(np.abs(v - snap["var"])) / kd
    print("%s: alpha %.2e  L^-1 %.2e  mean %.2e  var %.2e" % (what, ea, el, em, ev))
    assert ea < ALPHA_TOL, what
    assert el < LINV_TOL, what
    check_posterior(m, v, snap["mean"], snap["var"], kd)
    assert_array_equal(gp.X, snap["X"])
    assert_array_equal(gp.Y[:, 0], snap["Y"])


# ---- append_block ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.APPEND_BLOCK_CASES))
def test_append_block_against_long_double(mods, name):
    """Fit at n0, ONE ``append_XY`` of b rows (a block append): L^-1 (n <= 520), alpha, the
    posterior at 300 rows, X and Y against the long-double refit at n0 + b."""
    _, gpy, _, _ = mods
    spec, X, Y, Xs, n0, snap = B.append_block_reference(name)
    gp = _gp(gpy, spec, X[:n0], Y[:n0])
    dev = gp._fitted()
    version = dev.version
    gp.append_XY(X[n0:], Y[n0:, None])
    assert gp._dev is dev and dev.block == len(X) - n0 and dev.version == version + 1
    assert not dev.appended and not dev.removed
    _check_snapshot(gp, snap, Xs, R.kdiag(spec), "%s %d -> %d" % (name, n0, len(X)))


def test_append_block_past_capacity(mods):
    """A fit at 12 rows reserves 128: blocks of 16 succeed up to 124 rows, the block that would
    cross 128 returns False with the GP unchanged (the bits of alpha and L^-1); ``append_XY``
    then refits, and block appends resume."""
    _, gpy, _, _ = mods
    spec, X, Y, Xs, ref = B.capacity_reference()
    n = B.CAPACITY_N0
    gp = _gp(gpy, spec, X[:n], Y[:n])
    dev = gp._fitted()
    for _ in range(B.CAPACITY_BLOCKS):
        gp.append_XY(X[n:n + 16], Y[n:n + 16, None])
        n += 16
        assert dev.block == 16 and dev.n == n
    _check_snapshot(gp, ref[124], Xs, R.kdiag(spec), "capacity 124 (blocks)")
    Linv, alpha = dev.factor()
    version = dev.version
    assert dev.append_block(X[n:n + 16], Y[n:n + 16]) is False
    assert dev.n == 124 and dev.version == version and dev.block == 16
    again = dev.factor()
    assert_array_equal(again[0], Linv)
    assert_array_equal(again[1], alpha)
    gp.append_XY(X[n:n + 16], Y[n:n + 16, None])
    n += 16
    assert gp._dev is dev and dev.n == 140 and dev.block == 0          # a refit
    _check_snapshot(gp, ref[140], Xs, R.kdiag(spec), "capacity 140 (refit)")
    gp.append_XY(X[n:n + 16], Y[n:n + 16, None])
    assert dev.n == 156 and dev.block == 16                             # appends resume
    _check_snapshot(gp, ref[156], Xs, R.kdiag(spec), "capacity 156 (block)")


def test_append_XY_chunks_and_refused_sizes(mods):
    """20 rows arrive as chunks of 16 + 4 (two versions); a block of 0 or 17 rows is refused by
    ``DeviceGP.append_block`` before anything runs."""
    _, gpy, _, _ = mods
    spec, X, Y, Xs, ref = B.capacity_reference()
    gp = _gp(gpy, spec, X[:104], Y[:104])
    dev = gp._fitted()
    version = dev.version
    with pytest.raises(ValueError):
        dev.append_block(X[104:121], Y[104:121])
    with pytest.raises(ValueError):
        dev.append_block(X[:0], Y[:0])
    gp.append_XY(X[104:124], Y[104:124, None])
    assert dev.n == 124 and dev.version == version + 2 and dev.block == 4
    _check_snapshot(gp, ref[124], Xs, R.kdiag(spec), "104 -> 120 -> 124")


# ---- the rank-b refresh ---------------------------------------------------------------------
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
    assert np.array_equal(S[keep].astype(bool), exp["S"][keep]), what
    if ret is not None:
        want = exp["ret"]
        assert ret[1] == want[1], what
        if want[1]:
            assert abs(ret[0] - want[0]) < RET_TOL, what
        else:
            assert ret[0] == -np.inf, what


def _setup(mods, name, rows=None):
    """The GPs of a case at n_fit and a grid of its rows (``rows``: a slice, with its global
    offset), swept at beta0."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case, ref = B.RANKB_CASES[name], B.rankb_reference(name)
    G = len(case["gps"])
    gps = [_gp(gpy, spec, ref["X"][g], ref["Y"][g]) for g, (spec, _, _) in enumerate(case["gps"])]
    devs = [gp._fitted() for gp in gps]
    pts = ref["pts"]
    if case["ctx_col"] is not None:
        pts = pts.copy()                    # made with another context and told the case's one
        pts[:, -1] = 9.0
    if rows is None:
        grid = _hip.DeviceGrid(devs[0].ctx, pts, G)
    else:
        grid = _hip.DeviceGrid(devs[0].ctx, pts[rows], G, global_offset=rows.start)
    if case["ctx_col"] is not None:
        grid.set_context([case["ctx_col"]])
    grid.confidence(devs, ref["beta0"], ref["fmin"])
    return case, ref, gps, devs, grid


def _append_step(case, devs, st):
    which = [1 if b else 0 for b in case["b"]]
    for g, b in enumerate(case["b"]):
        if b:
            assert devs[g].append_block(st["xstar"][:b], st["ystar"][g][:b])
            assert devs[g].block == b
    return which


def _run_rankb(mods, name):
    """Sweep at n_fit, then per step: ``append_block`` on the flagged GPs, ``rankb_update`` with
    another beta, compare mean, var, Q, S and the returned maximum with the refits."""
    from safeopt_amd import _hip
    case = B.RANKB_CASES[name]
    ctx = _hip.Context.default()             # (the context of every GPRegression)
    old = ctx.set_share(case["share"]) if case["share"] is not None else None
    try:
        case, ref, gps, devs, grid = _setup(mods, name)
        assert devs[0].ctx is ctx
        G = len(devs)
        for t, st in enumerate(ref["steps"]):
            which = _append_step(case, devs, st)
            ret = grid.rankb_update(devs, which, st["beta"], ref["fmin"])
            _compare_grid(grid, G, st, ref["fmin"], ref["kdiag"], ret, "%s step %d" % (name, t))
    finally:
        if old is not None:
            ctx.set_share(old)
    return devs, grid


@pytest.mark.parametrize("name", sorted(set(B.RANKB_CASES) - {"b16_mat52_d2_N4099"}))
def test_rankb_against_long_double(mods, name):
    """k_rankb against refits in long double: flagged GPs against n + b_g rows, the others
    against n rows with the new beta.  Rows: every new x* itself, two training rows, two rows
    60 lengthscales away; grids of 1 and 15 rows; b differing per GP; followers of a shared
    factor, behind a flagged leader and behind an unflagged one; ``aba``: the third GP follows
    nobody; d = 8 goes 668 -> 672 -> 676; a context column set by ``set_context``."""
    _run_rankb(mods, name)


def test_rankb_full_block(mods):
    """b = 16 at n0 = 56 (n crosses 64), 4099 rows, two GPs with the same inputs."""
    _run_rankb(mods, "b16_mat52_d2_N4099")


def test_rankb_refused_without_a_record(mods):
    """After a single append, a pop, new data, new hyper-parameters and on a clone there is no
    block record: ``rankb_update`` raises, names the GP, and leaves mean, var, Q and S as they
    were."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    name = "g1_mat32_d2_N15"
    case, ref = B.RANKB_CASES[name], B.rankb_reference(name)
    spec = case["gps"][0][0]
    st = ref["steps"][0]
    xb, yb = st["xstar"][:3], st["ystar"][0][:3]
    rng = np.random.default_rng(5)
    Xo = rng.uniform(-2, 2, size=(20, 2))

    def never(dev):
        return dev

    def after_single_append(dev):
        assert dev.append_block(xb[:2], yb[:2])
        assert dev.append(xb[2], yb[2])
        return dev

    def after_pop(dev):
        assert dev.append_block(xb, yb)
        dev.pop()
        return dev

    def after_new_data(dev):
        assert dev.append_block(xb, yb)
        dev.set_data(Xo, np.sin(Xo.sum(1)))
        return dev

    def after_hyper_edit(dev):
        assert dev.append_block(xb, yb)
        dev.set_hyper([1.3], [[1.0, 0.5]], 0.01)
        return dev

    def clone(dev):
        assert dev.append_block(xb, yb)
        twin = dev.clone()
        assert twin.block == 0 and dev.block == 3
        return twin

    for change in (never, after_single_append, after_pop, after_new_data, after_hyper_edit, clone):
        gp = _gp(gpy, spec, ref["X"][0], ref["Y"][0])
        dev = gp._fitted()
        grid = _hip.DeviceGrid(dev.ctx, ref["pts"], 1)
        grid.confidence([dev], ref["beta0"], ref["fmin"])
        before = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        dev = change(dev)
        assert dev.block == 0
        with pytest.raises(_hip.HipError, match="GP 0"):
            grid.rankb_update([dev], [1], st["beta"], ref["fmin"])
        after = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b), change.__name__


#: (case, shards).  The refresh adds the same bits to a row wherever it sits; for the whole
#: posterior to agree bit for bit the sweep in front of it has to as well.  The thread-per-row
#: sweep (every GP at 48 observations or fewer before the block) does, at any shard; the
#: matrix-core sweep of ``g3_mixed_d3_N197`` (75 observations) folds |L^-1 k|^2 in an order that
#: depends on a row's place in its 64-row tile -- measured: 38 of 312 swept var differ in the
#: last bit for rows [37, 141), none for shards that start on a tile -- so that case is cut at
#: tile starts only.
SHARD_CASES = [("g3_mixed_d3_n48_N197", (slice(37, 141), slice(64, 197), slice(0, 1))),
               ("g3_mixed_d3_N197", (slice(64, 197), slice(128, 197), slice(0, 1)))]


@pytest.mark.parametrize("name,shards", SHARD_CASES, ids=[c[0] for c in SHARD_CASES])
def test_rankb_shard_independence(mods, name, shards):
    """A grid of rows [a, b) of a case, with its global offset, gives bit for bit the mean, var
    and Q of those rows of the whole grid (fixed summation order, no atomics).  The posterior
    the refresh starts from is checked first: it has to have the same bits in both grids."""
    from safeopt_amd import _hip
    what = (_hip.MEAN, _hip.VAR, _hip.Q)
    case, ref, _, devs, whole = _setup(mods, name)
    start = [whole.download(w) for w in what]
    st = ref["steps"][0]
    which = _append_step(case, devs, st)
    whole.rankb_update(devs, which, st["beta"], ref["fmin"])
    full = [whole.download(w) for w in what]
    assert not np.array_equal(full[0], start[0]) and not np.array_equal(full[1], start[1])
    for rows in shards:
        _, _, _, devs_s, part = _setup(mods, name, rows)
        got = [part.download(w) for w in what]
        assert_array_equal(got[0], start[0][:, rows])          # the same bits to start from
        assert_array_equal(got[1], start[1][:, rows])
        _append_step(case, devs_s, st)
        part.rankb_update(devs_s, which, st["beta"], ref["fmin"])
        got = [part.download(w) for w in what]
        assert_array_equal(got[0], full[0][:, rows])
        assert_array_equal(got[1], full[1][:, rows])
        assert_array_equal(got[2], full[2][rows])


# ---- end to end -----------------------------------------------------------------------------
def _safeopt(mods):
    safeopt_amd, gpy, _, _ = mods
    X, Y = B.e2e_data()
    gps = [gpy.models.GPRegression(X, Y[:, [g]], R.make_kernel(gpy.kern, spec), noise_var=R.NOISE)
           for g, spec in enumerate(B.E2E_SPECS)]
    grid = safeopt_amd.linearly_spaced_combinations([(-2, 2), (-2, 2)], B.E2E_SIDE)
    opt = safeopt_amd.SafeOpt(gps, grid, [0.0, 0.0], lipschitz=None, beta=2.0, threshold=0.0)
    assert opt._backend.small_step_devs() is None       # the large-grid path: sweeps and refreshes
    return opt


def _check_against_twin(opt, twin, x, what):
    """Q within 1e-8, S identical outside the excluded rows, and the row ``opt`` chose as wide
    (within 1e-8) as the widest row of the twin's M | G."""
    Qo, Qt = np.asarray(opt.Q), np.asarray(twin.Q)
    print("%s: Q %.2e" % (what, np.max(np.abs(Qo - Qt))))
    assert np.max(np.abs(Qo - Qt)) < Q_TOL, what
    fmin = np.asarray(twin.fmin, dtype=float)
    keep = ~np.any(np.abs(Qt[:, ::2] - fmin[None, :]) < R.S_EXCLUDE, axis=1)
    assert_array_equal(np.asarray(opt.S)[keep], np.asarray(twin.S)[keep])
    width = np.max((Qt[:, 1::2] - Qt[:, ::2]) / np.asarray(twin.scaling)[None, :], axis=1)
    mg = np.asarray(twin.M) | np.asarray(twin.G)
    row = np.flatnonzero(np.all(twin.inputs == np.asarray(x)[None, :], axis=1))
    assert row.size == 1 and mg.any(), what
    print("%s: width at the chosen row %.6f, twin's maximum %.6f"
          % (what, width[row[0]], width[mg].max()))
    assert abs(width[row[0]] - width[mg].max()) < Q_TOL, what


def test_safeopt_batch_round_trip(mods):
    """40 x 40 grid, 2 GPs, n = 30: ``optimize_batch(size=4)``, ``add_new_data_points``,
    ``optimize()`` -- the backend's streak rises by 4 (a block refresh, no sweep) -- against a
    twin fed by four ``add_new_data_point`` calls (a sweep).  Then a block of 16 with the
    streak at 4 takes the sweep."""
    opt, twin = _safeopt(mods), _safeopt(mods)
    Xb = opt.optimize_batch(size=4)
    assert Xb.shape == (4, 2) and opt._backend._rank1_streak == 0
    Yb = np.stack([B.e2e_f(Xb, g) for g in range(2)], axis=1)
    opt.add_new_data_points(Xb, Yb)
    assert [gp._dev.block for gp in opt.gps] == [4, 4] and opt.t == B.E2E_N + 4
    x = opt.optimize()
    assert opt._backend._rank1_streak == 4
    twin.optimize()
    for xr, yr in zip(Xb, Yb):
        twin.add_new_data_point(xr, yr)
    assert_array_equal(twin.x, opt.x)
    assert_array_equal(twin.y, opt.y)
    twin.optimize()
    assert twin._backend._rank1_streak == 0
    _check_against_twin(opt, twin, x, "block of 4")

    # 16 rows spread over M | G as optimize() left them (no interval update in between: the
    # streak stays at 4)
    mg = np.flatnonzero(np.asarray(opt.M) | np.asarray(opt.G))
    assert mg.size >= 16
    Xb = opt.inputs[mg[np.linspace(0, mg.size - 1, 16).astype(int)]]
    assert len(set(map(tuple, Xb))) == 16 and opt._backend._rank1_streak == 4
    Yb = np.stack([B.e2e_f(Xb, g) for g in range(2)], axis=1)
    opt.add_new_data_points(Xb, Yb)
    assert [gp._dev.block for gp in opt.gps] == [16, 16]
    x = opt.optimize()
    assert opt._backend._rank1_streak == 0                 # 4 + 16 > refresh_every: a sweep
    for xr, yr in zip(Xb, Yb):
        twin.add_new_data_point(xr, yr)
    twin.optimize()
    _check_against_twin(opt, twin, x, "block of 16")
    opt.remove_last_data_point()
    opt.remove_data_point(B.E2E_N + 1)
    assert opt.t == B.E2E_N + 18 and all(gp._dev.n == opt.t for gp in opt.gps)


def test_swarm_add_new_data_points(mods):
    """``SafeOptSwarm.add_new_data_points`` with a ``nan`` column entry: every GP's alpha and
    posterior match the twin fed row by row, and ``optimize()`` runs."""
    np.random.seed(2)
    opt = _swarm_problem(mods, "device")
    np.random.seed(2)
    twin = _swarm_problem(mods, "device")
    rng = np.random.default_rng(77)
    lo = np.array([b[0] for b in opt.bounds], dtype=float)
    hi = np.array([b[1] for b in opt.bounds], dtype=float)
    Xb = opt.gp.X[:1] + 0.05 * (hi - lo) * rng.uniform(-1, 1, size=(5, lo.size))
    Yb = np.stack([np.asarray(opt.gps[g].Y)[0, 0] + 0.1 * np.sin(3.0 * Xb.sum(1) + g)
                   for g in range(2)], axis=1)
    Yb[2, 1] = np.nan
    opt.add_new_data_points(Xb, Yb)
    for xr, yr in zip(Xb, Yb):
        twin.add_new_data_point(xr, yr)
    assert [gp._dev.block for gp in opt.gps] == [5, 4]
    assert_array_equal(opt.x, twin.x)
    assert_array_equal(opt.y, twin.y)
    Xs = lo + (hi - lo) * rng.uniform(size=(300, lo.size))
    for g, (a, b) in enumerate(zip(opt.gps, twin.gps)):
        assert_array_equal(a.X, b.X)
        assert_array_equal(a.Y, b.Y)
        al_a, al_b = a._fitted().factor()[1], b._fitted().factor()[1]
        ea = np.max(np.abs(al_a - al_b)) / np.max(np.abs(al_b))
        print("GP %d: alpha %.2e" % (g, ea))
        assert ea < ALPHA_TOL
        (ma, va), (mb, vb) = a.predict_noiseless(Xs), b.predict_noiseless(Xs)
        check_posterior(ma[:, 0], va[:, 0], mb[:, 0], vb[:, 0], float(a.kern.Kdiag(Xs[:1])[0]))
    x = np.ravel(opt.optimize())
    assert x.size == lo.size and np.all(x >= lo) and np.all(x <= hi)
