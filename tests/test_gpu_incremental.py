"""GPU parity of the incremental path -- ``sgp_gp_append`` / ``sgp_gp_pop`` (factor.hip) and the
closed-form refresh of the resident posterior, ``sgp_grid_rank1_update`` (k_rank1, expander.hip) --
against a long-double GP (tests/_incremental_ref.py), through the C ABI.

Every BO step but each 16th rests on these kernels.  The cases vary what selects code paths:
kernel kinds and products, d = 1 .. 8, both sides of k_rank1's LDS switch, GPs that are and
are not refreshed, followers of a shared factor, a new beta, context columns, fewer than 64
rows, n across 16 .. 1024 and the order of fit / pop / append.  The tolerances are the
project's: ``check_posterior`` (1e-9, 1e-5 relative), 1e-8 on L^-1, alpha (relative to
max |alpha|) and Q, equality of S outside the rows tests/test_incremental_ref_cpu.py counts.
That module also shows that a float64 implementation stays within 1 % of each of them on
these very cases."""
import numpy as np
import pytest

import _incremental_ref as R
from _gpu_common import (  # noqa: F401
    MEAN_TOL, VAR_TOL, mods, check_posterior)

pytestmark = pytest.mark.gpu

LINV_TOL = ALPHA_TOL = Q_TOL = RET_TOL = 1e-8


def _gp(gpy, spec, X, Y):
    return gpy.models.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpy.kern, spec),
                                   noise_var=R.NOISE)


def _check_snapshot(gp, snap, Xs, kd, what):
    """alpha, L^-1 (where the reference has it) and the posterior at Xs against a refit."""
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


# ---- append / pop -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.APPEND_CASES))
def test_append_against_long_double(mods, name):
    """Fit at n_fit, then ``sgp_gp_append`` row by row to n_end: alpha, L^-1 (n <= 520) and the
    posterior at 300 rows against the long-double refit after every append."""
    _, gpy, _, _ = mods
    spec, d, n_fit, n_end = R.APPEND_CASES[name]
    X, Y, Xs, _, _ = R.data(name, d, n_end)
    gp = _gp(gpy, spec, X[:n_fit], Y[:n_fit])
    dev = gp._fitted()
    for snap in R.append_reference(name):
        n = snap["n"]
        assert dev.append(X[n - 1], Y[n - 1]) and dev.appended, "append at n = %d refused" % n
        _check_snapshot(gp, snap, Xs, R.kdiag(spec), "%s n = %d" % (name, n))


@pytest.mark.parametrize("name", sorted(R.POP_CASES))
def test_pop_then_append(mods, name):
    """Fit, pop 7, append 3 OTHER rows, pop 1, append 2: what a pop leaves behind in the padded
    block (rows of L^-1, the packed operands, the scaled inputs, alpha, the update vector) must
    not reach a later append; n crosses a multiple of 16 downwards and upwards."""
    _, gpy, _, _ = mods
    spec, d, n = R.POP_CASES[name]
    X, Y, Xs, E, YE = R.data(name, d, n, extra=5)
    gp = _gp(gpy, spec, X, Y)
    dev = gp._fitted()
    e = 0
    for i, (what, snap) in enumerate(R.pop_reference(name)):
        if what == "pop":
            dev.pop()
            assert not dev.appended
        elif what == "append":
            assert dev.append(E[e], YE[e]) and dev.appended
            e += 1
        _check_snapshot(gp, snap, Xs, R.kdiag(spec), "%s call %d (%s)" % (name, i, what))


def test_append_past_capacity(mods):
    """``GPRegression.set_XY`` with one more row per call, from 12 rows on: bordered appends
    until the rows reserved at the fit are used up (128), one refit, appends again."""
    _, gpy, _, _ = mods
    spec, d, n0, n_end = R.CAPACITY
    X, Y, Xs, _, _ = R.data("capacity", d, n_end)
    ref = R.capacity_reference()
    gp = _gp(gpy, spec, X[:n0], Y[:n0])
    outcome = {}
    for n in range(n0 + 1, n_end + 1):
        gp.set_XY(X[:n], Y[:n, None])
        outcome[n] = gp._dev.appended
        if n in ref or not outcome[n]:
            assert n in ref, "refit at n = %d, which has no reference" % n
            _check_snapshot(gp, ref[n], Xs, R.kdiag(spec), "capacity n = %d (%s)"
                            % (n, "append" if outcome[n] else "refit"))
    refits = [n for n, a in outcome.items() if not a]
    print("refits at n =", refits)
    assert refits == [129]                        # both outcomes; 128 rows were reserved
    assert all(outcome[n] for n in range(130, n_end + 1))      # ... and appends resume


# ---- the rank-1 refresh -------------------------------------------------------------------
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


def _run_rank1(mods, name):
    """Sweep at n_fit, then per step: append (x*, y*) to the GPs of ``which``, refresh with
    another beta, compare mean, var, Q, S and the returned maximum with the refits."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case, ref = R.RANK1_CASES[name], R.rank1_reference(name)
    G = len(case["gps"])
    gps = [_gp(gpy, spec, ref["X"][g], ref["Y"][g]) for g, (spec, _, _) in enumerate(case["gps"])]
    devs = [gp._fitted() for gp in gps]
    ctx = devs[0].ctx
    old = ctx.set_share(case["share"]) if case["share"] is not None else None
    try:
        pts = ref["pts"]
        if case["ctx_col"] is not None:
            # the grid is made with another context and told the case's one
            pts = pts.copy()
            pts[:, -1] = 9.0
        grid = _hip.DeviceGrid(ctx, pts, G)
        if case["ctx_col"] is not None:
            grid.set_context([case["ctx_col"]])
        grid.confidence(devs, ref["beta0"], ref["fmin"])
        for t, st in enumerate(ref["steps"]):
            for g in range(G):
                if case["which"][g]:
                    assert devs[g].append(st["xstar"], st["ystar"][g])
            ret = grid.rank1_update(devs, case["which"], st["beta"], ref["fmin"])
            _compare_grid(grid, G, st, ref["fmin"], ref["kdiag"], ret, "%s step %d" % (name, t))
    finally:
        if old is not None:
            ctx.set_share(old)
    return gps, grid


@pytest.mark.parametrize("name", sorted(set(R.RANK1_CASES) - {"ctx_prod_d3", "streak_mat52_d2"}))
def test_rank1_against_long_double(mods, name):
    """k_rank1 against refits in long double: GPs of ``which`` against n + 1 rows, the others
    against n rows with the new beta.  Rows: x* itself, two training rows (r = 0), two rows 60
    lengthscales away, grids of 1 and 15 rows; d = 8 goes 671 -> 672 -> 673, staged in LDS and
    then not; ``aba``: the third GP follows nobody and must not inherit the second's c(x)."""
    _run_rank1(mods, name)


def test_rank1_with_context_columns(mods):
    """A grid with a context column (set_context) under a parameters x context product kernel:
    sweep, append, refresh as above; then, through the grid backend SafeOpt drives, a change
    of context makes the next ``confidence`` a sweep -- a refresh would correct the posterior
    of the old context's rows."""
    _, gpy, _, _ = mods
    from safeopt_amd.gp_opt import _HipGridBackend
    _run_rank1(mods, "ctx_prod_d3")
    case, ref = R.RANK1_CASES["ctx_prod_d3"], R.rank1_reference("ctx_prod_d3")
    st, sw = ref["steps"][0], R.context_switch_reference()
    G = len(case["gps"])
    gps = [_gp(gpy, spec, ref["X"][g], ref["Y"][g]) for g, (spec, _, _) in enumerate(case["gps"])]
    pts = ref["pts"].copy()
    pts[:, -1] = 9.0
    be = _HipGridBackend(gps, pts, 0)
    be.set_context([case["ctx_col"]])
    be.confidence(ref["beta0"], ref["fmin"])
    assert be._rank1_streak == 0

    def add(x, y):
        for g, gp in enumerate(gps):
            gp.set_XY(np.vstack([gp.X, x[None, :]]), np.vstack([gp.Y, [[y[g]]]]))
            assert gp._dev.appended
    add(st["xstar"], st["ystar"])
    ret = be.confidence(st["beta"], ref["fmin"])
    assert be._rank1_streak == 1                                   # a refresh
    _compare_grid(be.grid, G, st, ref["fmin"], ref["kdiag"], ret, "backend refresh")
    be.set_context([R.CTX_SECOND])
    add(sw["x2"], sw["y2"])
    be.confidence(sw["beta"], ref["fmin"])
    assert be._rank1_streak == 0                                   # a sweep
    _compare_grid(be.grid, G, sw, ref["fmin"], ref["kdiag"], None, "backend after set_context")


def test_rank1_streak(mods):
    """15 refreshes in a row (what a BO loop sees between two forced sweeps), n 56 -> 71 across
    64, 4099 rows, two GPs: every one, the 15th included, within the bounds of a single one."""
    _run_rank1(mods, "streak_mat52_d2")


def test_rank1_refused_without_a_record(mods):
    """After a pop, after new data, after new hyper-parameters and on a clone of a GP that was
    never appended to there is no append record: ``rank1_update`` raises and leaves mean, var,
    Q and S as they were."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    name = "g1_mat32_d2_N15"
    case, ref = R.RANK1_CASES[name], R.rank1_reference(name)
    spec = case["gps"][0][0]
    st = ref["steps"][0]
    rng = np.random.default_rng(5)
    Xo = rng.uniform(-2, 2, size=(20, 2))

    def after_pop(dev):
        assert dev.append(st["xstar"], st["ystar"][0])
        dev.pop()
        return dev

    def after_new_data(dev):
        assert dev.append(st["xstar"], st["ystar"][0])
        dev.set_data(Xo, np.sin(Xo.sum(1)))
        return dev

    def after_hyper_edit(dev):
        assert dev.append(st["xstar"], st["ystar"][0])
        dev.set_hyper([1.3], [[1.0, 0.5]], 0.01)
        return dev

    def fresh_clone(dev):
        return dev.clone()

    for change in (after_pop, after_new_data, after_hyper_edit, fresh_clone):
        gp = _gp(gpy, spec, ref["X"][0], ref["Y"][0])
        dev = gp._fitted()
        grid = _hip.DeviceGrid(dev.ctx, ref["pts"], 1)
        grid.confidence([dev], ref["beta0"], ref["fmin"])
        before = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        dev = change(dev)
        with pytest.raises(_hip.HipError):
            grid.rank1_update([dev], [1], st["beta"], ref["fmin"])
        after = [grid.download(w) for w in (_hip.MEAN, _hip.VAR, _hip.Q, _hip.S)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b), change.__name__
