"""Posterior sample paths on the device (csrc/paths.hip) against the NumPy statement of
tests/_paths_numpy.py (needs an MI355X).

Shapes: the odd values are the edges of the 4-wide k-step (m = 1, 5; n = 1, 17), the 16-wide
column block (S = 1, 5, 16, 17, 64), the 64-row tile and the last partial workgroup (N = 1, 63,
257, 4099), the 64-row LDS stage of [W ; V] (m = 68, 256; n = 100, 300).

Tolerances.  Weights: the backward error |Ky V - rhs|_inf / (|Ky|_inf |V|_inf + |rhs|_inf), which
does not see cond(Ky), held to 10 x that of the helper's own float64 Cholesky solve (not below
n 2^-53).  Evaluation: |device - reference| <= c x (sum of the absolute terms of the path),
c = max(100 D, (m + n + 8 (d + 2) A) 2^-53), D the helper's float64 / long-double discrepancy in
the same unit, A the largest cosine argument of the case (its rounding enters the cosine
absolutely).  The golden scenarios of ``thompson_points`` are those of tests/_golden.py.
"""
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
from _golden import load
from _gpu_common import mods, smooth, build_opt  # noqa: F401

pytestmark = pytest.mark.gpu

NOISE = 0.05 ** 2
LD = np.longdouble
KINDS = ["RBF", "Matern32", "Matern52", "product"]
D_, N_, M_, S_, R_ = [1, 2, 8], [1, 17, 100, 300], [1, 5, 68, 256], [1, 5, 16, 17, 64], \
    [1, 63, 257, 4099]


def _cases():
    """40 cases: every (kind, d) pair at least three times, every value of every axis."""
    rng = np.random.RandomState(11)
    out = []
    for i in range(40):
        out.append((KINDS[i % 4], D_[i % 3], N_[(i // 2 + i) % 4], M_[(i // 3 + 2 * i) % 4],
                    S_[(i + i // 5) % 5], R_[int(rng.randint(4)) if i % 5 else 3]))
    for ax, vals in ((2, N_), (3, M_), (4, S_), (5, R_)):
        assert sorted(set(c[ax] for c in out)) == vals
    return out


CASES = _cases()
IDS = ["%s-d%d-n%d-m%d-S%d-N%d" % c for c in CASES]


def make_kernel(ns, kind, d):
    if kind == "product":
        if d == 1:
            a, b = [0], [0]
        elif d == 2:
            a, b = [0], [1]
        else:
            a, b = [0, 1, 2, 3], [3, 4, 5, 6, 7]
        return (ns.Matern52(len(a), variance=1.3, lengthscale=np.linspace(0.9, 1.7, len(a)),
                            ARD=True, active_dims=a, name="pa") *
                ns.RBF(len(b), variance=0.9, lengthscale=np.linspace(0.7, 1.4, len(b)), ARD=True,
                       active_dims=b, name="pb"))
    ls = np.linspace(0.5, 2.5, d) if kind == "Matern52" else np.linspace(0.8, 1.6, d)
    return getattr(ns, kind)(d, variance=1.7, lengthscale=ls, ARD=True)


@functools.lru_cache(maxsize=None)
def problem(kind, d, n, m, S, N):
    """Data, random numbers and the rows of a case; computed once, never modified."""
    from safeopt_amd import paths as P
    import safeopt_amd.gpy as gpy
    rng = np.random.RandomState(1000 * n + 10 * m + S + d)
    X = rng.uniform(-2.5, 2.5, (n, d))
    Y = smooth(X, n) + 0.05 * rng.standard_normal((n, 1))
    Xs = rng.uniform(-3, 3, (N, d))
    desc = make_kernel(gpy.kern, kind, d)._desc(d)
    kern = ([int(k) for k in desc[1]], [float(v) for v in desc[2]], desc[3].copy())
    Om, b, W, E = P.draw_path_inputs((kern[0], kern[2]), NOISE, n, d, S, m, rng=rng)
    for a in (X, Y, Xs, Om, b, W, E, kern[2]):
        a.setflags(write=False)
    return kern, X, Y, Xs, Om, b, W, E


_GPS = {}


def device_gp(gpy, kind, d, n, m, S, N):
    key = (kind, d, n, m, S, N)
    if key not in _GPS:
        _, X, Y = problem(*key)[:3]
        _GPS[key] = gpy.models.GPRegression(X, Y, make_kernel(gpy.kern, kind, d), noise_var=NOISE)
    return _GPS[key]


@functools.lru_cache(maxsize=None)
def device_weights(case):
    import safeopt_amd.gpy as gpy
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    V = device_gp(gpy, *case)._fitted().path_weights(Om, b, W, E)
    V.setflags(write=False)
    return V


def record(name, value):
    """Observed error ratios for profiles/paths/SUMMARY.txt (scripts/bench_paths.py --figures)."""
    path = os.environ.get("SGP_PATHS_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write("%s %.6e\n" % (name, value))


# ---- 1. weights --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weights_backward_error(mods, case):
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    n = X.shape[0]
    V = device_weights(case)
    assert V.shape == (n, W.shape[1])
    Ky = pn.gram(kern, NOISE, X, LD)
    rhs = pn.weight_rhs(kern, X, Y, Om, b, W, E, LD)
    own = pn.weights_residual(Ky, pn.path_weights(kern, NOISE, X, Y[:, 0], Om, b, W, E).astype(LD), rhs)
    dev = pn.weights_residual(Ky, V.astype(LD), rhs)
    bound = 10 * max(float(own), n * 2.0 ** -53)
    print("weights residual: device %.3e, float64 solve %.3e, bound %.3e, ratio %.3f"
          % (dev, own, bound, dev / bound))
    record("weights", float(dev / bound))
    assert dev <= bound


# ---- 2. evaluation -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_evaluation_entry_by_entry(mods, case):
    _, gpy, _, _ = mods
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    kind, d, n, m, S, N = case
    V = device_weights(case)
    out = device_gp(gpy, *case)._fitted().paths_eval(Om, b, W, V, Xs)
    assert out.shape == (N, S)
    ref = pn.paths_eval(kern, X, Om, b, W, V, Xs)
    refl = pn.paths_eval_ld(kern, X, Om, b, W, V, Xs)
    budget = pn.abs_budget(kern, X, Om, b, W, V, Xs)
    Dm = float(np.max(np.abs(ref - refl) / budget))
    A = max(1.0, float(np.abs(pn.feature_args(Om, b, Xs)).max()))
    c = max(100 * Dm, (m + n + 8 * (d + 2) * A) * 2.0 ** -53)
    err = float(np.max(np.abs(out - ref) / budget))
    print("evaluation: |dev - ref| / budget %.3e, D %.3e, A %.1f, c %.3e, ratio %.3f"
          % (err, Dm, A, c, err / c))
    record("evaluation", err / c)
    record("evaluation_abs", err)
    assert np.all(np.abs(out - ref) <= c * budget)


# ---- 3. layouts and repeats --------------------------------------------------------------------

@pytest.mark.parametrize("case", [CASES[3], CASES[14], CASES[25]], ids=[IDS[3], IDS[14], IDS[25]])
def test_layouts_repeats_and_subsets_give_the_same_bits(mods, case):
    _, gpy, _, _ = mods
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    N, d = Xs.shape
    dev = device_gp(gpy, *case)._fitted()
    V = device_weights(case)
    out = dev.paths_eval(Om, b, W, V, np.ascontiguousarray(Xs))
    wide = np.zeros((2 * N, 2 * d + 1))
    wide[::2, 1::2] = Xs
    for other in (np.asfortranarray(Xs), wide[::2, 1::2], np.ascontiguousarray(Xs)):
        assert_array_equal(dev.paths_eval(Om, b, W, V, other), out)
    assert_array_equal(dev.path_weights(Om, b, W, E), V)
    rows = np.random.RandomState(0).permutation(N)[:max(1, N // 3)]
    assert_array_equal(dev.paths_eval(Om, b, W, V, Xs[rows]), out[rows])


def test_posterior_paths_of_the_model(mods):
    _, gpy, _, _ = mods
    case = CASES[5]
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    gp = gpy.models.GPRegression(X, Y, make_kernel(gpy.kern, case[0], case[1]), noise_var=NOISE)
    np.random.seed(4)
    pp = gp.posterior_paths(size=5, features=68)
    assert pp.V.shape == (X.shape[0], 5) and pp.W.shape == (68, 5)
    f = pp.paths(Xs)
    assert f.shape == (Xs.shape[0], 1, 5)
    assert_array_equal(pp.paths(Xs), f)
    sub = np.arange(0, Xs.shape[0], 3)
    assert_array_equal(pp.paths(Xs[sub]), f[sub])
    assert pp.paths(np.empty((0, Xs.shape[1]))).shape == (0, 1, 5)
    np.random.seed(4)
    assert_array_equal(gp.posterior_paths(size=5, features=68).paths(Xs), f)
    # the NumPy form with the same numbers
    ref = pn.paths_eval(kern, X, pp.Omega, pp.phase, pp.W, pp.V, Xs)
    assert np.max(np.abs(f[:, 0, :] - ref)) < 1e-11 * pn.abs_budget(kern, X, pp.Omega, pp.phase,
                                                                   pp.W, pp.V, Xs).max()
    # a snapshot: data or hyper-parameters changed -> stale
    gp.set_XY(np.vstack([X, Xs[:1]]), np.vstack([Y, [[0.3]]]))
    with pytest.raises(ValueError, match="stale"):
        pp.paths(Xs)
    pp2 = gp.posterior_paths(size=2, features=5)
    pp2.paths(Xs)
    gp.noise_var = 0.01
    with pytest.raises(ValueError, match="stale"):
        pp2.paths(Xs)


# ---- 4. grid -----------------------------------------------------------------------------------

def masked_argmax(values, mask, goff=0):
    """NumPy's first-index arg-max per path over the rows of ``mask``."""
    bv = np.full(values.shape[1], -np.inf)
    bi = np.full(values.shape[1], -1, dtype=np.int64)
    rows = np.flatnonzero(mask)
    if rows.size:
        k = np.argmax(values[rows], axis=0)
        bi = rows[k] + goff
        bv = values[rows[k], np.arange(values.shape[1])]
    return bv, bi


GRID_CASE = ("Matern52", 2, 100, 68, 17, 4099)


def grid_setup(mods, rows, goff=0):
    safeopt_amd, gpy, _, _ = mods
    from safeopt_amd import _hip
    gp = device_gp(gpy, *GRID_CASE)
    dev = gp._fitted()
    kern, X, Y, Xs, Om, b, W, E = problem(*GRID_CASE)
    V = device_weights(GRID_CASE)
    grid = _hip.DeviceGrid(dev.ctx, rows, 1, goff)
    return _hip, dev, grid, (Om, b, W, V)


@pytest.mark.parametrize("which", ["tensor", "rows"])
def test_grid_values_and_argmax(mods, which):
    safeopt_amd = mods[0]
    if which == "tensor":
        rows = safeopt_amd.linearly_spaced_combinations([(-3., 3.), (-2., 2.)], [30, 31])
    else:
        rows = problem(*GRID_CASE)[3]
    _hip, dev, grid, ops = grid_setup(mods, rows)
    N = rows.shape[0]
    vals, bv, bi = grid.paths(dev, *ops, mask=False, values=True)
    assert_array_equal(vals, dev.paths_eval(*ops, rows))
    ev, ei = masked_argmax(vals, np.ones(N, dtype=bool))
    assert_array_equal(bv, ev)
    assert_array_equal(bi, ei)
    none, bv2, bi2 = grid.paths(dev, *ops, mask=False, values=False)
    assert none is None
    assert_array_equal(bv2, bv)
    assert_array_equal(bi2, bi)
    rng = np.random.RandomState(2)
    last = np.zeros(N, dtype=bool)
    last[N - 2] = True                    # (4099: a row of the last, partial workgroup)
    one = np.zeros(N, dtype=bool)
    one[N // 3] = True
    for mask in (rng.rand(N) < 0.3, one, last, np.zeros(N, dtype=bool)):
        grid.upload_mask(_hip.S, mask)
        for want in (True, False):
            v, mv, mi = grid.paths(dev, *ops, mask=True, values=want)
            ev, ei = masked_argmax(vals, mask)
            assert_array_equal(mv, ev)
            assert_array_equal(mi, ei)
            if want:
                assert_array_equal(v, vals)
    assert np.all(mi == -1) and np.all(np.isneginf(mv))       # (the empty mask came last)
    # mask = 0 ignores S
    assert_array_equal(grid.paths(dev, *ops, mask=False)[2], bi)


def test_grid_tie_goes_to_the_lower_row_across_workgroups(mods):
    rows = problem(*GRID_CASE)[3].copy()
    N = rows.shape[0]
    _hip, dev, grid, ops = grid_setup(mods, rows)
    vals, bv, bi = grid.paths(dev, *ops, values=True)
    top = int(bi[0])
    twin = (top + 2048 + 7) % N                   # 32 tiles away: another workgroup
    assert twin // 64 != top // 64
    rows[twin] = rows[top]
    _hip, dev, grid, ops = grid_setup(mods, rows)
    vals, bv, bi = grid.paths(dev, *ops, values=True)
    assert vals[twin, 0] == vals[top, 0] == vals[:, 0].max()
    assert bi[0] == min(top, twin)
    ev, ei = masked_argmax(vals, np.ones(N, dtype=bool))
    assert_array_equal(bi, ei)
    assert_array_equal(bv, ev)
    mask = np.zeros(N, dtype=bool)
    mask[[top, twin]] = True
    grid.upload_mask(_hip.S, mask)
    assert grid.paths(dev, *ops, mask=True)[2][0] == min(top, twin)


def test_grid_global_offset(mods):
    rows = problem(*GRID_CASE)[3]
    _hip, dev, grid, ops = grid_setup(mods, rows[1000:3000], goff=1000)
    _, bv, bi = grid.paths(dev, *ops)
    vals = dev.paths_eval(*ops, rows)
    ev, ei = masked_argmax(vals[1000:3000], np.ones(2000, dtype=bool), goff=1000)
    assert_array_equal(bi, ei)
    assert_array_equal(bv, ev)


# ---- 5. SafeOpt.thompson_points ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["safeopt_1d_rbf", "safeopt_2d_rbf", "safeopt_context"])
def test_thompson_points_end_to_end(mods, name):
    z, meta = load(name)
    t = meta["recorded"][0]
    opt = build_opt(mods, z, meta, t)
    ctx = z["it%d_context" % t] if meta["num_contexts"] else None
    with pytest.raises(RuntimeError):                 # nothing is safe before the first step
        opt.thompson_points(size=3, features=16)
    x_next = opt.optimize(context=ctx)
    before = [np.array(a) for a in (opt.Q, opt.S, opt.M, opt.G, opt.x, opt.y, opt.gp.X, opt.gp.Y)]
    np.random.seed(9)
    x, v, values = opt.thompson_points(size=8, features=68, return_values=True)
    dp = opt.parameter_set.shape[1]
    assert x.shape == (8, dp) and v.shape == (8,) and values.shape == (opt.inputs.shape[0], 8)
    S = np.array(opt.S)
    for k in range(8):
        hits = np.flatnonzero((opt.parameter_set == x[k]).all(1))
        assert hits.size and S[hits].any()
    ev, ei = masked_argmax(values, S)
    assert_array_equal(v, ev)
    assert_array_equal(x, opt.parameter_set[ei])
    np.random.seed(9)
    pp = opt.gp.posterior_paths(size=8, features=68)
    at = pp.paths(opt.inputs[ei])[:, 0, :]
    assert_array_equal(v, at[np.arange(8), np.arange(8)])
    np.random.seed(9)
    x2, v2 = opt.thompson_points(size=8, features=68)
    assert_array_equal(x2, x)
    assert_array_equal(v2, v)
    xa, va = opt.thompson_points(size=4, features=16, within='all')
    assert xa.shape == (4, dp)
    after = [np.array(a) for a in (opt.Q, opt.S, opt.M, opt.G, opt.x, opt.y, opt.gp.X, opt.gp.Y)]
    for a, b in zip(before, after):
        assert_array_equal(a, b)
    assert_array_equal(opt.optimize(context=ctx), x_next)
    # pending edits of opt.S reach the device first
    opt.S[:] = False
    with pytest.raises(RuntimeError):
        opt.thompson_points(size=2, features=16)
    keep = int(np.flatnonzero(S)[0])
    opt.S[keep] = True
    xs, _ = opt.thompson_points(size=3, features=16)
    assert_array_equal(xs, np.repeat(opt.parameter_set[keep:keep + 1], 3, axis=0))
    with pytest.raises(ValueError):
        opt.thompson_points(within='nowhere')
    # a stale snapshot
    y = np.full((1, len(opt.gps)), float(np.mean(opt.y[:, 0])))
    opt.add_new_data_point(x_next, y, context=ctx)
    with pytest.raises(ValueError, match="stale"):
        pp.paths(opt.inputs[:3])


def test_thompson_points_needs_one_rank(mods):
    z, meta = load("safeopt_1d_rbf")
    opt = build_opt(mods, z, meta, meta["recorded"][0])

    class TwoRanks(object):
        world, rank = 2, 0
    opt._comm = TwoRanks()
    with pytest.raises(NotImplementedError, match="one rank"):
        opt.thompson_points()


# ---- 6. caps -----------------------------------------------------------------------------------

def test_caps_and_empty_inputs(mods):
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    case = CASES[0]
    kern, X, Y, Xs, Om, b, W, E = problem(*case)
    n, d = X.shape
    gp = device_gp(gpy, *case)
    dev = gp._fitted()
    V = device_weights(case)
    with pytest.raises((_hip.HipError, ValueError), match="64"):
        dev.path_weights(Om, b, np.zeros((Om.shape[0], 65)), np.zeros((n, 65)))
    with pytest.raises((_hip.HipError, ValueError), match="64"):
        dev.paths_eval(Om, b, np.zeros((Om.shape[0], 65)), np.zeros((n, 65)), Xs)
    big = 16385
    with pytest.raises((_hip.HipError, ValueError), match="16384"):
        dev.paths_eval(np.zeros((big, d)), np.zeros(big), np.zeros((big, 1)), np.zeros((n, 1)), Xs)
    with pytest.raises((_hip.HipError, ValueError), match="16384"):
        gp.posterior_paths(size=1, features=big)
    assert dev.paths_eval(Om, b, W, V, np.empty((0, d))).shape == (0, W.shape[1])
    # a GP that never received data
    desc = gp.kern._desc(d)
    fresh = _hip.DeviceGP(dev.ctx, desc, NOISE)
    with pytest.raises((_hip.HipError, ValueError)):
        fresh.paths_eval(Om, b, W, V, Xs)
    with pytest.raises(_hip.HipError, match="no data"):
        fresh.path_weights(Om, b, W, np.zeros((0, W.shape[1])))


def test_unfitted_gp_raises_as_the_exact_draw_does(mods):
    """An infeasible theta in ``lml`` leaves the data resident and the factor missing: the three
    path entry points refuse with the error the exact draw (``posterior_samples_f``'s device
    call) gives, and the GPRegression refits at its own hyper-parameters for both."""
    _, gpy, _, _ = mods
    from safeopt_amd import _hip
    rng = np.random.RandomState(11)
    X = rng.uniform(-2, 2, (20, 2))
    X = np.vstack([X, X])                       # duplicated inputs
    Y = np.sin(X).sum(1)[:, None]
    Y[20:] += 0.01
    k = gpy.kern.RBF(2, 1.0, [1.0, 1.0], ARD=True)
    gp = gpy.models.GPRegression(X, Y, k, noise_var=NOISE)
    pp = gp.posterior_paths(size=3, features=5)
    Xs = rng.uniform(-2, 2, (7, 2))
    before = pp.paths(Xs)
    dev = gp._fitted()
    desc = k._desc(2)
    # Ky = K - 0.9e-8 I on duplicated rows: not positive definite
    assert gp._evaluate(desc[2], desc[3], -1.9e-8)[4] != 0
    with pytest.raises(_hip.HipError, match="not fitted") as exact:
        dev.draw(Xs, np.zeros((7, 3)))
    grid = _hip.DeviceGrid(dev.ctx, Xs, 1)
    for call in (lambda: dev.path_weights(pp.Omega, pp.phase, pp.W, np.zeros((40, 3))),
                 lambda: dev.paths_eval(pp.Omega, pp.phase, pp.W, pp.V, Xs),
                 lambda: grid.paths(dev, pp.Omega, pp.phase, pp.W, pp.V)):
        with pytest.raises(_hip.HipError, match="not fitted") as err:
            call()
        assert str(err.value) == str(exact.value)
    with pytest.raises(ValueError, match="stale"):
        pp.paths(Xs)
    # the model refits at the values its objects hold, for the exact draw and for paths alike
    assert gp.posterior_samples_f(Xs, size=2).shape == (7, 1, 2)
    np.random.seed(3)
    again = gp.posterior_paths(size=3, features=5)
    assert again.paths(Xs).shape == before.shape
