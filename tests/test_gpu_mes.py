"""Max-value entropy search on the device (csrc/mes.hip; needs an MI355X): ``sgp_mes_eval``,
``sgp_grid_mes`` and ``SafeOpt.mes_point`` against tests/_mes_ref.py -- a 50-digit evaluation
of the definition and the float64 restatement of the device's stable form.

Tolerance of a term, per point, in units of ``EPS (1 + gamma^2 / 2)`` (for very negative gamma
the two parts of the term cancel from gamma^2 / 2 down to a logarithm): the restatement's own
maximum over the points of the test is measured against mpmath IN the test, and the device is
allowed 4 times that -- its erfcx / exp / log are a few ulp each where SciPy's and NumPy's are
at most one; the factor covers three such calls and the division.  Both maxima are printed, and
written to the file ``SAFEOPT_MES_PARITY_OUT`` names when it is set (profiles/mes/parity.txt
was taken that way).  Tolerance of alpha against the restatement on the SAME (mean, var,
ystar, floor): the same ``4 host_max``, in the unit ``EPS mean_k (1 + gamma_k^2 / 2)`` -- gamma
has the same bits on both sides (IEEE subtraction, square root and division), each of the K
terms differs by at most its own tolerance, and both sides add them in the same order; the
largest difference in that unit is printed and recorded like the figures of the terms.
Everything else is equality: bits of a row against the same row elsewhere, arg-max, floor.

The grids (tests/_mes_problems.py): 1000 rows (four workgroups, the last ragged) and 70 x 70
(twenty).  The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _mes_problems as P
import _mes_ref as ref
from _gpu_common import build_opt, mods                                     # noqa: F401

pytestmark = pytest.mark.gpu

FACTOR = 4.0


@pytest.fixture(scope="module")
def ctx(hip_device):
    from safeopt_amd import _hip
    return _hip.Context.default()


@functools.lru_cache(maxsize=None)
def _sweep():
    """gamma of test 1 (with both zeros), the 50-digit values, the restatement's error."""
    g = np.concatenate([ref.gamma_set(), [0.0, -0.0]])
    exact = ref.term_mp(g)
    return g, exact, ref.units(ref.term(g), g, exact)


def _check_alpha(what, got, mean, var, ystar, floor):
    """alpha against the restatement on the same inputs: within test 1's tolerance, 4 x the
    restatement's own maximum over the points of test 1, in the mean unit of the row."""
    host_max = _sweep()[2].max()
    sig = np.sqrt(np.maximum(var, 1e-15))
    unit = ref.EPS * np.mean([1.0 + 0.5 * ((max(y, floor) - mean) / sig) ** 2 for y in ystar],
                             axis=0)
    u = np.abs(got - ref.alpha(mean, var, ystar, floor)) / unit
    _record("%s, K = %d, %d rows: max |device - restatement| = %.3f units of EPS mean_k "
            "(1 + g_k^2 / 2) (allowed %.3f)" % (what, len(ystar), got.size, u.max(),
                                                  FACTOR * host_max))
    assert u.max() <= FACTOR * host_max


def _record(line):
    print(line)
    out = os.environ.get("SAFEOPT_MES_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


# ---- 1. term by term ---------------------------------------------------------------------------

def test_term_against_mpmath(ctx):
    g, exact, host_u = _sweep()
    one, zero = np.ones(1), np.zeros(1)
    got = np.array([ctx.mes_eval(zero, one, [y])[0] for y in g])     # K = 1, mean 0, var 1
    dev_u = ref.units(got, g, exact)
    _record("var = 1: %d points of gamma in [-40, 40]; max error in units of EPS (1 + g^2 / 2): "
            "host restatement %.3f, device %.3f (allowed %.3f)"
            % (g.size, host_u.max(), dev_u.max(), FACTOR * host_u.max()))
    assert np.all(np.isfinite(got))
    assert np.all(got[g >= 0] >= 0.0)
    assert dev_u.max() <= FACTOR * host_u.max()
    # the same points as the rows of ONE call: (0 - (-g)) / 1 = g, the same bits
    assert_array_equal(ctx.mes_eval(-g, np.ones_like(g), [0.0]), got)


@pytest.mark.parametrize("var", [1e-15, 1e-30, 1e6])
def test_term_at_other_variances(ctx, var):
    sigma = np.sqrt(max(var, 1e-15))                                  # 1e-30 is clipped
    ys = np.concatenate([np.linspace(-40.0, 40.0, 321), [0.0, -0.0]]) * sigma
    g = ys / sigma                                                    # as the device forms it
    exact = ref.term_mp(g)
    host_u = ref.units(ref.term(g), g, exact)
    got = np.array([ctx.mes_eval(np.zeros(1), np.full(1, var), [y])[0] for y in ys])
    dev_u = ref.units(got, g, exact)
    _record("var = %g: %d points; host restatement %.3f, device %.3f (allowed %.3f)"
            % (var, g.size, host_u.max(), dev_u.max(), FACTOR * host_u.max()))
    assert np.all(np.isfinite(got)) and np.all(got[g >= 0] >= 0.0)
    assert dev_u.max() <= FACTOR * host_u.max()


# ---- 2. the mean over K, in order --------------------------------------------------------------

NS = (1, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("K", [1, 2, 16, 64])
def test_rows_do_not_depend_on_launch(ctx, K):
    rng = np.random.default_rng(100 + K)
    mean = rng.normal(size=1000)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(4.0), size=1000))
    ystar = rng.normal(1.0, 1.5, size=K)
    floor = 0.4
    full = ctx.mes_eval(mean, var, ystar, floor)
    _check_alpha("sgp_mes_eval", full, mean, var, ystar, floor)
    for N in NS:
        assert_array_equal(ctx.mes_eval(mean[:N], var[:N], ystar, floor), full[:N])
        perm = rng.permutation(1000)[:N]
        assert_array_equal(ctx.mes_eval(mean[perm], var[perm], ystar, floor), full[perm])
        assert_array_equal(ctx.mes_eval(mean[:N], var[:N], ystar, np.inf), np.zeros(N))
    # no floor: the floor argument at -inf and a floor below every maximum agree
    assert_array_equal(ctx.mes_eval(mean, var, ystar), ctx.mes_eval(mean, var, ystar, -1e9))


@pytest.mark.parametrize("ystar", [[], list(range(65)), [0.5, float("nan")], [float("inf")]],
                         ids=["K=0", "K=65", "nan", "inf"])
def test_bad_maxima_are_refused_with_nothing_written(ctx, ystar):
    import ctypes as C
    from safeopt_amd import _hip
    mean, var = np.zeros(5), np.ones(5)
    out = np.full(5, -7.0)
    ys = np.asarray(ystar, dtype=np.float64)
    rc = _hip.lib().sgp_mes_eval(ctx.h, _hip.dptr(mean), _hip.dptr(var), 5, _hip.dptr(ys),
                                 int(ys.size), -np.inf, _hip.dptr(out))
    assert rc != 0 and np.all(out == -7.0)
    with pytest.raises(_hip.HipError):
        ctx.mes_eval(mean, var, ys)
    # N = 0: nothing to do, nothing written
    assert _hip.lib().sgp_mes_eval(ctx.h, _hip.dptr(mean), _hip.dptr(var), 0, _hip.dptr(mean),
                                   1, -np.inf, _hip.dptr(out)) == 0
    assert np.all(out == -7.0)


# ---- 3. the grid -------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["line", "plane"])
def grid(request, mods, ctx):
    """An optimiser after ``optimize()``, with what the device holds: posterior of GP 0 and
    masks.  The tests of this module leave ``S`` on the device as they found it."""
    from safeopt_amd import _hip
    z, meta = P.problem(request.param)
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    be = opt._backend
    state = dict(name=request.param, opt=opt, be=be, N=z["parameter_set"].shape[0],
                 mean=be.download(_hip.MEAN)[0].copy(), var=be.download(_hip.VAR)[0].copy(),
                 S=np.array(be.download(_hip.S)), M=np.array(be.download(_hip.M)),
                 G=np.array(be.download(_hip.G)))
    assert state["S"].any() and not state["S"].all() and (state["M"] | state["G"]).any()
    return state


def _ystar(K=16, seed=5):
    return np.random.default_rng(seed).normal(2.0, 0.7, size=K)


def test_grid_alpha_is_eval_alpha(grid, ctx):
    from safeopt_amd import _hip
    ystar = _ystar()
    al, v, i, fl = grid["be"].grid.mes(ystar, rows=_hip.MES_S, floor='mean', alpha=True)
    assert fl == grid["mean"][grid["S"]].max()
    assert_array_equal(al, ctx.mes_eval(grid["mean"], grid["var"], ystar, fl))
    _check_alpha("sgp_grid_mes (%s)" % grid["name"], al, grid["mean"], grid["var"], ystar, fl)
    # alpha = False: the same pick
    assert grid["be"].grid.mes(ystar, rows=_hip.MES_S, floor='mean')[1:] == (v, i, fl)


@pytest.mark.parametrize("rows", ["ALL", "S", "MG"])
@pytest.mark.parametrize("floor", ["mean", None, 2.25])
def test_grid_pick_is_first_maximum_over_the_mask(grid, rows, floor):
    from safeopt_amd import _hip
    mask = {"ALL": np.ones(grid["N"], dtype=bool), "S": grid["S"],
            "MG": grid["M"] | grid["G"]}[rows]
    al, v, i, fl = grid["be"].grid.mes(_ystar(), rows=getattr(_hip, "MES_" + rows), floor=floor,
                                       alpha=True)
    if floor == "mean":
        assert fl == (grid["mean"].max() if rows == "ALL" else grid["mean"][grid["S"]].max())
    else:
        assert fl == (-np.inf if floor is None else floor)
    assert np.all(np.isfinite(al))
    want = int(np.argmax(np.where(mask, al, -np.inf)))
    assert (v, i) == (al[want], want)


def test_empty_mask_has_no_pick(grid):
    from safeopt_amd import _hip
    be = grid["be"]
    try:
        be.upload_mask(_hip.S, np.zeros(grid["N"], dtype=bool))
        al, v, i, fl = be.grid.mes(_ystar(), rows=_hip.MES_S, floor='mean', alpha=True)
        assert (v, i, fl) == (-np.inf, -1, -np.inf) and np.all(np.isfinite(al))
    finally:
        be.upload_mask(_hip.S, grid["S"])


def test_grid_refuses_bad_arguments(grid):
    from safeopt_amd import _hip
    g = grid["be"].grid
    for bad in ([], np.zeros(65), [np.nan]):
        with pytest.raises(_hip.HipError):
            g.mes(bad)
    with pytest.raises(_hip.HipError):
        g.mes([1.0], rows=3)
    with pytest.raises(_hip.HipError):
        g.mes([1.0], floor=float("nan"))
    with pytest.raises(ValueError):
        g.mes([1.0], floor="max")


def test_grid_without_a_posterior_is_refused(ctx):
    from safeopt_amd import _hip
    g = _hip.DeviceGrid(ctx, np.linspace(0.0, 1.0, 10)[:, None], 1)
    with pytest.raises(_hip.HipError, match="no current posterior"):
        g.mes([1.0])


def test_new_context_columns_void_the_posterior(mods, ctx):
    """The rows change with the context: what a pass left in mean / var describes the old
    rows, and ``sgp_grid_mes`` refuses it until the next pass."""
    from safeopt_amd import _hip
    _, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("plane")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    dev = [gp._fitted()]
    g = _hip.DeviceGrid(ctx, z["parameter_set"][:300], 1)
    g.posterior(dev)
    assert g.mes([2.0], rows=_hip.MES_ALL, floor=None)[2] >= 0
    g.set_context([0.25])
    with pytest.raises(_hip.HipError, match="no current posterior"):
        g.mes([2.0], rows=_hip.MES_ALL, floor=None)
    g.posterior(dev)
    assert g.mes([2.0], rows=_hip.MES_ALL, floor=None)[2] >= 0


# ---- 4. ties -----------------------------------------------------------------------------------

def test_lowest_row_wins_a_tie_from_a_late_workgroup(grid):
    from safeopt_amd import _hip
    be, N = grid["be"], grid["N"]
    first = 256 * ((N - 1) // 256 - 1)               # first row of the last full workgroup
    mask = np.zeros(N, dtype=bool)
    mask[[first, first + 1, first + 300 if first + 300 < N else N - 1, N - 1]] = True
    try:
        be.upload_mask(_hip.S, mask)
        al, v, i, _ = be.grid.mes([1e6], rows=_hip.MES_S, floor=None, alpha=True)
        assert np.all(al == 0.0) and (v, i) == (0.0, first)
        # every row: row 0
        assert be.grid.mes([1e6], rows=_hip.MES_ALL, floor=None)[1:3] == (0.0, 0)
    finally:
        be.upload_mask(_hip.S, grid["S"])


def test_tie_on_a_shard_returns_the_global_row(grid, ctx):
    from safeopt_amd import _hip
    opt, N = grid["opt"], grid["N"]
    lo, hi = N // 3 + 5, N - 7                        # a shard that starts inside a workgroup
    dev = [g._fitted() for g in opt.gps]
    shard = _hip.DeviceGrid(ctx, opt.inputs[lo:hi], len(dev), global_offset=lo)
    shard.posterior(dev)
    mask = np.zeros(hi - lo, dtype=bool)
    mask[[300, 301, hi - lo - 1]] = True
    shard.upload_mask(_hip.S, mask)
    assert shard.mes([1e6], rows=_hip.MES_S, floor=None)[1:3] == (0.0, lo + 300)
    assert shard.mes([1e6], rows=_hip.MES_ALL, floor=None)[1:3] == (0.0, lo)
    # the shard's rows have the bits of the whole grid's rows
    ystar = _ystar()
    al = shard.mes(ystar, rows=_hip.MES_ALL, floor=2.0, alpha=True)[0]
    whole = grid["be"].grid.mes(ystar, rows=_hip.MES_ALL, floor=2.0, alpha=True)[0]
    assert_array_equal(shard.download(_hip.MEAN)[0], grid["mean"][lo:hi])
    assert_array_equal(al, whole[lo:hi])


# ---- 5. mes_point end to end -------------------------------------------------------------------

def _state(opt):
    from safeopt_amd import _hip
    be = opt._backend
    out = [np.array(be.download(w)) for w in (_hip.Q, _hip.S, _hip.M, _hip.G, _hip.MEAN,
                                              _hip.VAR)]
    out.extend(np.array(a) for a in opt.gp._fitted().factor())
    return out


def test_mes_point_end_to_end(grid):
    opt, S = grid["opt"], grid["S"]
    ids = np.flatnonzero(S)
    sig = np.sqrt(grid["var"])
    smallest = ids[sig[S] == sig[S].min()]
    before = _state(opt)
    for seed in P.SEEDS[grid["name"]]:
        np.random.seed(seed)
        x, a, values, ystar = opt.mes_point(paths=P.PATHS, features=P.FEATURES,
                                            return_values=True)
        np.random.seed(seed)
        x2, a2 = opt.mes_point(paths=P.PATHS, features=P.FEATURES)
        assert_array_equal(x2, x)
        assert a2 == a and values.shape == (grid["N"],) and ystar.shape == (P.PATHS,)
        # the arg-max of the restatement on the downloaded posterior and the returned maxima
        floor = grid["mean"][S].max()
        want = ref.alpha(grid["mean"], grid["var"], ystar, floor)
        assert P.top_two_gap(want, S) > 1e-9
        row = ids[np.argmax(want[S])]
        assert S[row] and row not in smallest
        assert_array_equal(x, opt.inputs[row])
        assert a == values[row] == values[S].max()
        # candidates M | G: a row of M | G, the same alpha array
        np.random.seed(seed)
        x3, a3, values3, _ = opt.mes_point(paths=P.PATHS, features=P.FEATURES, within='MG',
                                           return_values=True)
        mg = grid["M"] | grid["G"]
        assert_array_equal(values3, values)
        assert_array_equal(x3, opt.inputs[np.argmax(np.where(mg, values, -np.inf))])
        # no mask at all: maxima and floor over every row
        np.random.seed(seed)
        x4, a4, values4, ystar4 = opt.mes_point(paths=P.PATHS, features=P.FEATURES,
                                                within='all', return_values=True)
        assert np.all(ystar4 >= ystar) and a4 == values4.max()
    for u, w in zip(before, _state(opt)):
        assert_array_equal(u, w)


def test_the_floor_keeps_the_pick_off_the_incumbent(grid):
    """Maxima below the mean, no floor: gamma < 0, the terms grow like gamma^2 / 2 and the pick
    is the row of S with the smallest sigma.  The floor undoes it."""
    from safeopt_amd import _hip
    S = grid["S"]
    ids = np.flatnonzero(S)
    sig = np.sqrt(grid["var"])
    smallest = ids[np.argmin(sig[S])]
    low = np.full(P.PATHS, grid["mean"][S].min() - 50.0)
    g = grid["be"].grid
    assert g.mes(low, rows=_hip.MES_S, floor=None)[2] == smallest
    al, v, i, fl = g.mes(low, rows=_hip.MES_S, floor='mean', alpha=True)
    assert i != smallest and S[i] and fl == grid["mean"][S].max()
    assert np.all(al[S] <= np.log(2.0))              # gamma >= 0 on every candidate


def test_mes_point_without_a_safe_row(mods):
    z, meta = P.problem("line")
    opt = build_opt(mods, z, meta, 0)
    opt.optimize()
    opt.S[:] = False
    np.random.seed(1)
    with pytest.raises(RuntimeError, match="no safe points"):
        opt.mes_point(paths=4, features=32)


def test_max_value_entropy_of_a_gp(mods, ctx):
    """``GPRegression.max_value_entropy``: predict_noiseless, then sgp_mes_eval."""
    _, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("plane")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    X = z["parameter_set"][::37]
    ystar = _ystar(K=8)
    a = gp.max_value_entropy(X, ystar, floor=1.5)
    mean, var = gp.predict_noiseless(X)
    assert a.shape == (X.shape[0], 1)
    assert_array_equal(a, ctx.mes_eval(mean, var, ystar, 1.5))
    assert_array_equal(gp.max_value_entropy(X, ystar), ctx.mes_eval(mean, var, ystar))
