"""The candidate selection of ``SafeOpt.ise_point`` on the device (csrc/ise.hip:
``sgp_grid_ise_keys`` / ``_hist`` / ``_list``) and the candidates by value (``sgp_grid_ise_at``),
on one rank (needs an MI355X).

The device's keys against NumPy's over all safe rows: the measured error, in the unit of
``gp_opt.ISE_KEY_EPS`` (``max(1, largest key)``), must stay below a QUARTER of the bound the
superset argument of ``gp_opt.ise_threshold`` relies on -- the bound is reasoned in gp_opt.py
(ulp counts of a quotient, a log1p and at most eight additions), not read off this measurement.
Each measured value is printed, and appended to the file ``SAFEOPT_ISE_SELECT_OUT`` names when it
is set (profiles/ise_select/SUMMARY.txt was taken that way).  Everything else is equality: the
histogram against a NumPy histogram of the DEVICE keys, the list row by row, ``ise_point``'s rows
against ``gp_opt.ise_candidates`` on the downloaded state, ``sgp_grid_ise_at`` against
``sgp_grid_ise``.  The file also passes with ``SGP_POISON=1`` and ``=2`` in front of it.
"""
import ctypes as C
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _mes_problems as P
from _gpu_common import build_opt, mods                                     # noqa: F401

pytestmark = pytest.mark.gpu

INF = np.inf


def _record(line):
    print(line)
    out = os.environ.get("SAFEOPT_ISE_SELECT_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _two_gp_problem(fmin):
    """``plane`` with a second GP: other values at the same inputs (the optimiser's GPs share
    them), another kernel and another noise."""
    z, meta = P.problem("plane")
    X = z["it0_X0"]
    Y = P._smooth(X, 43)
    z = dict(z, it0_X1=X, it0_Y1=Y - Y.min() + 0.4, beta_all=np.array([P.BETA]))
    spec = [dict(kind="RBF", input_dim=2, variance=0.9, lengthscale=[0.5, 0.8], ARD=True,
                 active_dims=[0, 1])]
    meta = dict(meta, kernels=meta["kernels"] + [spec], noise_vars=[P.NOISE, 0.2 ** 2],
                fmin=list(fmin))
    return z, meta


PROBLEMS = ("line", "plane", "two", "two-one-inactive")
_OPTS = {}


def _problem_opt(mods, name):
    """The optimiser of a problem after one ``optimize()``, built once per module."""
    if name not in _OPTS:
        if name in ("line", "plane"):
            z, meta = P.problem(name)
        else:
            z, meta = _two_gp_problem([0.0, -0.5] if name == "two" else [0.0, -INF])
        opt = build_opt(mods, z, meta, 0)
        opt.optimize()
        _OPTS[name] = opt
    return _OPTS[name]


def _state(opt):
    """``(var (G, N), S, s, active, fmin)`` from the device, as the host selection reads them."""
    from safeopt_amd import _hip
    be = opt._backend
    var, S = np.array(be.download(_hip.VAR)), np.array(be.download(_hip.S), dtype=bool)
    fmin = np.asarray(opt.fmin, dtype=float).reshape(-1)
    s = np.array([float(g.noise_var) + 1e-8 for g in opt.gps])
    return var, S, s, np.isfinite(fmin), fmin


def _np_keys(var, s, active):
    key = np.zeros(var.shape[1])
    for g in np.flatnonzero(active):
        key = key + 0.5 * np.log1p(var[g] / s[g])
    return key


def _device_keys(opt):
    """Every safe row with its device key: the list entry with ``thr = -inf``."""
    be = opt._backend
    fmin = np.asarray(opt.fmin, dtype=float).reshape(-1)
    return be.grid.ise_list(be._dev(), fmin, -INF, be.grid.N)


def _bins(key, lo, hi):
    """The rule of ``k_pass_hist`` / ``k_ise_hist``."""
    return np.clip(((key - lo) * (4096.0 / (hi - lo))).astype(np.int64), 0, 4095)


# ---- 1. keys, histogram, list -----------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_device_keys_against_numpy(mods, name):
    from safeopt_amd import gp_opt
    opt = _problem_opt(mods, name)
    be = opt._backend
    var, S, s, active, fmin = _state(opt)
    assert 0 < S.sum() < S.size and (name != "two-one-inactive" or active.tolist() == [True, False])
    count, rows, dkey, x, v = _device_keys(opt)
    assert count == S.sum()
    assert_array_equal(rows, np.flatnonzero(S))
    # x / var: the bits of the resident arrays
    assert_array_equal(x, opt.inputs[rows])
    assert_array_equal(v, var[:, rows].T)
    key = _np_keys(var, s, active)[rows]
    err = np.max(np.abs(dkey - key)) / max(1.0, key.max())
    _record("%-16s %5d safe rows, keys in [%.6g, %.6g]: max |device key - NumPy key| = %.3e "
            "max(1, key) = %.3f ISE_KEY_EPS (allowed 0.25)"
            % (name, count, key.min(), key.max(), err, err / gp_opt.ISE_KEY_EPS))
    assert err <= gp_opt.ISE_KEY_EPS / 4
    # count, min and max are those of the device keys
    assert be.grid.ise_keys(be._dev(), fmin) == (count, dkey.min(), dkey.max())


@pytest.mark.parametrize("name", PROBLEMS)
def test_histogram_bin_by_bin(mods, name):
    opt = _problem_opt(mods, name)
    be = opt._backend
    fmin = np.asarray(opt.fmin, dtype=float).reshape(-1)
    count, _rows, dkey, _x, _v = _device_keys(opt)
    lo, hi = dkey.min(), dkey.max()
    # the whole range, and one that clamps keys at both ends
    for a, b in ((lo, hi), (lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo))):
        h = be.grid.ise_hist(be._dev(), fmin, a, b)
        assert h.dtype == np.uint32 and h.sum() == count
        assert_array_equal(h, np.bincount(_bins(dkey, a, b), minlength=4096))


@pytest.mark.parametrize("name", PROBLEMS)
def test_list_row_by_row(mods, name):
    from safeopt_amd import _hip
    opt = _problem_opt(mods, name)
    be = opt._backend
    grid, devs = be.grid, be._dev()
    var, S, _s, _active, fmin = _state(opt)
    count, rows, dkey, x, v = _device_keys(opt)
    for q in (0.0, 0.5, 0.97, 1.0):
        thr = float(np.quantile(dkey, q))
        n, r2, k2, x2, v2 = grid.ise_list(devs, fmin, thr, grid.N)
        keep = dkey >= thr
        assert n == keep.sum() and n >= 1
        assert_array_equal(r2, rows[keep])                    # ascending global row
        assert_array_equal(k2, dkey[keep])
        assert_array_equal(x2, x[keep])
        assert_array_equal(v2, v[keep])
    assert grid.ise_list(devs, fmin, np.nextafter(dkey.max(), INF), grid.N)[0] == 0
    # cap below the count: the full count, and nothing written behind cap rows
    d, G, cap = grid.d, grid.G, 5
    gi, ky = np.full(count, -7, dtype=np.int64), np.full(count, -7.0)
    xo, vo = np.full((count, d), -7.0), np.full((count, G), -7.0)
    n = C.c_int64(-7)
    rc = _hip.lib().sgp_grid_ise_list(
        grid.h, _hip._gp_array(devs), G, _hip.dptr(fmin), -INF, cap, C.byref(n),
        gi.ctypes.data_as(_hip.c_i64_p), _hip.dptr(ky), _hip.dptr(xo), _hip.dptr(vo))
    assert rc == 0 and n.value == count > cap
    assert_array_equal(gi[:cap], rows[:cap])
    assert_array_equal(ky[:cap], dkey[:cap])
    assert_array_equal(xo[:cap], x[:cap])
    assert_array_equal(vo[:cap], v[:cap])
    assert np.all(gi[cap:] == -7) and np.all(ky[cap:] == -7.0)
    assert np.all(xo[cap:] == -7.0) and np.all(vo[cap:] == -7.0)
    # S and var are only read
    assert_array_equal(np.array(be.download(_hip.S), dtype=bool), S)
    assert_array_equal(np.array(be.download(_hip.VAR)), var)


def test_a_shard_lists_global_rows(mods):
    from safeopt_amd import _hip
    opt = _problem_opt(mods, "plane")
    be = opt._backend
    from safeopt_amd import gp_opt
    _var, S, s, active, fmin = _state(opt)
    lo, hi = 1225, 2450 + 37                              # starts and ends inside a workgroup
    shard = _hip.DeviceGrid(be.ctx, opt.inputs[lo:hi], 1, global_offset=lo)
    shard.posterior(be._dev())
    shard.upload_mask(_hip.S, S[lo:hi])
    var = np.array(shard.download(_hip.VAR))
    rows = lo + np.flatnonzero(S[lo:hi])
    n, r2, k2, x2, v2 = shard.ise_list(be._dev(), fmin, -INF, hi - lo)
    assert n == rows.size > 0
    assert_array_equal(r2, rows)
    assert_array_equal(x2, opt.inputs[rows])
    assert_array_equal(v2, var[:, rows - lo].T)
    key = _np_keys(var, s, active)[rows - lo]
    assert np.max(np.abs(k2 - key)) / max(1.0, key.max()) <= gp_opt.ISE_KEY_EPS / 4
    thr = float(np.median(k2))
    n3, r3, k3, _x3, _v3 = shard.ise_list(be._dev(), fmin, thr, hi - lo)
    assert n3 == (k2 >= thr).sum()
    assert_array_equal(r3, rows[k2 >= thr])
    assert_array_equal(k3, k2[k2 >= thr])
    assert shard.ise_keys(be._dev(), fmin) == (n, k2.min(), k2.max())
    h = shard.ise_hist(be._dev(), fmin, k2.min(), k2.max())
    assert_array_equal(h, np.bincount(_bins(k2, k2.min(), k2.max()), minlength=4096))
    # a shard without a safe row
    shard.upload_mask(_hip.S, np.zeros(hi - lo, dtype=bool))
    assert shard.ise_keys(be._dev(), fmin) == (0, INF, -INF)
    assert shard.ise_list(be._dev(), fmin, -INF, 10)[0] == 0
    assert not shard.ise_hist(be._dev(), fmin, 0.0, 1.0).any()


def test_refusals_leave_the_outputs_untouched(mods):
    from safeopt_amd import _hip
    opt = _problem_opt(mods, "line")
    be = opt._backend
    grid, devs = be.grid, be._dev()
    fmin = np.asarray(opt.fmin, dtype=float).reshape(-1)
    fresh = _hip.DeviceGrid(be.ctx, opt.inputs[:50], 1)          # no pass has swept it
    two = _hip.DeviceGrid(be.ctx, opt.inputs[:50], 2)
    lib, d = _hip.lib(), _hip.dptr
    i64 = lambda a: a.ctypes.data_as(_hip.c_i64_p)                       # noqa: E731
    no = np.array([-INF])

    def keys(g, gps, fm):
        n, lo, hi = C.c_int64(-7), C.c_double(-7.0), C.c_double(-7.0)
        rc = lib.sgp_grid_ise_keys(g.h, _hip._gp_array(gps), len(gps), d(fm), C.byref(n),
                                   C.byref(lo), C.byref(hi))
        return rc, (n.value, lo.value, hi.value) == (-7, -7.0, -7.0)

    def hist(g, gps, fm, a=0.0, b=1.0):
        h = np.full(4096, 7, dtype=np.uint32)
        rc = lib.sgp_grid_ise_hist(g.h, _hip._gp_array(gps), len(gps), d(fm), a, b,
                                   h.ctypes.data_as(_hip.c_u32_p))
        return rc, bool(np.all(h == 7))

    def lst(g, gps, fm, thr=-INF, cap=20):
        gi, ky = np.full(20, -7, dtype=np.int64), np.full(20, -7.0)
        xo, vo = np.full((20, g.d), -7.0), np.full((20, g.G), -7.0)
        n = C.c_int64(-7)
        rc = lib.sgp_grid_ise_list(g.h, _hip._gp_array(gps), len(gps), d(fm), thr, cap,
                                   C.byref(n), i64(gi), d(ky), d(xo), d(vo))
        return rc, bool(n.value == -7 and np.all(gi == -7) and np.all(ky == -7.0)
                        and np.all(xo == -7.0) and np.all(vo == -7.0))

    def at(g, gps, fm, cand, K, about=_hip.ISE_UNSAFE):
        cand = np.ascontiguousarray(cand, dtype=np.int64)
        xc, vx = np.zeros((max(K, 1), g.d)), np.ones((g.G, max(K, 1)))
        al, tg = np.full(max(K, 1), -7.0), np.full(max(K, 1), -7, dtype=np.int64)
        v, i = C.c_double(-7.0), C.c_int64(-7)
        rc = lib.sgp_grid_ise_at(g.h, _hip._gp_array(gps), len(gps), d(fm), i64(cand), d(xc),
                                 d(vx), K, about, d(al), i64(tg), C.byref(v), C.byref(i))
        return rc, bool(np.all(al == -7.0) and np.all(tg == -7) and v.value == -7.0
                        and i.value == -7)

    refused = []
    for what, call in (("keys", keys), ("hist", hist), ("list", lst)):
        refused += [(what + ": no active GP", call(grid, devs, no)),
                    (what + ": no posterior", call(fresh, devs, fmin)),
                    (what + ": G of the grid", call(two, devs, fmin))]
    refused += [("hist: empty range", hist(grid, devs, fmin, 1.0, 1.0)),
                ("hist: reversed range", hist(grid, devs, fmin, 2.0, 1.0)),
                ("hist: infinite range", hist(grid, devs, fmin, 0.0, INF)),
                ("list: NaN threshold", lst(grid, devs, fmin, thr=float("nan"))),
                ("list: negative cap", lst(grid, devs, fmin, cap=-1)),
                ("at: K = 0", at(grid, devs, fmin, [3], 0)),
                ("at: K = 4097", at(grid, devs, fmin, np.zeros(4097), 4097)),
                ("at: about", at(grid, devs, fmin, [3], 1, about=2)),
                ("at: negative row", at(grid, devs, fmin, [-1], 1)),
                ("at: no active GP", at(grid, devs, no, [3], 1)),
                ("at: no posterior", at(fresh, devs, fmin, [3], 1)),
                ("at: G of the grid", at(two, devs, fmin, [3], 1))]
    for what, (rc, clean) in refused:
        assert rc != 0, what
        assert clean, what
    with pytest.raises(_hip.HipError, match="no current posterior"):
        fresh.ise_keys(devs, fmin)
    with pytest.raises(_hip.HipError, match="empty key range"):
        grid.ise_hist(devs, fmin, 1.0, 1.0)
    # ... and the grid still answers
    for call in (keys, hist, lst):
        rc, clean = call(grid, devs, fmin)
        assert rc == 0 and not clean
    rc, clean = at(grid, devs, fmin, [3], 1)
    assert rc == 0 and not clean


# ---- 2. ise_point selects on the device --------------------------------------------------------
class _CountDownloads(object):
    """Wraps ``DeviceGrid.download`` of an optimiser's grid: what was asked for."""

    def __init__(self, opt):
        self.grid, self.inner, self.asked = opt._backend.grid, opt._backend.grid.download, []

    def __enter__(self):
        self.grid.download = lambda what, out=None: (self.asked.append(what)
                                                     or self.inner(what, out))
        return self

    def __exit__(self, *exc):
        del self.grid.download


@pytest.mark.parametrize("name", ["line", "plane", "two"])
def test_ise_point_rows_are_the_host_selection(mods, name):
    from safeopt_amd import _hip, gp_opt
    opt = _problem_opt(mods, name)
    var, S, s, active, _fmin = _state(opt)
    nS = int(S.sum())
    for about in ("unsafe", "all"):
        for K in (1, 7, 40, 64, 65, nS, nS + 5):
            if K > _hip.MAX_ISE:
                continue
            with _CountDownloads(opt) as dl:
                x, a, rows, values, targets = opt.ise_point(candidates=K, about=about,
                                                            return_values=True)
            assert opt._ise_path == 'device', (K, opt._ise_path)
            assert _hip.VAR not in dl.asked and _hip.S not in dl.asked
            assert_array_equal(rows, gp_opt.ise_candidates(var, S, s, active, K))
            assert rows.dtype == np.int64 and rows.size == min(K, nS)
            assert a == values.max() and S[np.flatnonzero(np.all(opt.inputs == x, axis=1))[0]]


def _opt_on(mods, params):
    """``line``'s GP over another parameter set, intervals and safe set computed."""
    safeopt_amd, gpy, _, _ = mods
    from _golden import make_kernel
    z, meta = P.problem("line")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    opt = safeopt_amd.SafeOpt(gp, params, P.FMIN, beta=P.BETA, threshold=0.1)
    opt.update_confidence_intervals()
    opt.compute_safe_set()
    return opt


def test_exact_ties_take_the_lower_row(mods):
    from safeopt_amd import gp_opt
    base = np.linspace(-3.0, 3.0, 300)[:, None]
    opt = _opt_on(mods, np.repeat(base, 3, axis=0))             # every row three times
    var, S, s, active, _fmin = _state(opt)
    assert 0 < S.sum() < S.size
    assert_array_equal(var[:, 0::3], var[:, 1::3])              # (the keys tie exactly)
    assert_array_equal(var[:, 0::3], var[:, 2::3])
    for K in (1, 2, 4, 40, 41):
        rows = opt.ise_point(candidates=K, return_values=True)[2]
        assert opt._ise_path == 'device'
        assert_array_equal(rows, gp_opt.ise_candidates(var, S, s, active, K))
        # a triple is taken from its lowest row up
        assert rows[0] % 3 == 0 and (K < 2 or rows[1] == rows[0] + 1)


def test_identical_rows_fall_back_to_the_host_selection(mods):
    from safeopt_amd import gp_opt
    z, _meta = P.problem("line")
    x0 = z["it0_X0"][np.argmax(z["it0_Y0"][:, 0])]
    opt = _opt_on(mods, np.tile(x0, (600, 1)))
    var, S, s, active, _fmin = _state(opt)
    assert S.all()                                               # (the best observation is safe)
    x, a, rows, values, targets = opt.ise_point(candidates=9, about='all', return_values=True)
    assert opt._ise_path == 'host: degenerate key range'
    assert_array_equal(rows, gp_opt.ise_candidates(var, S, s, active, 9))
    assert_array_equal(rows, np.arange(9))
    assert_array_equal(x, x0)
    with pytest.raises(RuntimeError, match="no row qualifies"):
        opt.ise_point(candidates=9)


# ---- 3. candidates by value ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plane", "two"])
def test_ise_at_with_resident_values_is_sgp_grid_ise(mods, name):
    from safeopt_amd import _hip, dist
    opt = _problem_opt(mods, name)
    be = opt._backend
    devs = be._dev()
    _var, S, _s, _active, fmin = _state(opt)
    N = S.size
    # (grids of this test's own, all swept by the same pass: the shards' posterior is the whole
    # grid's, row for row)
    grid = _hip.DeviceGrid(be.ctx, opt.inputs, len(devs))
    grid.posterior(devs)
    grid.upload_mask(_hip.S, S)
    var = np.array(grid.download(_hip.VAR))
    shards = []
    for lo, hi in ((0, 1000), (1000, 1000 + 1237), (2237, N)):
        shard = _hip.DeviceGrid(be.ctx, opt.inputs[lo:hi], len(devs), global_offset=lo)
        shard.posterior(devs)
        shard.upload_mask(_hip.S, S[lo:hi])
        assert_array_equal(np.array(shard.download(_hip.VAR)), var[:, lo:hi])
        shards.append(shard)
    rng = np.random.default_rng(3)
    for K in (1, 17, 65):
        cand = rng.choice(np.flatnonzero(S), size=K, replace=False)
        xc, vx = opt.inputs[cand], var[:, cand]
        for about in (_hip.ISE_UNSAFE, _hip.ISE_ALL):
            want = grid.ise(devs, fmin, cand, about=about)[:4]
            got = grid.ise_at(devs, fmin, cand, xc, vx, about=about)
            assert_array_equal(got[0], want[0])
            assert_array_equal(got[1], want[1])
            assert got[2:] == want[2:]
            # without a communicator the merged form is the same call
            again = grid.ise_at(devs, fmin, cand, xc, vx, about=about, comm=True)
            assert_array_equal(again[0], want[0])
            assert again[2:] == want[2:]
            # three uneven shards, each against ALL candidates: their merge is the whole grid's
            parts = [shard.ise_at(devs, fmin, cand, xc, vx, about=about) for shard in shards]
            al, tg = dist.merge_ise_records([p[0] for p in parts], [p[1] for p in parts])
            assert_array_equal(al, want[0])
            assert_array_equal(tg, want[1])
            assert dist.pick_ise(al, tg, cand) == want[2:]
