"""Every device implementation of the expander flag against a reference MARGIN, flag by flag.

``flags[c, i]`` -- candidate c lifts some unsafe row above ``fmin_i`` (gp_opt.py:579-606) -- comes
out of ``pass_test`` (k_expander_many and its pruning tests), ``expander_check`` (k_expander for
2 .. 16 candidates, the filter / list pair for one, the probe with ``near_frac``),
``expander_batch``, ``expander_pass`` (flags folded into G) and ``expanders_small_all``
(step_small.hip); ``lipschitz_check`` / ``pass_lipschitz_test`` are the distance form.  The
reference is ``_expander_ref.margins``: ``best[c, i] = max over the unsafe rows of l2 - fmin_i``.

The decision band is MEASURED on the CPU, never taken from device output: a flag is asserted where
``|best| > band = max(100 D, 1e-9 sqrt(k(x, x)))``.  D = max |best_float64 - best_longdouble| over
the small cases (tests/test_expander_ref.py prints and bounds it):

    rbf_d1_n1 3.0e-14   m32_d2_n16_grid 7.6e-14   m52_d3_g3_inf 3.1e-13   prod_d3_n49 1.9e-13
    rbf_d2_one_safe 8.4e-12   m32_d1_one_row 6.0e-12   prod_d3_one_row 6.1e-15
                                                        -> D <= 1e-11, 100 D = 1e-9

so the floor decides: band = 1.3e-9 at variance 1.7 (1.08e-9 for the product kernel, 1.17).  The
factor 100 is room for the device's summation order (MFMA slots, split contraction) and its
2^(u/32) exponential; the floor is the band of the full_sets scenario in
test_gpu_expander_passes.py.  No entry of any case lies inside the band, every case has at least
10 % decided hits and 10 % decided non-hits (asserted again here before the device is touched;
for the candidates the device selects itself the margins are taken with ITS downloaded mean / var,
which are held to the project's 1e-9 bound against the oracle);
profiles/expander_flags/SUMMARY.txt has the counts per case.

Which form of MODE 1 runs cannot be read from Python.  An item is 16 listed rows x 4 groups and
goes one per workgroup while ``ceil(rows / 16) * ceil(groups / 4) <= kManyCoopItems = 1024``, else
``kManyChunk = 8`` groups per wave.  The cases of 129 candidates (9 groups -> 3 chunks) stay
cooperative up to 341 * 16 listed rows, i.e. always at ~1000 rows; ``m52_d2_n520_big`` has 4100
candidates = 257 groups -> 65 chunks and, by the reference, more than 2048 unsafe rows that some
candidate lifts (all of them are listed: the pruning tests are necessary conditions), so at least
128 * 65 = 8320 items > 1024: the per-wave form.
"""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _expander_ref as er

pytestmark = pytest.mark.gpu

BETA = er.BETA


@pytest.fixture(scope="module")
def mods(hip_device):
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    return safeopt_amd, gpy, _hip


class Dev(object):
    pass


@functools.lru_cache(maxsize=None)
def _device(name):
    """The device side of a case: GPs, grid, one confidence pass, S / mean / var downloaded."""
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    c = er.build_case(name)
    # the band cannot hide a failure: checked on the reference BEFORE the device is touched
    in_band, hits, non = er.shares(c)
    assert in_band <= 0.01 and hits >= 0.10 and non >= 0.10, (name, in_band, hits, non)
    dv = Dev()
    dv.c = c
    dv.gps = [gpy.models.GPRegression(X, Y, c.kernel(gpy.kern), noise_var=er.NOISE)
              for X, Y in zip(c.X, c.Y)]
    dv.devs = [g._fitted() for g in dv.gps]
    ctx = dv.devs[0].ctx
    dv.grid = _hip.DeviceGrid(ctx, c.pts, c.G)
    if c.axes_sides:
        assert dv.grid.set_axes(_hip.tensor_grid_axes(c.pts))
    dv.grid.confidence(dv.devs, BETA, c.fmin)
    dv.S = dv.grid.download(_hip.S)
    dv.mean = dv.grid.download(_hip.MEAN)
    dv.var = dv.grid.download(_hip.VAR)
    assert_array_equal(dv.S, c.S)                # (fmin lies in a gap of the lower bounds)
    # the project's bound on the posterior (tests/_gpu_common.py): 1e-9 of max |mean| / of k(x, x)
    dm, dvar = np.max(np.abs(dv.mean - c.mean)), np.max(np.abs(dv.var - c.var))
    print("%s: device posterior: |d mean| %.3g, |d var| %.3g" % (name, dm, dvar))
    assert dm < 1e-9 * np.max(np.abs(c.mean)) and dvar < 1e-9 * c.kdiag
    # The candidates the device selects itself carry ITS upper bounds: their margins are taken
    # with the downloaded mean / var, and the band conditions hold for them as well.
    dv.best_safe = None
    if c.best_safe is not None:
        dv.best_safe = er.safe_row_margins(c, dv.mean, dv.var)
        in_band, hits, non = er.shares(c, dv.best_safe)
        assert in_band <= 0.01 and (c.safe_rows.size == 1 or (hits >= 0.10 and non >= 0.10))
    # the candidates: safe rows through gather_rows, then the points off the grid
    parts = [dv.grid.gather_rows(c.rows[a:a + 4096]) for a in range(0, c.rows.size, 4096)]
    x, mean, var, Qr = [np.concatenate([p[j] for p in parts]) for j in range(4)] if parts else \
        dv.grid.gather_rows(c.rows)                 # (4096 rows per call)
    assert_array_equal(x, c.pts[c.rows])
    assert_array_equal(mean, dv.mean[:, c.rows].T)
    assert_array_equal(Qr[:, 1::2], mean + BETA * np.sqrt(var))
    dv.xc = np.concatenate([x, c.xc[c.rows.size:]])
    dv.mu_c, dv.u_c = c.mu_c, c.u_c             # (the operand u - mu of both sides)
    return dv


def check(c, flags, best, what):
    """``flags`` (K, G) against the margins on the decided entries; inactive columns are zero
    (``fill_fmin_active``: a GP with fmin = -inf has no operands and no scan: its flags stay as
    the entry point zeroed them).  Returns the number of entries compared."""
    flags = np.asarray(flags) != 0
    assert flags.shape == best.shape, (what, flags.shape, best.shape)
    assert not flags[:, ~c.active].any(), what
    dec, hit = er.decided(c, best)
    bad = np.argwhere(dec & (flags != hit))
    assert bad.size == 0, "%s: %s: %d decided flags differ, first (candidate, GP, margin): %s" % (
        c.name, what, len(bad), [(int(a), int(b), float(best[a, b])) for a, b in bad[:5]])
    return int(dec.sum())


@pytest.mark.parametrize("name", list(er.CASES))
def test_pass_test_against_the_margins(mods, name):
    dv = _device(name)
    c = dv.c
    for K in c.Ks:
        fl = dv.grid.pass_test(dv.devs, BETA, c.fmin, dv.xc[:K], (dv.u_c - dv.mu_c)[:K])
        n = check(c, fl, c.best[:K], "pass_test K = %d" % K)
        print("%s: pass_test K = %d: %d entries compared" % (name, K, n))
    if c.n_special:                               # 50 lengthscales from everything: never a hit
        assert not fl[-1].any()


@pytest.mark.parametrize("name", list(er.CASES))
def test_expander_check_in_sixteens_singly_and_probed(mods, name):
    dv = _device(name)
    c = dv.c
    K = min(c.xc.shape[0], 144)
    rows = np.r_[0:K - c.n_special, c.xc.shape[0] - c.n_special:c.xc.shape[0]]
    xc, mu, u, best = dv.xc[rows], dv.mu_c[rows], dv.u_c[rows], c.best[rows]
    f16 = np.concatenate([dv.grid.expander_check(dv.devs, BETA, c.fmin, xc[a:a + 16], mu[a:a + 16],
                                                 u[a:a + 16]) for a in range(0, len(rows), 16)])
    n16 = check(c, f16, best, "expander_check m <= 16")
    p16 = np.concatenate([dv.grid.expander_check(dv.devs, BETA, c.fmin, xc[a:a + 16], mu[a:a + 16],
                                                 u[a:a + 16], 0.5) for a in range(0, len(rows), 16)])
    # ragged m: slices of 5 and of 7 (m = 2 .. 15 otherwise occurs only as the tail of a case)
    for m in (5, 7):
        top = min(len(rows), 35)
        fm = np.concatenate([dv.grid.expander_check(dv.devs, BETA, c.fmin, xc[a:a + m], mu[a:a + m],
                                                    u[a:a + m]) for a in range(0, top, m)])
        check(c, fm, best[:top], "expander_check m = %d" % m)
    one = np.r_[0:min(24, len(rows)), len(rows) - c.n_special:len(rows)]
    f1 = np.concatenate([dv.grid.expander_check(dv.devs, BETA, c.fmin, xc[k], mu[k], u[k])
                         for k in one])
    n1 = check(c, f1, best[one], "expander_check m = 1")
    p1 = np.concatenate([dv.grid.expander_check(dv.devs, BETA, c.fmin, xc[k], mu[k], u[k], 0.5)
                         for k in one])
    # the probe is one-sided: a subset of the exact flags
    dec, hit = er.decided(c, best)
    assert not ((p16 != 0) & dec & ~hit).any() and not ((p1 != 0) & dec[one] & ~hit[one]).any()
    assert not p16[:, ~c.active].any() and not p1[:, ~c.active].any()
    # ... and the implementations agree with each other where the reference decides
    fp = dv.grid.pass_test(dv.devs, BETA, c.fmin, xc, u - mu)
    assert_array_equal((fp != 0)[dec], (f16 != 0)[dec])
    assert_array_equal((f1 != 0)[dec[one]], (f16[one] != 0)[dec[one]])
    print("%s: expander_check: %d entries in sixteens, %d singly" % (name, n16, n1))


@pytest.mark.parametrize("name", [k for k, v in er.CASES.items() if v["walk"]])
def test_device_selected_candidates(mods, name):
    """Every safe row as a candidate of the device's own selections: ``expanders_small_all``
    (where ``step_small_ok`` admits the shape), ``expander_batch`` walked to the end, and
    ``expander_pass(mode=1)`` in several passes, whose G is "every active GP certifies"
    (gp_opt.py:615) and empty outside S."""
    _, _, _hip = mods
    dv = _device(name)
    c, grid = dv.c, dv.grid
    safe, best = c.safe_rows, dv.best_safe
    N = c.pts.shape[0]
    n_cand, n_unsafe = grid.candidates(0.0, np.ones(c.G), np.zeros(c.G), True)
    assert (n_cand, n_unsafe) == (safe.size, N - safe.size)
    if grid.step_small_ok(dv.devs):
        assert max(g.n for g in dv.devs) <= 48 and N <= 16384
        rows, w, fl = grid.expanders_small_all(dv.devs, BETA, c.fmin)
        assert_array_equal(rows, safe)
        print("%s: expanders_small_all: %d entries" % (name, check(c, fl, best, "expanders_small_all")))
    else:
        assert max(g.n for g in dv.devs) > 48
    got_rows, got_flags, cut = [], [], -1
    while True:
        w, idx, fl = grid.expander_batch(dv.devs, BETA, c.fmin, 1, np.inf, cut, 16)
        got_rows.append(idx)
        got_flags.append(fl)
        if idx.size < 16:
            break
        cut = int(idx[-1])
    assert_array_equal(np.concatenate(got_rows), safe)       # (mode 1: ascending rows)
    n = check(c, np.concatenate(got_flags), best, "expander_batch")
    print("%s: expander_batch: %d entries in %d batches" % (name, n, len(got_rows)))
    # expander_pass, mode 1: the device marks the hits of every pass
    want = max(16, safe.size // 4 + 1)
    cut_w, tested, passes = np.inf, 0, 0
    while True:
        t, hits, key, row, left, amax = grid.expander_pass(dv.devs, BETA, c.fmin, 1, cut_w, -1,
                                                           -(float(N) + 1.0), 1.0, want)
        tested += t
        passes += 1
        if t == 0 or left == -np.inf:
            break
        cut_w = left
    assert tested == safe.size and (passes >= 2 or safe.size <= want)
    Gm = grid.download(_hip.G)
    assert not Gm[~c.S].any()
    dec, hit = er.decided(c, best)
    act = c.active[None, :]
    sure1 = np.all(hit | ~act, axis=1)
    sure0 = np.any(dec & ~hit, axis=1)
    assert_array_equal(Gm[safe][sure1], True)
    assert_array_equal(Gm[safe][sure0], False)
    print("%s: expander_pass mode 1: %d rows in %d passes, %d marked, %d compared" % (
        name, tested, passes, int(Gm.sum()), int(sure1.sum() + sure0.sum())))


@pytest.mark.parametrize("name", [k for k, v in er.CASES.items() if "lip" in v])
def test_lipschitz_flags(mods, name):
    """``lipschitz_check`` (m <= 16) and ``pass_lipschitz_test`` against the cdist formula; band
    1e-12 (|u| + L diameter): the kernels claim cdist's own summation order."""
    dv = _device(name)
    c = dv.c
    L, best, bnd = er.lipschitz_case(c)
    dec = (np.abs(best) > bnd) & c.active[None, :]
    hit = (best >= 0) & dec
    assert dec[:, c.active].mean() >= 0.99
    assert hit.sum() >= 0.1 * dec.sum() and dec.sum() - hit.sum() >= 0.1 * dec.sum()
    fmin = c.fmin
    # pass_lipschitz_test: ONE value per candidate in every column -- some row certifies every
    # active GP, which is "every GP has a row" since each comparison is monotone in the distance
    fl = dv.grid.pass_lipschitz_test(fmin, L, dv.xc, dv.u_c) != 0
    assert_array_equal(fl, np.repeat(fl[:, :1], c.G, axis=1))
    act = c.active[None, :]
    sure1 = np.all(hit | ~act, axis=1)
    sure0 = np.any(dec & ~hit, axis=1)
    assert_array_equal(fl[sure1, 0], True)
    assert_array_equal(fl[sure0, 0], False)
    K = min(64, dv.xc.shape[0])
    f16 = np.concatenate([dv.grid.lipschitz_check(fmin, L, dv.xc[a:a + 16], dv.u_c[a:a + 16])
                          for a in range(0, K, 16)]) != 0
    assert_array_equal(f16[dec[:K]], hit[:K][dec[:K]])
    assert not f16[:, ~c.active].any()          # (no constraint: the column stays zero)
    print("%s: lipschitz: %d entries, %d hits" % (name, int(dec.sum()), int(hit.sum())))


def test_no_unsafe_row(mods):
    """``np.any`` over no row is False (gp_opt.py:602): every flag is 0 and nothing is marked."""
    _, gpy, _hip = mods
    c = er.build_case("m52_d3_g3_inf")
    gps = [gpy.models.GPRegression(X, Y, c.kernel(gpy.kern), noise_var=er.NOISE)
           for X, Y in zip(c.X, c.Y)]
    devs = [g._fitted() for g in gps]
    grid = _hip.DeviceGrid(devs[0].ctx, c.pts, c.G)
    fmin = np.array([-50.0, -np.inf, -50.0])
    grid.confidence(devs, BETA, fmin)
    assert grid.download(_hip.S).all()
    K = 40
    xc, mu, u = c.xc[:K], c.mu_c[:K], c.u_c[:K]
    assert not grid.pass_test(devs, BETA, fmin, xc, u - mu).any()
    assert not grid.expander_check(devs, BETA, fmin, xc[:16], mu[:16], u[:16]).any()
    assert not grid.expander_check(devs, BETA, fmin, xc[0], mu[0], u[0]).any()
    assert not grid.lipschitz_check(fmin, np.ones(3), xc[:16], u[:16]).any()
    assert not grid.pass_lipschitz_test(fmin, np.ones(3), xc, u).any()
    n_cand, n_unsafe = grid.candidates(0.0, np.ones(3), np.zeros(3), True)
    assert (n_cand, n_unsafe) == (c.pts.shape[0], 0)
    t, hits, key, row, left, amax = grid.expander_pass(devs, BETA, fmin, 1, np.inf, -1,
                                                       -(float(c.pts.shape[0]) + 1.0), 1.0, 4096)
    assert t == c.pts.shape[0] and hits == 0
    assert not grid.download(_hip.G).any()


@pytest.mark.parametrize("name", ["m32_d1_one_row", "prod_d3_one_row", "m52_d2_n272_one_row"])
def test_block_bound_is_tight_for_a_candidate_on_the_row(mods, name):
    """Where the block test has no slack: ONE unsafe row in the wave, ONE candidate in the group,
    and the candidate IS the row -- ``c(x) = var(x) = sd(x) sd(x_c)``, the Cauchy-Schwarz bound of
    the block holds with equality.  The margin is linear in u (``c r / s2``), so u is set for
    margins just above and just below zero: a bound that prunes a little too much (0.9 of it)
    loses the hits.  One observation block and one part: the block tests; a product of two parts
    and n = 272: the PAIR test, which with a single listed row is all that keeps the pair."""
    dv = _device(name)
    c = dv.c
    go, x = c.gos[0], c.pts[:1]
    mu, var = [a[0, 0] for a in go.predict_noiseless(x)]
    # fmin beyond what the smaller variance alone can give (beta sd): the mean has to rise, u - mu
    # is positive and |delta| c in the bound is what the pair really adds
    fmin = np.array([mu - BETA * np.sqrt(var) + 1.5 * BETA * np.sqrt(var)])
    m0, _ = er.margins(go, c.U, x, [0.0], BETA, fmin[0])
    m1, _ = er.margins(go, c.U, x, [1.0], BETA, fmin[0])
    for want in (1e-2, 1e-4, 1e-6, -1e-6, -1e-4, -1e-2):
        u = (want - m0[0]) / (m1[0] - m0[0])
        assert u > mu
        best, _ = er.margins(go, c.U, x, [u], BETA, fmin[0])
        assert abs(best[0] - want) < 1e-9 and abs(best[0]) > er.band(c)
        fl = dv.grid.pass_test(dv.devs, BETA, fmin, x, [[u - mu]])
        assert bool(fl[0, 0]) == (want > 0), (want, fl)
        f1 = dv.grid.expander_check(dv.devs, BETA, fmin, x, [[mu]], [[u]])
        assert bool(f1[0, 0]) == (want > 0), (want, f1)


@pytest.mark.parametrize("name", ["m32_d3_n272", "m52_d8_n256", "m32_d2_n16_grid"])
def test_bounds_are_tight_for_a_full_group_on_an_unsafe_row(mods, name):
    """``_expander_ref.tight_group``: 16 candidates on the unsafe row closest to fmin, margins
    +-1e-6 .. +-1e-2, where Cauchy-Schwarz holds with equality -- d = 3 Matern32 with ARD ratio 5
    and n = 272 (the pair test), d = 8 at n = 256 (the row-level block test), a tensor grid.  Through
    the pass kernels, the 16-candidate scan and the one-candidate filter / list."""
    dv = _device(name)
    xs, mu, u, fmin, best = er.tight_group(name)
    want = best > 0
    fl = dv.grid.pass_test(dv.devs, BETA, fmin, xs, (u - mu)[:, None])
    assert_array_equal(fl[:, 0] != 0, want)
    f16 = dv.grid.expander_check(dv.devs, BETA, fmin, xs, mu[:, None], u[:, None])
    assert_array_equal(f16[:, 0] != 0, want)
    f1 = np.concatenate([dv.grid.expander_check(dv.devs, BETA, fmin, xs[k], mu[k], u[k])
                         for k in range(16)])
    assert_array_equal(f1[:, 0] != 0, want)
