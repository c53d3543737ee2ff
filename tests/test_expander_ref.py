"""The margin reference of tests/_expander_ref.py against ``son.expander_hits_rank1``, the refit
form and its own long-double restatement, and the conditions under which the case matrix of
tests/test_gpu_expander_flags.py decides nearly every flag with both answers present (no GPU)."""
import numpy as np
import pytest

import _expander_ref as er
from oracle import gp_numpy as gpn
from oracle import safeopt_numpy as son


def small_problem(seed=3, n=12, N=200, K=20):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(n, 2))
    Y = er._smooth(X, seed) + 0.3
    gp = gpn.GPRegression(X, Y, gpn.Matern52(2, 1.7, [0.7, 1.9], ARD=True), noise_var=er.NOISE)
    pts = rng.uniform(-3, 3, size=(N, 2))
    Q = son.confidence_intervals([gp], pts, er.BETA)
    fmin = float(np.quantile(Q[:, 0], 0.5))
    S = son.safe_set(Q, [fmin])
    cand = np.flatnonzero(S)[:K]
    return gp, pts, Q, S, cand, fmin


def test_sign_of_the_margin_is_expander_hits_rank1():
    for name in ("m52_d3_g3_inf", "prod_d3_n49", "rbf_d2_n257_grid"):
        c = er.build_case(name)
        inputs = np.concatenate([c.U, c.xc])
        unsafe = np.arange(inputs.shape[0]) < c.U.shape[0]
        cand = np.arange(c.U.shape[0], inputs.shape[0])
        for i in np.flatnonzero(c.active):
            hits = son.expander_hits_rank1(c.gos[i], inputs, unsafe, cand, c.u_c[:, i], er.BETA,
                                           c.fmin[i])
            clear = np.abs(c.best[:, i]) > 1e-12
            assert clear.sum() >= cand.size - 2
            np.testing.assert_array_equal(hits[clear], (c.best[:, i] >= 0)[clear])
            assert hits.any() and not hits.all()


def test_margin_equals_the_refit_form():
    """append / predict / pop per candidate (gp_opt.py:585-606), n <= 12, N <= 200, K <= 20: to D,
    the discrepancy between float64 and long double measured over the small cases."""
    gp, pts, Q, S, cand, fmin = small_problem()
    U = pts[~S]
    best, arg = er.margins(gp, U, pts[cand], Q[cand, 1], er.BETA, fmin)
    for k, idx in enumerate(cand):
        son._append_point(gp, pts[[idx]], np.atleast_2d(Q[idx, 1]))
        m2, v2 = gp.predict_noiseless(U)
        son._pop_point(gp)
        l2 = m2[:, 0] - er.BETA * np.sqrt(v2[:, 0]) - fmin
        assert abs(l2.max() - best[k]) < er.D_MAX, (k, l2.max(), best[k])
        assert l2[arg[k]] > l2.max() - er.D_MAX


def test_longdouble_solve_and_kernels():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(9, 9))
    A = A.dot(A.T) + np.eye(9)
    B = rng.normal(size=(9, 3))
    np.testing.assert_allclose(np.asarray(er.solve_longdouble(A, B), dtype=float),
                               np.linalg.solve(A, B), rtol=1e-12)
    x, y = rng.uniform(-2, 2, size=(7, 3)), rng.uniform(-2, 2, size=(5, 3))
    for spec in ("RBF", "Matern32", "Matern52", [("RBF", (0, 1)), ("Matern52", (1, 2))]):
        k = er.make_kernel(gpn, spec, 3, 0.8)
        np.testing.assert_allclose(np.asarray(er.kern_longdouble(k, x, y), dtype=float), k.K(x, y),
                                   rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", er.SMALL)
def test_float64_and_longdouble_margins_agree(name):
    D = er.discrepancy(name)
    print("%s: D = %.3g" % (name, D))
    assert D <= er.D_MAX


@pytest.mark.parametrize("name", list(er.CASES))
def test_the_reference_decides_the_case(name):
    """At most 1 % of the entries inside the band, at least 10 % hits and 10 % non-hits among
    the decided ones -- from the oracle alone."""
    c = er.build_case(name)
    assert 100.0 * er.D_MAX <= er.band(c) < 2e-9
    in_band, hits, non = er.shares(c)
    dec, hit = er.decided(c, c.best)
    print("%s: band %.3g, in band %.4f, decided hits %d, non-hits %d of %d x %d" % (
        name, er.band(c), in_band, hit.sum(), dec.sum() - hit.sum(), c.xc.shape[0],
        int(c.active.sum())))
    assert in_band <= 0.01 and hits >= 0.10 and non >= 0.10
    assert c.xc.shape[0] == max(c.Ks)
    if c.best_safe is not None:      # every safe row as a candidate (the device's own selections)
        in_band, hits, non = er.shares(c, c.best_safe)
        dec, hit = er.decided(c, c.best_safe)
        print("%s: every safe row: in band %.4f, decided hits %d, non-hits %d of %d x %d" % (
            name, in_band, hit.sum(), dec.sum() - hit.sum(), c.safe_rows.size, int(c.active.sum())))
        assert in_band <= 0.01
        assert c.safe_rows.size == 1 or (hits >= 0.10 and non >= 0.10)     # (one row: one answer)
    if c.n_special:                  # x_c = a training point | an unsafe row | far from everything
        assert np.all(np.abs(c.best[-3:][:, c.active]) > er.band(c))
        assert np.all(c.best[-1][c.active] < 0)
    if "lip" in c.cfg:
        L, best, bnd = er.lipschitz_case(c)
        dec = (np.abs(best) > bnd)[:, c.active]
        hit = (best >= 0)[:, c.active] & dec
        assert dec.mean() >= 0.99 and hit.sum() >= 0.1 * dec.sum()
        assert (dec.sum() - hit.sum()) >= 0.1 * dec.sum()


def test_big_case_leaves_the_one_item_per_workgroup_form():
    """>= 2048 unsafe rows are lifted above fmin by some candidate of the 4100: the device lists
    at least those (its pruning tests are necessary conditions)."""
    c = er.build_case("m52_d2_n520_big")
    assert c.xc.shape[0] >= 4097 and int((c.row_best[0] >= 0).sum()) >= 2048


def test_lipschitz_margin_is_the_formula_of_the_reference():
    gp, pts, Q, S, cand, fmin = small_problem(seed=5)
    L = 0.7
    best = er.lipschitz_margins(pts[~S], pts[cand], Q[cand, 1], [L], [fmin])
    for k, idx in enumerate(cand):
        d = np.sqrt(((pts[~S] - pts[idx]) ** 2).sum(axis=1))
        assert abs(best[k, 0] - np.max(Q[idx, 1] - L * d - fmin)) < 1e-13
    assert np.all(er.lipschitz_margins(pts[:0], pts[cand], Q[cand, 1], [L], [fmin]) == -np.inf)


@pytest.mark.parametrize("name", ["m32_d3_n272", "m52_d8_n256", "m32_d2_n16_grid"])
def test_tight_groups_are_decided_by_their_own_row(name):
    """``tight_group`` asserts what the GPU test relies on: the margins are the wanted ones, far
    outside the band, and attained at the row the candidates sit on."""
    xs, mu, u, fmin, best = er.tight_group(name)
    assert xs.shape[0] == 16 and (best > 0).sum() == 8 and np.all(u > mu)
