"""Pooling of repeated measurements, without a GPU: the identity behind it in long double
(tests/_reweigh_ref.py: refits only), the log-to-row map ``safeopt_amd.pooling.PoolBook`` on
random sequences, and the host logic of ``GPRegression.pool_data`` / ``unpool_data`` and of the
optimisers' ``pool_repeats`` on stand-ins for the device objects.
"""
import numpy as np
import pytest

import _reweigh_ref as R
from safeopt_amd import gp_opt
from safeopt_amd import gpy
from safeopt_amd.pooling import PoolBook, row_key

LD = R.LD


# ---- the identity -----------------------------------------------------------------------------
def pooled(ys, rhos):
    """``(ybar, r)`` of measurements ``ys`` with noise scales ``rhos`` at one input."""
    ys, rhos = np.asarray(ys, dtype=LD), np.asarray(rhos, dtype=LD)
    r = LD(1) / (LD(1) / rhos).sum()
    return r * (ys / rhos).sum(), r


def pool_term(ys, rhos, noise):
    """``log p(measurements) - log p(pooled observation)`` of one input."""
    ys, rhos = np.asarray(ys, dtype=LD), np.asarray(rhos, dtype=LD)
    s = LD(noise) + LD(1e-8)
    ybar, r = pooled(ys, rhos)
    return (-LD(0.5) * (len(ys) - 1) * np.log(LD(2) * LD(np.pi) * s) - LD(0.5) * np.log(rhos).sum()
            + LD(0.5) * np.log(r) - ((ys * ys / rhos).sum() - ybar * ybar / r) / (LD(2) * s))


def _repeats(seed, equal_scales):
    """12 inputs in [-2, 2]^2, 1 .. 4 measurements each; scales ones or drawn from 1/16 .. 4."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (12, 2))
    counts = rng.integers(1, 5, size=12)
    rows, ys, rhos = [], [], []
    for i, k in enumerate(counts):
        f = np.sin(X[i, 0]) + 0.3 * X[i, 1]
        rows.append(np.repeat(X[i:i + 1], k, axis=0))
        ys.append(f + 0.05 * rng.normal(size=k))
        rhos.append(np.ones(k) if equal_scales else rng.choice(R.SCALES, size=k))
    return X, counts, rows, ys, rhos


@pytest.mark.parametrize("equal_scales", [True, False])
def test_pooling_identity(equal_scales):
    """Posterior and corrected marginal likelihood of pooled against unpooled data, both as
    long-double fits: k measurements (y_j, rho_j) at one input are one observation with r = 1 /
    sum 1/rho_j and y = r sum y_j / rho_j, and the likelihoods differ by ``pool_term``."""
    spec = R.single("Matern52", 2)
    X, counts, rows, ys, rhos = _repeats(3, equal_scales)
    assert counts.max() > 2 and counts.min() == 1
    full = R.ScaledGP(spec, np.vstack(rows), np.concatenate(ys), np.concatenate(rhos))
    yb, rb = zip(*(pooled(y, p) for y, p in zip(ys, rhos)))
    pool = R.ScaledGP(spec, X, np.array(yb, dtype=LD), np.array(rb, dtype=LD))
    Xs = np.random.default_rng(4).uniform(-3, 3, (50, 2))
    (m1, v1), (m2, v2) = full.predict(Xs), pool.predict(Xs)
    em, ev = float(np.max(np.abs(m1 - m2))), float(np.max(np.abs(v1 - v2)))
    term = sum(pool_term(y, p, R.NOISE) for y, p in zip(ys, rhos))
    el = float(abs(full.log_likelihood() - (pool.log_likelihood() + term)))
    print("pooled against unpooled: mean %.2e  var %.2e  likelihood %.2e (term %.6g)"
          % (em, ev, el, float(term)))
    # the unpooled Ky has k equal rows up to the noise: cond ~ 1e4, long double eps 1e-19
    assert em < 1e-13 and ev < 1e-13
    assert el < 1e-11 * abs(float(full.log_likelihood()))


def test_model_pool_term_matches():
    """``GPRegression._pool_term`` (float64, from the sufficient statistics) against the
    long-double statement, value and derivative in noise_var."""
    _, counts, _, ys, rhos = _repeats(5, False)
    gp = object.__new__(gpy.GPRegression)
    gp.X = np.zeros((len(ys), 1))
    gp._stats = []
    for y, p in zip(ys, rhos):
        gp._stats.append(None if len(y) == 1 and p[0] == 1.0 else
                         [len(y), (1 / p).sum(), (y / p).sum(), (y * y / p).sum(),
                          np.log(p).sum()])
    val, grad = gp._pool_term(R.NOISE)
    want = float(sum(pool_term(y, p, R.NOISE) for y, p in zip(ys, rhos)))
    h = 1e-7
    fd = float(sum(pool_term(y, p, R.NOISE + h) - pool_term(y, p, R.NOISE - h)
                   for y, p in zip(ys, rhos)) / (2 * LD(h)))
    print("pool term %.12g (long double %.12g), derivative %.10g (difference %.10g)"
          % (val, want, grad, fd))
    assert abs(val - want) < 1e-10 * abs(want)
    assert abs(grad - fd) < 1e-6 * abs(fd)


# ---- the book ---------------------------------------------------------------------------------
def _rebuild(x, y, rho, g, initial):
    """The pooled data of GP ``g`` straight from the log: the first ``initial`` rows as they
    are, then one row per distinct input in the rest, unless an initial row has it."""
    rows = {}                        # key -> [x, sum 1/rho, sum y/rho, k]
    order = []
    for j in range(len(x)):
        if np.isnan(y[j][g]):
            continue
        key = row_key(x[j])
        if j < initial:
            key = (key, j) if key in rows else key            # equal initial rows stay apart
        if key not in rows:
            rows[key] = [x[j], 0.0, 0.0, 0]
            order.append(key)
        ent = rows[key]
        ent[1] += 1.0 / rho[j][g]
        ent[2] += y[j][g] / rho[j][g]
        ent[3] += 1
    out = [(tuple(rows[k][0]), rows[k][2] / rows[k][1], 1.0 / rows[k][1], rows[k][3])
           for k in order]
    return sorted(out)


def _image(book, g, x, y, rho):
    X, yb, r, k = book.image(g, x, y, rho)
    return sorted((tuple(X[i]), yb[i], r[i], int(k[i])) for i in range(len(yb)))


@pytest.mark.parametrize("seed", range(6))
def test_book_follows_random_sequences(seed):
    """add (new input / repeat), remove, remove-last, nan columns, two GPs: after every call
    the pooled (X, ybar, r) of every GP rebuilt from the log equals the book's, and the actions
    it returned lead a shadow GP there."""
    rng = np.random.default_rng(seed)
    G, d = 2, 2
    sites = rng.uniform(-2, 2, (7, d))
    sites[1, 0] = -0.0                                    # -0.0 and 0.0 are one input
    x = [sites[i] for i in (0, 1, 2)]
    y = [list(rng.normal(size=G)) for _ in x]
    rho = [[1.0] * G for _ in x]
    initial = len(x)
    book = PoolBook(np.array(x), np.ones((initial, G), dtype=bool))
    shadow = [[[row_key(xx), 1] for xx in x] for _ in range(G)]      # per GP: [key, count]

    for step in range(120):
        what = rng.choice(["new", "repeat", "repeat", "remove", "last"])
        if what in ("new", "repeat") or len(x) <= 2:
            xx = rng.uniform(-2, 2, d) if what == "new" else sites[rng.integers(len(sites))].copy()
            if what != "new" and rng.uniform() < 0.2:
                xx = xx * 1.0 + 0.0
                xx[xx == 0.0] = 0.0                       # +0.0 where the site has -0.0
            yy = list(rng.normal(size=G))
            if rng.uniform() < 0.25:
                yy[rng.integers(G)] = np.nan
            pp = list(rng.choice(R.SCALES, size=G))
            acts = book.add(xx, ~np.isnan(yy))
            for g, act in enumerate(acts):
                assert (act is None) == bool(np.isnan(yy[g]))
                if act is None:
                    continue
                if act[0] == "append":
                    assert act[1] == len(shadow[g])
                    assert all(k != row_key(xx) for k, _ in shadow[g])
                    shadow[g].append([row_key(xx), 1])
                else:
                    assert shadow[g][act[1]][0] == row_key(xx)
                    shadow[g][act[1]][1] += 1
            x.append(xx)
            y.append(yy)
            rho.append(pp)
        else:
            index = len(x) - 1 if what == "last" else int(rng.integers(len(x)))
            where = book.locate(index)
            acts = book.remove(index)
            for g, act in enumerate(acts):
                assert (act is None) == bool(np.isnan(y[index][g]))
                if act is None:
                    continue
                assert act[1] == where[g] and shadow[g][act[1]][0] == row_key(x[index])
                if act[0] == "unpool":
                    shadow[g][act[1]][1] -= 1
                    assert shadow[g][act[1]][1] >= 1
                else:
                    assert shadow[g][act[1]][1] == 1
                    del shadow[g][act[1]]
            if index < initial:
                initial -= 1
            del x[index], y[index], rho[index]
        assert book.t == len(x)
        for g in range(G):
            assert book.rows(g) == len(shadow[g])
            assert [c for _, c in shadow[g]] == book.count[g]
            assert _image(book, g, x, y, rho) == pytest.approx(_rebuild(x, y, rho, g, initial)), \
                (seed, step, what)
            for j in range(len(x)):
                row = book.where[j][g]
                assert (row is None) == bool(np.isnan(y[j][g]))
                if row is not None:
                    assert shadow[g][row][0] == row_key(x[j]) and j in book.members(g, row)


def test_book_equal_initial_rows_stay_apart():
    """The initial data are taken as they are: two equal initial rows are two GP rows; a repeat
    goes to the first; when that one leaves, to the other."""
    x0 = np.array([[1.0], [2.0], [1.0]])
    book = PoolBook(x0, np.ones((3, 1), dtype=bool))
    assert book.rows(0) == 3
    assert book.add([1.0], [True]) == [("pool", 0)]
    assert book.remove(3) == [("unpool", 0)]
    assert book.remove(0) == [("remove", 0)]
    assert book.locate(1) == [1] and book.match([1.0], 0) == 1
    assert book.add([1.0], [True]) == [("pool", 1)]
    with pytest.raises(IndexError):
        book.remove(7)


# ---- the model and the optimiser on stand-ins ----------------------------------------------
class _FakeDev(object):
    """A DeviceGP as far as ``GPRegression`` looks at it; it records the calls."""

    def __init__(self, n, fail=False):
        self.n, self.fail, self.calls = n, fail, []

    def reweigh(self, index, y, r):
        self.calls.append(("reweigh", index, y, r))
        return not self.fail

    def append(self, x, y, r=None):
        self.calls.append(("append", r))
        self.n += 1
        return True

    def append_block(self, X, y, r=None):
        self.calls.append(("append_block", len(y), None if r is None else list(r)))
        self.n += len(y)
        return True

    def remove(self, index):
        self.calls.append(("remove", index))
        self.n -= 1
        return True

    def pop(self):
        self.calls.append(("pop",))
        self.n -= 1

    def set_data(self, X, Y, r=None):
        self.calls.append(("set_data", len(X), None if r is None else list(r)))
        self.n = len(X)


def _fake_gp(X, Y, fail=False, incremental=True):
    gp = object.__new__(gpy.GPRegression)
    gp.X, gp.Y = np.array(X, dtype=float), np.array(Y, dtype=float)
    gp.input_dim = gp.X.shape[1]
    gp.noise_var = 0.01
    gp.incremental = incremental
    gp._dev = _FakeDev(gp.X.shape[0], fail)
    gp._dev_fitted = True
    gp._device_gp = lambda in_place=False: gp._dev
    gp._fitted = lambda: gp._dev
    return gp


def test_model_pool_and_unpool():
    gp = _fake_gp([[0.0], [1.0]], [[0.5], [1.5]])
    gp.pool_data(1, 2.5, noise_scale=1.0)
    assert gp._dev.calls == [("reweigh", 1, 2.0, 0.5)]
    assert gp.Y[1, 0] == 2.0 and list(gp.noise_scale) == [1.0, 0.5]
    assert list(gp.pooled_counts()) == [1, 2]
    gp.pool_data(1, 1.0, noise_scale=0.5)                 # precision 1 + 1 + 2
    assert gp._dev.calls[-1] == ("reweigh", 1, (1.5 + 2.5 + 2 * 1.0) / 4, 0.25)
    gp.unpool_data(1, 2.5)
    assert gp._dev.calls[-1][1:] == (1, pytest.approx((1.5 + 2.0) / 3), pytest.approx(1 / 3))
    gp.unpool_data(1, 1.0, noise_scale=0.5)
    assert gp.Y[1, 0] == pytest.approx(1.5) and gp.noise_scale[1] == pytest.approx(1.0)
    assert gp._stats[1] is None
    with pytest.raises(ValueError):                       # the last member of a row
        gp.unpool_data(1, 1.5)
    with pytest.raises(ValueError):
        gp.pool_data(0, np.nan)
    with pytest.raises(ValueError):
        gp.pool_data(0, 1.0, noise_scale=0.0)
    with pytest.raises(IndexError):
        gp.pool_data(2, 1.0)
    assert not gp.noise_scale.flags.writeable


def test_model_reweigh_falls_back_to_a_refit():
    for kw in (dict(fail=True), dict(incremental=False)):
        gp = _fake_gp([[0.0], [1.0]], [[0.5], [1.5]], **kw)
        gp.reweigh_data(0, y=0.7, noise_scale=4.0)
        assert gp._dev.calls[-1] == ("set_data", 2, [4.0, 1.0])
        assert gp.Y[0, 0] == 0.7
    gp = _fake_gp([[0.0], [1.0]], [[0.5], [1.5]])
    gp.pool_data(0, 0.7)
    gp.reweigh_data(0, noise_scale=2.0)                   # drops the pooling statistics
    assert gp._stats[0] is None and gp._dev.calls[-1] == ("reweigh", 0, 0.6, 2.0)


def test_model_scales_follow_the_rows():
    gp = _fake_gp([[0.0], [1.0], [2.0]], [[0.5], [1.5], [2.5]])
    gp.set_XY(np.vstack([gp.X, [[3.0]]]), np.vstack([gp.Y, [[3.5]]]),
              noise_scale=[1.0, 1.0, 1.0, 0.25])
    assert gp._dev.calls == [("append", 0.25)]           # the kept rows' scales are equal
    gp.pool_data(1, 1.7)
    gp.remove_data(0)
    assert list(gp.noise_scale) == [0.5, 1.0, 0.25] and list(gp.pooled_counts()) == [2, 1, 1]
    gp.append_XY([[4.0], [5.0]], [[4.5], [5.5]], noise_scale=[2.0, 4.0])
    assert gp._dev.calls[-1] == ("append_block", 2, [2.0, 4.0])
    assert list(gp.noise_scale) == [0.5, 1.0, 0.25, 2.0, 4.0]
    gp.set_XY(gp.X[:-1], gp.Y[:-1], noise_scale=gp.noise_scale[:-1])
    assert gp._dev.calls[-1] == ("pop",) and list(gp.pooled_counts()) == [2, 1, 1, 1]
    gp.set_XY(gp.X, gp.Y)                                 # other scales for the kept rows: a refit
    assert gp._dev.calls[-1] == ("set_data", 4, None) and list(gp.noise_scale) == [1.0] * 4


def _fake_opt(x0, y0, pool):
    y0 = np.array(y0, dtype=float)
    x0 = np.array(x0, dtype=float)
    gps = [_fake_gp(x0, y0[:, [g]]) for g in range(y0.shape[1])]
    for gp in gps:
        gp.loo = None
    opt = object.__new__(gp_opt.GaussianProcessOptimization)
    opt.gps, opt.gp, opt.num_contexts = gps, gps[0], 0
    opt._x, opt._y = x0, y0
    if pool:
        opt._pool = PoolBook(x0, np.ones(y0.shape, dtype=bool))
    return opt


def test_optimiser_pools_repeats_and_takes_them_back():
    opt = _fake_opt([[0.0], [1.0]], [[0.5, 5.0], [1.5, 6.0]], pool=True)
    opt.add_new_data_point([1.0], [2.5, np.nan])          # a repeat: GP 0 pools, GP 1 did not see
    assert opt.gps[0]._dev.calls == [("reweigh", 1, 2.0, 0.5)] and opt.gps[1]._dev.calls == []
    opt.add_new_data_point([3.0], [3.5, 7.0], noise_scale=[1.0, 0.25])
    assert opt.gps[0]._dev.calls[-1] == ("append", 1.0)
    assert opt.gps[1]._dev.calls[-1] == ("append", 0.25)
    assert opt.t == 4 and opt.gps[0].X.shape[0] == 3 and opt.gps[1].X.shape[0] == 3
    assert np.array_equal(opt._rho, [[1, 1], [1, 1], [1, 1], [1, 0.25]])
    opt.add_new_data_point([3.0], [3.7, 7.2], noise_scale=0.5)
    assert opt.gps[1]._dev.calls[-1][:2] == ("reweigh", 2)
    assert opt.gps[1].noise_scale[2] == pytest.approx(1 / 6)
    # taking back: the newest (pooled), then a pooled one in the middle, then a singleton
    opt.remove_last_data_point()
    assert opt.t == 4 and opt.gps[1].noise_scale[2] == pytest.approx(0.25)
    assert opt.gps[0].Y[2, 0] == pytest.approx(3.5)
    opt.remove_data_point(1)                              # member of GP 0's pooled row 1
    assert opt.gps[0]._dev.calls[-1][:2] == ("reweigh", 1) and opt.gps[0].Y[1, 0] == 2.5
    assert opt.gps[1]._dev.calls[-1] == ("remove", 1)     # GP 1 held it alone
    assert opt.t == 3 and opt.gps[0].X.shape[0] == 3 and opt.gps[1].X.shape[0] == 2
    opt.remove_data_point(0)
    assert opt.gps[0]._dev.calls[-1] == ("remove", 0) and opt.gps[1]._dev.calls[-1] == ("remove", 0)
    for g in range(2):
        X, yb, r, k = opt._pool.image(g, opt._x, opt._y, opt._rho)
        assert np.array_equal(X, opt.gps[g].X)
        assert np.allclose(yb, opt.gps[g].Y[:, 0]) and np.allclose(r, opt.gps[g].noise_scale)
    with pytest.raises(ValueError):                       # GP 1 would be left without data
        opt.remove_data_point(1)
        opt.remove_data_point(0)


def test_optimiser_batch_pools_row_by_row_and_appends_the_rest():
    opt = _fake_opt([[0.0], [1.0]], [[0.5], [1.5]], pool=True)
    opt.add_new_data_points([[2.0], [1.0], [2.0], [3.0]], [[2.5], [1.7], [2.7], [3.5]])
    calls = opt.gps[0]._dev.calls
    assert calls[0] == ("append_block", 2, None)          # 2.0 and 3.0, one block
    assert [c[:2] for c in calls[1:]] == [("reweigh", 1), ("reweigh", 2)]
    assert opt.t == 6 and opt.gps[0].X.shape[0] == 4
    assert list(opt.gps[0].pooled_counts()) == [1, 2, 2, 1]


def test_without_pooling_scales_are_passed_to_the_appends():
    opt = _fake_opt([[0.0], [1.0]], [[0.5], [1.5]], pool=False)
    opt.add_new_data_point([1.0], [2.5], noise_scale=0.25)
    assert opt.gps[0]._dev.calls == [("append", 0.25)] and opt.gps[0].X.shape[0] == 3
    opt.add_new_data_point([2.0], [2.5])                  # the GP holds scales: they stay
    assert opt.gps[0]._dev.calls[-1] == ("append", 1.0)
    assert list(opt.gps[0].noise_scale) == [1.0, 1.0, 0.25, 1.0]
    opt.remove_last_data_point()
    assert opt.gps[0]._dev.calls[-1] == ("pop",) and list(opt.gps[0].noise_scale) == [1, 1, 0.25]
    assert opt._rho.shape == (3, 1)
    with pytest.raises(ValueError):
        opt.add_new_data_point([2.0], [2.5], noise_scale=-1.0)
    with pytest.raises(ValueError):
        opt.add_new_data_point([2.0], [2.5], noise_scale=[1.0, 2.0])
