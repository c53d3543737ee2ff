"""Information-theoretic safe exploration without a GPU: the yardstick (tests/_ise_ref.py: the
float64 restatement of the device's stable form against the closed form of Bottero et al. 2022
at 80 digits), the exact properties of the form, the host logic of ``SafeOpt.ise_point`` /
``info_point`` through a NumPy stand-in (tests/_ise_backend.py) and the declarations."""
import os
import re
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _ise_ref as ref                                                     # noqa: E402


# ---- 1. the restatement against mpmath ---------------------------------------------------------

def test_restatement_error_is_measured():
    """The yardstick of tests/test_gpu_ise.py: measured, printed, not bounded here."""
    mu, vz, vx, c, s = ref.point_set()
    exact, unit, u = ref.point_reference()
    k = int(np.argmax(u))
    print("restatement: %d points, max error %.3f units of EPS (1 + t) sqrt(kappa) ln2 e^-t, at "
          "(mu, vz, vx, c, s) = %r" % (u.size, u.max(), (mu[k], vz[k], vx[k], c[k], s[k])))
    assert u.size == 6000 and np.all(np.isfinite(exact)) and np.isfinite(u.max())
    assert np.all(np.isfinite(ref.term(mu, vz, vx, c, s)))


# ---- 2. exact properties -----------------------------------------------------------------------

def _random(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    vz, vx = 10.0 ** rng.uniform(-6, 2, n), 10.0 ** rng.uniform(-6, 2, n)
    mu = rng.normal(size=n) * np.sqrt(vz) * 3.0
    rho = rng.uniform(-1.0, 1.0, n)
    s = vx * 10.0 ** rng.uniform(-6, 1, n)
    return mu, vz, vx, rho * np.sqrt(vx * vz), s


def test_zero_at_zero_covariance_and_the_bounds():
    mu, vz, vx, c, s = _random()
    t = ref.C1 * mu * mu / vz
    assert np.all(ref.term(mu, vz, vx, 0.0 * c, s) == 0.0)
    got = ref.term(mu, vz, vx, c, s)
    assert np.all(got >= 0.0) and np.all(got <= ref.LN2 * np.exp(-t))


def test_full_correlation_without_noise_is_the_whole_entropy():
    mu, vz, vx, c, _ = _random()
    full = np.sign(c) * np.sqrt(vx * vz) * (1.0 + 1e-9)       # r2 rounds to or above 1
    t = ref.C1 * (mu * mu) / vz
    assert_array_equal(ref.term(mu, vz, vx, full, 0.0), ref.LN2 * np.exp(-t))


def test_monotone_in_the_covariance():
    mu, vz, vx, _, s = (a[:200] for a in _random())
    rho = np.linspace(0.0, 1.0, 401)[:, None]
    for sign in (1.0, -1.0):
        got = ref.term(mu, vz, vx, sign * rho * np.sqrt(vx * vz), s)
        assert np.all(np.diff(got, axis=0) >= -4 * ref.EPS * ref.LN2)


def test_small_correlation_limit_pins_both_constants():
    """I / (ln2 e^-t e) -> c1 + t (1 - 2 c1) as r2 -> 0, e = r2 vx / B."""
    mu, vz, vx, _, s = _random()
    r2 = 1e-10
    c = np.sqrt(r2 * vx * vz)
    t = ref.C1 * mu * mu / vz
    e = r2 * vx / (s + vx + (2 * ref.C1 - 1) * r2 * vx)
    ratio = ref.term(mu, vz, vx, c, s) / (ref.LN2 * np.exp(-t) * e)
    want = 1.0 / (np.pi * np.log(2.0)) + t * (1.0 - 2.0 / (np.pi * np.log(2.0)))
    assert np.max(np.abs(ratio / want - 1.0)) < 1e-6


def test_naive_form_agrees_where_it_is_well_conditioned():
    mu, vz, vx, c, s = _random()
    t = ref.C1 * mu * mu / vz
    r2 = c * c / (vx * vz)
    ok = (r2 > 0.05) & (r2 < 0.95) & (t < 30.0)
    a, b = ref.term(mu, vz, vx, c, s)[ok], ref.naive(mu, vz, vx, c, s)[ok]
    assert ok.sum() > 500 and np.max(np.abs(a - b) / a) < 1e-11
    # ... and has no digits where it is not: r2 = 1e-18 is below the naive form's resolution
    tiny = np.sqrt(1e-18 * vx * vz)
    assert np.all(ref.term(mu, vz, vx, tiny, s)[t < 30] > 0.0)
    assert np.any(ref.naive(mu, vz, vx, tiny, s)[t < 30] <= 0.0)


def test_gap_to_the_exact_mutual_information():
    """Information, not a threshold: the approximation against I(y_x; [f(z) >= fmin]) by
    quadrature over the measurement, 300 random draws."""
    from scipy.special import ndtr
    rng = np.random.default_rng(9)
    n = 300
    vz, vx = rng.uniform(0.05, 2.0, n), rng.uniform(0.05, 2.0, n)
    mu = rng.normal(size=n) * np.sqrt(vz) * 1.5
    c = rng.uniform(-1.0, 1.0, n) * np.sqrt(vx * vz)
    s = rng.uniform(1e-4, 0.5, n)

    def h(p):
        p = np.clip(p, 1e-300, 1.0)
        q = np.clip(1.0 - p, 1e-300, 1.0)
        return -(p * np.log(p) + q * np.log(q))

    eta = np.linspace(-12.0, 12.0, 24001)
    wgt = np.exp(-0.5 * eta * eta) / np.sqrt(2 * np.pi) * (eta[1] - eta[0])
    gap = np.empty(n)
    for i in range(n):
        shift = c[i] / np.sqrt(vx[i] + s[i])
        sd = np.sqrt(vz[i] - shift * shift)
        exact = h(ndtr(mu[i] / np.sqrt(vz[i]))) - np.sum(wgt * h(ndtr((mu[i] + shift * eta) / sd)))
        gap[i] = abs(ref.term(mu[i], vz[i], vx[i], c[i], s[i]) - exact)
    print("gap to the exact mutual information by quadrature: max %.3e nats over %d draws"
          % (gap.max(), n))
    assert np.isfinite(gap.max())


# ---- 3. the host logic of ise_point / info_point -----------------------------------------------

def _opt(fmin=(0.0, 0.5), n_gps=2):
    import safeopt_amd
    from oracle import gp_numpy as gpn
    from _ise_backend import use_ise_backend
    use_ise_backend()
    x = np.linspace(-1.0, 1.0, 5)[:, None]
    gps = [gpn.GPRegression(x, np.cos(x) + 1.0 + 0.1 * g, gpn.RBF(1, 1.0, 0.5 + 0.1 * g),
                            noise_var=1e-4 * (g + 1)) for g in range(n_gps)]
    opt = safeopt_amd.SafeOpt(gps if n_gps > 1 else gps[0], np.linspace(-2.0, 2.0, 60)[:, None],
                              list(fmin)[:n_gps] if n_gps > 1 else fmin[0])
    opt.update_confidence_intervals()
    opt.compute_safe_set()
    return opt


def _host(opt, rows, about):
    """alpha, targets and the pick of ``rows`` from the stand-in's own pairs."""
    be = opt._backend
    pr = be.ise(np.asarray(opt.fmin, dtype=float), rows, 0, pairs=True)[4]
    be.calls.pop()
    al, tg = ref.alpha(pr, ~be.S if about == 'unsafe' else np.ones(be.S.size, dtype=bool))
    return (al, tg) + ref.pick(al, tg, rows)


@pytest.mark.parametrize("about", ["unsafe", "all"])
def test_ise_point_selects_reduces_and_strips(about):
    opt = _opt()
    S = opt._backend.S.copy()
    assert 3 < S.sum() < S.size
    var, _, s = opt._backend.ise_state()
    want_rows = ref.select(var, S, s, np.array([True, True]), 7)
    x, a, rows, values, targets = opt.ise_point(candidates=7, about=about, return_values=True)
    assert_array_equal(rows, want_rows)
    assert rows.dtype == np.int64 and np.all(S[rows])
    al, tg, v, i = _host(opt, rows, about)
    assert_array_equal(values, al)
    assert_array_equal(targets, tg)
    assert a == v and x.shape == (1,)
    assert_array_equal(x, opt.inputs[i])
    if about == 'unsafe':
        assert not np.any(S[targets])
    assert opt._backend.calls[-1][1] == (0 if about == 'unsafe' else 1)
    x2, a2 = opt.ise_point(candidates=7, about=about)
    assert_array_equal(x2, x)
    assert a2 == a
    # more candidates than safe rows: all of S
    rows_all = opt.ise_point(candidates=4096, about=about, return_values=True)[2]
    assert sorted(rows_all) == list(np.flatnonzero(S))


def test_candidate_selection_orders_by_key_then_row():
    from safeopt_amd.gp_opt import ise_candidates
    var = np.array([[0.5, 0.2, 0.5, 0.9, 0.5, 0.1], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    S = np.array([True, True, True, False, True, True])
    s = np.array([0.01, 0.02])
    both, first = np.array([True, True]), np.array([True, False])
    assert ise_candidates(var, S, s, both, 3).tolist() == [0, 2, 4]      # ties: the lower row
    assert ise_candidates(var, S, s, both, 9).tolist() == [0, 2, 4, 1, 5]
    assert ise_candidates(var, S, s, first, 4).tolist() == ref.select(var, S, s, first, 4).tolist()
    rng = np.random.default_rng(4)
    var = rng.choice([0.1, 0.2, 0.3], size=(3, 200))
    S = rng.random(200) < 0.6
    s = np.array([0.01, 0.02, 0.03])
    act = np.array([True, False, True])
    for K in (1, 17, 500):
        assert_array_equal(ise_candidates(var, S, s, act, K), ref.select(var, S, s, act, K))


def test_explicit_rows_and_ties_between_candidates():
    opt = _opt()
    S = opt._backend.S
    ids = np.flatnonzero(S)
    rows = np.array([ids[3], ids[1], ids[3], ids[0]])                    # a duplicate
    x, a, got_rows, values, targets = opt.ise_point(candidates=rows, return_values=True)
    assert_array_equal(got_rows, rows)
    assert values[0] == values[2] and targets[0] == targets[2]
    al, tg, v, i = _host(opt, rows, 'unsafe')
    assert (a, int(np.flatnonzero(np.all(opt.inputs == x, axis=1))[0])) == (v, i)
    # equal alpha: the lowest global row wins, wherever it stands in the list
    assert ref.pick(np.array([0.3, 0.7, 0.7]), np.array([5, 5, 5]), np.array([9, 8, 4])) == (0.7, 4)
    assert ref.pick(np.array([0.3, 0.7]), np.array([-1, -1]), np.array([9, 8])) == (-np.inf, -1)
    unsafe = np.flatnonzero(~S)[0]
    with pytest.raises(ValueError, match="outside the safe set"):
        opt.ise_point(candidates=np.array([ids[0], unsafe]))
    for bad in (np.array([[1, 2]]), np.array([], dtype=int), np.array([0.5]), np.array([-1]),
                np.array([60]), np.zeros(4097, dtype=int)):
        with pytest.raises(ValueError):
            opt.ise_point(candidates=bad)


@pytest.mark.parametrize("kw", [dict(about='safe'), dict(about=None), dict(candidates=0),
                                dict(candidates=4097), dict(candidates=2.5)])
def test_ise_point_refuses_bad_arguments(kw):
    opt = _opt()
    with pytest.raises(ValueError):
        opt.ise_point(**kw)
    assert opt._backend.calls == []


def test_ise_point_errors():
    opt = _opt()
    opt.S[:] = False
    with pytest.raises(RuntimeError, match="no safe points"):
        opt.ise_point()
    opt = _opt()
    opt.S[:] = True
    with pytest.raises(RuntimeError, match="no row qualifies"):
        opt.ise_point()
    assert opt.ise_point(about='all')[1] > 0.0
    opt = _opt(fmin=(-np.inf, -np.inf))
    with pytest.raises(ValueError, match="finite fmin"):
        opt.ise_point()
    assert opt._backend.calls == []
    # an inactive GP adds nothing
    one = _opt(fmin=(0.0, -np.inf))
    rows = np.flatnonzero(one._backend.S)[:4]
    v = one.ise_point(candidates=rows, return_values=True)[3]
    alone = _opt(fmin=(0.0,), n_gps=1)
    assert_array_equal(alone._backend.S, one._backend.S)
    assert_array_equal(alone.ise_point(candidates=rows, return_values=True)[3], v)


def test_one_rank_guard_comes_before_anything_runs():
    opt = _opt()

    class Two(object):
        rank, world = 0, 2
    opt._comm = Two()
    for call in (opt.ise_point, opt.info_point):
        with pytest.raises(NotImplementedError, match="one rank"):
            call()
    assert opt._backend.calls == []


def test_backend_without_ise_is_refused():
    import safeopt_amd
    from oracle import gp_numpy as gpn
    from _oracle_backend import OracleGridBackend, use_oracle_backend
    assert not hasattr(OracleGridBackend, 'ise')
    use_oracle_backend()
    x = np.linspace(-1.0, 1.0, 5)[:, None]
    gp = gpn.GPRegression(x, np.cos(x) + 1.0, gpn.RBF(1, 1.0, 0.5), noise_var=1e-4)
    opt = safeopt_amd.SafeOpt(gp, np.linspace(-2.0, 2.0, 50)[:, None], 0.0)
    with pytest.raises(NotImplementedError):
        opt.ise_point()


def test_state_is_untouched():
    opt = _opt()
    be = opt._backend
    before = [a.copy() for a in (be.Q, be.S, be.M, be.G, opt.x, opt.y)]
    rs = np.random.get_state()
    opt.ise_point(candidates=5)
    opt.ise_point(candidates=np.flatnonzero(be.S)[:3], about='all', return_values=True)
    for u, w in zip(before, (be.Q, be.S, be.M, be.G, opt.x, opt.y)):
        assert_array_equal(u, w)
    now = np.random.get_state()
    assert rs[0] == now[0] and np.array_equal(rs[1], now[1]) and rs[2:] == now[2:]


def test_info_point_takes_the_larger_acquisition():
    opt = _opt()
    x_i, a_i = opt.ise_point(candidates=8)
    x_m = np.array([-7.0])
    for a_m, which in ((a_i * 0.5, 'ise'), (a_i, 'mes'), (a_i * 2.0, 'mes')):
        opt.mes_point = lambda paths=16, features=1024, _a=a_m: (x_m, _a)
        x, a, w = opt.info_point(candidates=8)
        assert w == which and a == (a_i if which == 'ise' else a_m)
        assert_array_equal(x, x_i if which == 'ise' else x_m)
    # no row qualifies for ISE: the MES pick
    opt.S[:] = True
    opt.mes_point = lambda paths=16, features=1024: (x_m, 1e-9)
    assert opt.info_point()[1:] == (1e-9, 'mes')


# ---- 4. the declarations -----------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sgp_ise_eval", "sgp_grid_ise"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"#define\s+SGP_MAX_ISE\s+4096\b", code)
    for name, val in (("SGP_ISE_UNSAFE", 0), ("SGP_ISE_ALL", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), code), name
    from safeopt_amd import _hip
    assert (_hip.ISE_UNSAFE, _hip.ISE_ALL, _hip.MAX_ISE) == (0, 1, 4096)
    for name in ("sgp_ise_eval", "sgp_grid_ise"):
        assert name in _hip.PROTOTYPES


def test_ise_source_is_built_without_contraction():
    from safeopt_amd import build
    assert "ise.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA["ise.hip"]
    assert any(h.endswith("ise_term.h") for h in build.HEADERS)
