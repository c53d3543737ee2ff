"""Removal of any observation, without a GPU: the float64 restatement of the downdate against
the long-double refit (tests/_remove_ref.py), and the host logic -- ``remove_data_point``,
``GPRegression.remove_data`` and the choice of ``_HipGridBackend.confidence`` -- on stand-ins
for the device objects.

Tolerances: the project's 1e-8 (L^-1 absolute; alpha, w and alpha_i relative to the largest
entry; P_ii relative).  ``restatement_errors`` prints what float64 gives per case; the table
is in profiles/remove/SUMMARY.txt."""
import os
import re

import numpy as np
import pytest

import _remove_ref as R
from safeopt_amd import _hip, gp_opt, gpy

TOL = 1e-8


# ---- the restatement against the long-double refit -------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FACTOR_CASES))
def test_restatement_against_long_double(name):
    e = R.restatement_errors(name)
    Mn, an, w, ai, P = e.pop("result")
    print(name, {k: "%.1e" % v for k, v in e.items()})
    n = R.FACTOR_CASES[name][2] - 1
    assert Mn.shape == (n, n) and an.shape == (n,) and w.shape == (n,)
    assert np.all(Mn[np.triu_indices(n, 1)] == 0.0)           # by construction
    assert np.all(np.diag(Mn) > 0.0)
    assert P > 0.0
    for what in ("Linv", "alpha", "w", "alpha_i", "P_ii"):
        assert e[what] < TOL, (name, what, e[what])


def test_record_is_the_append_of_the_row_to_the_reduced_gp():
    """{w, alpha_i, P_ii} of the truth are what an append of (x_i, y_i) to the reduced GP
    writes: {Ky_new^-1 k, r / s2, 1 / s2} -- and the rank-1 formulas with both signs flipped
    take the posterior of the full data to that of the reduced data."""
    spec, d, n, i = R.FACTOR_CASES["rbf_d3_n130_i64"]
    X, Y, Xs, t = R.factor_reference("rbf_d3_n130_i64")
    full = R.RefGP(spec, X, Y)
    m0, v0 = full.predict(Xs)
    keep = np.arange(n) != i
    cx = R.kern(spec, X[i:i + 1], Xs)[0] - R.LD(1) * t["w"] @ R.kern(spec, X[keep], Xs)
    assert abs(R.f64(full.alpha()[i]) - t["alpha_i"]) < 1e-12 * np.max(np.abs(t["alpha"]))
    assert np.max(np.abs(R.f64(m0 - cx * t["alpha_i"]) - t["mean"])) < 1e-12
    assert np.max(np.abs(R.clip_var(v0 + cx * cx * t["P_ii"]) - t["var"])) < 1e-12


# ---- the C ABI ---------------------------------------------------------------------------------
def test_entry_points_are_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "safeopt_hip.h")).read()
    for name in ("sgp_gp_remove", "sgp_grid_rank1_remove"):
        assert name in _hip.PROTOTYPES
        assert re.search(r"\bint %s\(" % name, header)
    assert _hip.PROTOTYPES["sgp_grid_rank1_remove"] == _hip.PROTOTYPES["sgp_grid_rank1_update"]


# ---- remove_data_point on stand-ins ------------------------------------------------------------
class _FakeDev(object):
    """A DeviceGP as far as ``GPRegression`` and the grid backend look at it."""
    serial = 0

    def __init__(self, n, fail_remove=False):
        _FakeDev.serial += 1
        self.serial, self.n, self.version = _FakeDev.serial, n, 1
        self.appended = self.removed = False
        self.fail_remove, self.calls = fail_remove, []

    def remove(self, index):
        self.calls.append(("remove", index))
        if self.fail_remove:
            return False
        self.n -= 1
        self.version += 1
        self.appended, self.removed = False, True
        return True

    def append(self, x, y):
        self.calls.append(("append",))
        self.n += 1
        self.version += 1
        self.appended, self.removed = True, False
        return True

    def pop(self):
        self.calls.append(("pop",))
        self.n -= 1
        self.version += 1
        self.appended = self.removed = False

    def set_data(self, X, Y):
        self.calls.append(("set_data", len(X)))
        self.n = len(X)
        self.version += 1
        self.appended = self.removed = False


def _fake_gp(X, Y, fail_remove=False, incremental=True):
    gp = object.__new__(gpy.GPRegression)
    gp.X, gp.Y = np.array(X, dtype=float), np.array(Y, dtype=float)
    gp.input_dim = gp.X.shape[1]
    gp.incremental = incremental
    gp._dev = _FakeDev(gp.X.shape[0], fail_remove)
    gp._dev_fitted = True
    gp._device_gp = lambda in_place=False: gp._dev
    gp._fitted = lambda: gp._dev
    return gp


def _fake_opt(y, **kw):
    """A measurement log of len(y) rows; GP g observed the rows where y[:, g] is a number."""
    y = np.array(y, dtype=float)
    x = np.arange(float(len(y)))[:, None]
    opt = object.__new__(gp_opt.GaussianProcessOptimization)
    opt.gps = [_fake_gp(x[~np.isnan(y[:, g])], y[~np.isnan(y[:, g])][:, [g]], **kw)
               for g in range(y.shape[1])]
    opt.gp = opt.gps[0]
    opt._x, opt._y = x, y
    return opt


NAN = np.nan
LOG = [[1.0, 10.0], [2.0, NAN], [NAN, 30.0], [4.0, 40.0], [5.0, NAN]]


def test_row_mapping_with_nan_columns():
    opt = _fake_opt(LOG)
    opt.remove_data_point(3)                # GP 0 saw rows 0, 1 in front of it, GP 1 rows 0, 2
    assert [gp._dev.calls for gp in opt.gps] == [[("remove", 2)], [("remove", 2)]]
    assert opt.x[:, 0].tolist() == [0.0, 1.0, 2.0, 4.0] and opt.t == 4
    assert opt.gps[0].X[:, 0].tolist() == [0.0, 1.0, 4.0]
    assert opt.gps[0].Y[:, 0].tolist() == [1.0, 2.0, 5.0]
    assert opt.gps[1].X[:, 0].tolist() == [0.0, 2.0] and opt.gps[1].Y[:, 0].tolist() == [10.0, 30.0]
    opt.remove_data_point(1)                # only GP 0 observed it
    assert opt.gps[0]._dev.calls[-1] == ("remove", 1) and len(opt.gps[1]._dev.calls) == 1
    assert opt.y.tolist()[0] == [1.0, 10.0] and np.isnan(opt.y[1, 0]) and opt.t == 3
    opt.remove_data_point(0)                # the first row of both
    assert [gp._dev.calls[-1] for gp in opt.gps] == [("remove", 0), ("remove", 0)]
    assert opt.gps[0].X[:, 0].tolist() == [4.0] and opt.gps[1].X[:, 0].tolist() == [2.0]


def test_errors_come_before_any_device_call():
    opt = _fake_opt(LOG)
    for bad in (-1, 5, 17, 1.5):
        with pytest.raises(IndexError):
            opt.remove_data_point(bad)
    opt = _fake_opt([[1.0, 10.0], [2.0, NAN], [3.0, NAN]])
    with pytest.raises(ValueError):         # GP 1 has one observation, and it is row 0
        opt.remove_data_point(0)
    assert all(gp._dev.calls == [] for gp in opt.gps) and opt.t == 3
    assert opt.gps[0].X.shape[0] == 3
    opt.remove_data_point(2)                # GP 1 did not see row 2: fine
    assert opt.gps[0]._dev.calls == [("remove", 2)] and opt.gps[1]._dev.calls == []


def test_fallback_to_set_xy():
    opt = _fake_opt(LOG, fail_remove=True)            # the pivot of the downdate fails
    opt.remove_data_point(0)
    assert opt.gps[0]._dev.calls == [("remove", 0), ("set_data", 3)]
    assert opt.gps[0].X[:, 0].tolist() == [1.0, 3.0, 4.0] and not opt.gps[0]._dev.removed
    opt = _fake_opt(LOG, incremental=False)           # no one-row updates asked for
    opt.remove_data_point(3)
    assert opt.gps[0]._dev.calls == [("set_data", 3)]
    assert opt.gps[1]._dev.calls == [("set_data", 2)]
    gp = _fake_gp(np.zeros((1, 1)), np.zeros((1, 1)))
    with pytest.raises(ValueError):
        gp.remove_data(0)
    with pytest.raises(IndexError):
        _fake_gp(np.zeros((3, 1)), np.zeros((3, 1))).remove_data(3)


def test_remove_last_data_point_still_pops():
    opt = _fake_opt(LOG)
    opt.remove_last_data_point()
    assert opt.gps[0]._dev.calls == [("pop",)] and opt.gps[1]._dev.calls == []


# ---- the choice of confidence() ----------------------------------------------------------------
class _FakeGrid(object):
    def __init__(self):
        self.calls = []

    def confidence(self, devs, beta, fmin, defer=False):
        self.calls.append(("sweep", None))
        return 0.0, True

    def rank1_update(self, devs, which, beta, fmin, defer=False):
        self.calls.append(("rank1_update", list(which)))
        return 0.0, True

    def rank1_remove(self, devs, which, beta, fmin, defer=False):
        self.calls.append(("rank1_remove", list(which)))
        return 0.0, True


def _backend(devs):
    be = object.__new__(gp_opt._HipGridBackend)
    be._dev = lambda: devs
    be.gps = devs
    be.grid = _FakeGrid()
    be._seen = [None] * len(devs)
    be._rank1_streak = 0
    be.incremental, be.refresh_every = True, 16
    return be


def test_confidence_takes_the_removal_refresh():
    devs = [_FakeDev(20), _FakeDev(20), _FakeDev(20)]
    be = _backend(devs)
    be.confidence(2.0, [0.0] * 3)
    assert be.grid.calls == [("sweep", None)] and be._rank1_streak == 0
    devs[0].remove(3)
    devs[2].remove(5)
    be.confidence(2.0, [0.0] * 3)
    assert be.grid.calls[-1] == ("rank1_remove", [1, 0, 1]) and be._rank1_streak == 1
    devs[1].append(None, 0.0)
    be.confidence(2.0, [0.0] * 3)
    assert be.grid.calls[-1] == ("rank1_update", [0, 1, 0]) and be._rank1_streak == 2
    be.confidence(2.0, [0.0] * 3)                     # nothing changed: the sweep of old
    assert be.grid.calls[-1] == ("sweep", None) and be._rank1_streak == 0


def test_confidence_sweeps_when_a_refresh_does_not_fit():
    def fresh():
        devs = [_FakeDev(20), _FakeDev(20)]
        be = _backend(devs)
        be.confidence(2.0, [0.0, 0.0])
        return devs, be
    devs, be = fresh()                                # an append here, a removal there
    devs[0].append(None, 0.0)
    devs[1].remove(4)
    be.confidence(2.0, [0.0, 0.0])
    assert be.grid.calls[-1] == ("sweep", None) and be._rank1_streak == 0
    devs, be = fresh()                                # two changes since the last sweep
    devs[0].remove(4)
    devs[0].remove(4)
    be.confidence(2.0, [0.0, 0.0])
    assert be.grid.calls[-1] == ("sweep", None)
    devs, be = fresh()                                # a removal, then a refit
    devs[0].remove(4)
    be.confidence(2.0, [0.0, 0.0])
    devs[0].set_data(np.zeros((5, 1)), np.zeros(5))
    be.confidence(2.0, [0.0, 0.0])
    assert [c[0] for c in be.grid.calls] == ["sweep", "rank1_remove", "sweep"]
    devs, be = fresh()                                # the streak is shared with the appends
    be.refresh_every = 3
    for t in range(4):
        (devs[0].remove(0) if t % 2 else devs[0].append(None, 0.0))
        be.confidence(2.0, [0.0, 0.0])
    assert [c[0] for c in be.grid.calls[1:]] == ["rank1_update", "rank1_remove", "rank1_update",
                                                 "sweep"]
    assert be._rank1_streak == 0
    devs, be = fresh()
    be.incremental = False
    devs[0].remove(1)
    be.confidence(2.0, [0.0, 0.0])
    assert be.grid.calls[-1] == ("sweep", None)
