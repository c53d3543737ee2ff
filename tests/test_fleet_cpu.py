"""``SafeOptFleet`` without a GPU: on the NumPy stand-in for the grid backend, which has no
one-launch step, a fleet is its members' own ``optimize()`` one after another -- the points,
the exception rules and the constructor's refusals."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import safeopt_amd
from _oracle_backend import OracleGridBackend
from oracle import gp_numpy as gpn
from safeopt_amd import gp_opt


@pytest.fixture
def oracle_backend():
    gp_opt._BACKEND_FACTORY = OracleGridBackend
    yield OracleGridBackend


def _opt(seed=3, fmin=0.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(5, 1))
    Y = 1.5 + 0.3 * np.sin(2 * X) + 0.01 * rng.normal(size=(5, 1))
    gp = gpn.GPRegression(X, Y, gpn.RBF(1, variance=1.0, lengthscale=0.7), noise_var=1e-4)
    grid = safeopt_amd.linearly_spaced_combinations([(-3.0, 3.0)], 61)
    return safeopt_amd.SafeOpt(gp, grid, fmin, threshold=0.05)


def test_fleet_is_exported():
    assert safeopt_amd.SafeOptFleet is gp_opt.SafeOptFleet
    assert "SafeOptFleet" in safeopt_amd.__all__


def test_fleet_falls_back_to_the_members_own_optimize(oracle_backend):
    seeds = (3, 4, 5)
    fleet = safeopt_amd.SafeOptFleet([_opt(s) for s in seeds])
    twins = [_opt(s) for s in seeds]
    assert len(fleet) == 3
    for _ in range(2):
        X = fleet.optimize()
        assert isinstance(X, list) and len(X) == 3
        for o, t, x in zip(fleet.opts, twins, X):
            xt = t.optimize()
            assert_array_equal(x, xt)
            for name in "QSMG":
                assert_array_equal(getattr(o, name), getattr(t, name))
            y = np.array([[1.5 + 0.3 * np.sin(2 * float(x[0]))]])
            o.add_new_data_point(x, y)
            t.add_new_data_point(xt, y)


def test_exceptions_stand_in_place_or_are_raised_after_every_member(oracle_backend):
    def members():
        return [_opt(3), _opt(4, fmin=10.0), _opt(5), _opt(6, fmin=10.0)]

    twins = members()
    fleet = safeopt_amd.SafeOptFleet(members())
    X = fleet.optimize(return_exceptions=True)
    assert isinstance(X[1], EnvironmentError) and isinstance(X[3], EnvironmentError)
    for b in (0, 2):
        assert_array_equal(X[b], twins[b].optimize())
    # raised: the first one in member order, and only after all members were stepped
    fleet = safeopt_amd.SafeOptFleet(members())
    with pytest.raises(EnvironmentError):
        fleet.optimize()
    for b in (0, 2):
        for name in "QSMG":
            assert_array_equal(getattr(fleet.opts[b], name), getattr(twins[b], name))
    with pytest.raises(ValueError):
        fleet.optimize(contexts=[None])


def test_constructor_refusals(oracle_backend):
    class TwoRanks(object):
        world, rank = 2, 0

    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([])
    with pytest.raises(TypeError):
        safeopt_amd.SafeOptFleet([_opt(), object()])
    a, b = _opt(3), _opt(4)
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, b, a])
    shared = safeopt_amd.SafeOpt(a.gps[0], a.parameter_set, 0.0, threshold=0.05)
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, shared])
    b._comm = TwoRanks()
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, b])
    c = _opt(5)
    c._backend.ctx = object()
    with pytest.raises(ValueError):
        safeopt_amd.SafeOptFleet([a, c])
    assert len(safeopt_amd.SafeOptFleet([a, _opt(6)])) == 2
