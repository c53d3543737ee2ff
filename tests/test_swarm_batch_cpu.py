"""SafeOptSwarm.optimize_batch without a GPU: the algebra of DESIGN.md 4.13 in NumPy, the
choice between the two candidates, the loop over the picks on fake device GPs, the argument
errors.  The device side: tests/test_gpu_swarm_batch.py."""
import logging
import types

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _paths_numpy as pn
import _swarm_batch_ref as ref
from _gpu_common import VAR_TOL
from safeopt_amd import _hip
from safeopt_amd import gp_opt
from safeopt_amd.dist import LocalComm


# ---- the algebra -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_tail_rows_equal_the_refit(case):
    """var - sum_j t_j^2 (float64) against the posterior refitted on X plus the pending picks in
    long double: at least 100 x inside the bound the device variance is held to (2 VAR_TOL
    k(x, x)), so the reference itself does not eat the tolerance."""
    kerns = ref.problem(case)[0]
    pend = ref.pending(case)
    var, down, var_h = ref.tail_row_var_h(case, pend)
    slow = ref.refit_var_h(case, pend, dtype=np.longdouble)
    for g in range(case[5]):
        kdiag = pn.prior_variance(kerns[g])
        err = float(np.max(np.abs(var_h[g] - slow[g]))) / kdiag
        print("GP %d: max |tail rows - refit| / k(x, x) = %.3e" % (g, err))
        assert err <= 2 * VAR_TOL / 100
        assert np.all(down[g] >= 0) and np.all(var_h[g] <= var[g])
    # the downdate is really there: the pending pick that equals a particle (row 100 of the
    # 5000) takes most of its variance
    i = 100 if case[4] == 5000 else 0
    assert var_h[0][i] < 0.5 * var[0][i] or var[0][i] < 2 * ref.NOISE


@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_a_far_pending_point_takes_nothing(case):
    """A pending pick 400 lengthscales from everything: k underflows to 0, down == 0 exactly,
    var_h == var."""
    var, down, var_h = ref.tail_row_var_h(case, ref.pending(case, far_only=True))
    assert np.all(down == 0.0)
    assert_array_equal(var_h, var)


@pytest.mark.parametrize("case", ref.FORMULA_CASES, ids=ref.FORMULA_IDS)
def test_fmin_keeps_the_particles_off_the_band_edges(case):
    """The constraints of the whole-formula test split the particles, keep every scaled slack
    above -1 and leave (almost) no particle within EDGE_GAP of a band edge."""
    G, P = case[5], case[4]
    mean, var = ref.real_posterior(case)
    fmin = ref.fmin_of(case)
    assert fmin.shape == (G,) and np.all(np.isfinite(fmin))
    for st in ("maximizers", "expanders"):
        _, safe, scaled, _ = ref.hall_fitness(st, mean, var, var, fmin, ref.SCALING,
                                              ref.best_lower_bound_of(case))
        assert 0 < safe.sum() < P
        assert scaled.min() > -1.0
        near = ref.near_band_edge(scaled)
        print("%s: %d of %d particles near a band edge" % (st, np.count_nonzero(near), P))
        assert np.count_nonzero(near) <= 0.01 * P


def test_restated_fitness_is_the_plain_one_without_pending_picks():
    """var_h = var: the restatement is SafeOptSwarm's own fitness, (sd / scaling + pen) x
    interest, on hand-made numbers."""
    mean = np.array([[1.0, 0.2], [0.5, 0.4]])
    var = np.array([[0.04, 0.09], [0.01, 0.16]])
    fmin = np.array([-np.inf, 0.0])
    scaling = np.array([2.0, 0.5, 1.0])
    v, safe, scaled, (width, pen, interest) = ref.hall_fitness("expanders", mean, var, var, fmin,
                                                               scaling, 0.0, beta=2.0)
    assert_array_equal(width, np.maximum(np.sqrt(var[0]) / 2.0, np.sqrt(var[1]) / 0.5))
    assert_array_equal(safe, [True, False])
    np.testing.assert_allclose(scaled[1], [(0.5 - 0.2) / 0.5, (0.4 - 0.8) / 0.5])
    np.testing.assert_allclose(pen, [0.0, 10 * -0.8])
    z = scaled[1] / 0.2
    np.testing.assert_allclose(interest, 2 * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) / 0.2)
    vm = ref.hall_fitness("maximizers", mean, var, 0.25 * var, fmin, scaling, 1.0, beta=2.0)
    np.testing.assert_allclose(vm[3][0], 0.5 * width)
    np.testing.assert_allclose(vm[3][2], 1 / (1 + np.exp(-10 * (mean[0] + 2 * np.sqrt(var[0]) - 1.0)
                                                       / 2.0)))
    assert_array_equal(vm[1], safe)


# ---- step 3: the choice between the candidates ------------------------------------------------

def test_choice_strict_threshold_unconstrained_and_ucb():
    scaling = np.array([2.0, 0.5])
    fmin = np.array([-np.inf, 0.0])
    choose = gp_opt.swarm_batch_choice
    # maximiser 0.8 / 2 = 0.4; expander: GP 0 does not count (fmin = -inf), GP 1 0.1 / 0.5 = 0.2
    assert choose([0.8, 9.0], [5.0, 0.1], scaling, fmin, 0.0) == "maximizers"
    # equal values: the maximiser wins only when strictly larger
    assert choose([0.8, 0.0], [0.0, 0.2], scaling, fmin, 0.0) == "expanders"
    assert choose(np.array([0.8, 0.0]), np.array([0.0, 0.2 * (1 - 1e-15)]), scaling, fmin,
                  0.0) == "maximizers"
    # below the threshold the expander's GP does not count: value 0, and 0 > 0 is false
    assert choose([0.8, 0.0], [0.0, 0.3], scaling, fmin, 0.31) == "maximizers"
    assert choose([0.0, 0.0], [0.0, 0.3], scaling, fmin, 0.31) == "expanders"
    assert choose([0.8, 0.0], [0.0, 0.3], scaling, fmin, 0.3) == "expanders"      # >= threshold
    # a finite fmin for GP 0 makes it count
    assert choose([0.8, 0.0], [1.0, 0.0], scaling, np.array([0.0, 0.0]), 0.0) == "expanders"
    # ucb: always the maximiser
    assert choose([0.1, 0.0], [0.0, 9.0], scaling, fmin, 0.0, ucb=True) == "maximizers"
    assert choose([0.1, 0.0], None, scaling, fmin, 0.0, ucb=True) == "maximizers"
    # a swarm without a candidate
    assert choose(None, [0.0, 9.0], scaling, fmin, 0.0) == "expanders"
    assert choose([0.1, 0.0], None, scaling, fmin, 0.0) == "maximizers"
    assert choose(None, None, scaling, fmin, 0.0) is None
    assert choose(None, [0.0, 9.0], scaling, fmin, 0.0, ucb=True) is None


def test_choice_equals_the_restatement_on_random_numbers():
    rng = np.random.RandomState(4)
    for _ in range(300):
        G = rng.randint(1, 4)
        sd_m = rng.choice([0.0, 0.1, 0.2, 0.4], size=G)
        sd_e = rng.choice([0.0, 0.1, 0.2, 0.4], size=G)
        scaling = rng.choice([0.5, 1.0, 2.0], size=G)
        fmin = np.where(rng.rand(G) < 0.4, -np.inf, 0.0)
        thr = float(rng.choice([0.0, 0.15, 0.2]))
        ucb = bool(rng.rand() < 0.2)
        m = None if rng.rand() < 0.1 else sd_m
        e = None if rng.rand() < 0.1 else sd_e
        assert gp_opt.swarm_batch_choice(m, e, scaling, fmin, thr, ucb=ucb) == \
            ref.batch_choice_reference(m, e, scaling, fmin, thr, ucb)


# ---- steps 2 and 4: the loop on fake device GPs ------------------------------------------------

class _FakeClone(object):
    def __init__(self, log, fail_at):
        self.log, self.fail_at, self.rows, self.alive = log, fail_at, [], True

    def append(self, x, y):
        assert self.alive and y == 0.0
        self.rows.append(np.array(x))
        self.log.append(("append", len(self.rows)))
        return len(self.rows) != self.fail_at

    def destroy(self):
        self.alive = False
        self.log.append(("destroy",))


class _FakeDev(object):
    def __init__(self, log, fail_at=0):
        self.log, self.fail_at, self.clones = log, fail_at, []

    def clone(self):
        self.clones.append(_FakeClone(self.log, self.fail_at))
        return self.clones[-1]


def _picker(log, stop_after=99, boom_at=0):
    def next_pick(clones):
        b = len(clones[0].rows)
        assert all(len(c.rows) == b and c.alive for c in clones)
        log.append(("pick", b))
        if b == boom_at:
            raise RuntimeError("boom")
        if b > stop_after:
            return None
        return np.array([10.0 * b, -b]), np.array([0.5 / b, 0.25 / b])
    return next_pick


def test_loop_appends_then_picks_and_releases_the_clones():
    log = []
    devs = [_FakeDev(log), _FakeDev(log)]
    X, sd = gp_opt.swarm_batch_loop(np.array([1.0, 2.0]), np.array([0.7, 0.3]), 4, devs,
                                    _picker(log))
    assert_array_equal(X, [[1.0, 2.0], [10.0, -1], [20.0, -2], [30.0, -3]])
    assert_array_equal(sd, [[0.7, 0.3], [0.5, 0.25], [0.25, 0.125], [0.5 / 3, 0.25 / 3]])
    # every clone received the pick before, in order, before the next swarm ran
    for dv in devs:
        assert len(dv.clones) == 1 and not dv.clones[0].alive
        assert_array_equal(np.array(dv.clones[0].rows), X[:3])
    assert log == [("append", 1)] * 2 + [("pick", 1)] + [("append", 2)] * 2 + [("pick", 2)] + \
        [("append", 3)] * 2 + [("pick", 3)] + [("destroy",)] * 2


def test_size_one_clones_nothing():
    log = []
    X, sd = gp_opt.swarm_batch_loop(np.array([1.0]), np.array([0.7]), 1, [_FakeDev(log)],
                                    _picker(log))
    assert X.shape == (1, 1) and sd.shape == (1, 1) and log == []


def test_loop_ends_when_no_candidate_is_left():
    log = []
    devs = [_FakeDev(log)]
    X, sd = gp_opt.swarm_batch_loop(np.array([1.0, 2.0]), np.array([0.7, 0.3]), 6, devs,
                                    _picker(log, stop_after=2))
    assert X.shape == (3, 2) and sd.shape == (3, 2)
    assert not devs[0].clones[0].alive


def test_loop_ends_at_a_non_positive_pivot(caplog):
    log = []
    devs = [_FakeDev(log), _FakeDev(log, fail_at=3)]
    with caplog.at_level(logging.INFO, logger=gp_opt.__name__):
        X, sd = gp_opt.swarm_batch_loop(np.array([1.0, 2.0]), np.array([0.7, 0.3]), 6, devs,
                                        _picker(log))
    assert X.shape == (3, 2) and sd.shape == (3, 2)
    assert any("non-positive pivot" in r.getMessage() and r.levelno == logging.INFO
               for r in caplog.records)
    assert ("pick", 3) not in log
    assert all(not c.alive for dv in devs for c in dv.clones)


def test_loop_releases_the_clones_when_a_call_raises():
    log = []
    devs = [_FakeDev(log), _FakeDev(log)]
    with pytest.raises(RuntimeError, match="boom"):
        gp_opt.swarm_batch_loop(np.array([1.0, 2.0]), np.array([0.7, 0.3]), 6, devs,
                                _picker(log, boom_at=2))
    assert all(not c.alive for dv in devs for c in dv.clones)


# ---- errors ------------------------------------------------------------------------------------

class _Stub(object):
    """What optimize_batch touches before it runs anything."""

    def __init__(self, world=1):
        self._comm = types.SimpleNamespace(world=world, rank=0)
        self.calls = 0

    def optimize(self, ucb=False):
        self.calls += 1
        raise AssertionError("optimize() must not run")


@pytest.mark.parametrize("size", [0, -1, _hip.MAX_BATCH + 1])
def test_size_limits(size):
    stub = _Stub()
    with pytest.raises(ValueError, match="SGP_MAX_BATCH"):
        gp_opt.SafeOptSwarm.optimize_batch(stub, size=size)
    assert stub.calls == 0


def test_two_ranks_raise_before_anything_runs_or_is_drawn():
    stub = _Stub(world=2)
    state = np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError, match="one rank"):
        gp_opt.SafeOptSwarm.optimize_batch(stub, size=4)
    assert stub.calls == 0
    assert_array_equal(np.random.get_state()[1], state)
    assert LocalComm().world == 1


def test_abi_table_declares_the_entry_points():
    for name in ("sgp_swarm_fitness_hall", "sgp_swarm_run_hall"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.swarm_fitness_hall) and callable(_hip.swarm_run_hall)
    from safeopt_amd.swarm import DeviceSwarmOptimization
    assert callable(DeviceSwarmOptimization.set_clones)
