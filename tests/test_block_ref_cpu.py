"""CPU side of the block-append tests: the reference of tests/test_gpu_block.py checked against
itself, and the host logic of ``add_new_data_points`` and of the backend's choice between the
block refresh, the rank-1 refresh and a sweep, with stub handles (no GPU).

Figures (long double, this module's own run):
  * the tail-row formula of DESIGN.md 4.4b against the refit: at most 1e-17 on mean
    (relative to max |mean|) and on var / k(x, x) over all cases -- asked: 1e-12, a thousandth
    of the GPU tolerance, so that the formula's own rounding cannot show there;
  * the update without cross terms misses the refit by 2e-2 .. 3 in every case -- asked:
    100 x 1e-9;
  * rows excluded from the comparison of S: none in any case -- asked: at most 1 %.
"""
import os
import re

import numpy as np
import pytest

import _block_ref as B
import _incremental_ref as R
from _gpu_common import MEAN_TOL, VAR_TOL

import safeopt_amd.gpy as gpy
from safeopt_amd import _hip
from safeopt_amd.gp_opt import GaussianProcessOptimization, _HipGridBackend

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMULA_TOL = 1e-12


def _flagged(name):
    c = B.RANKB_CASES[name]
    return [g for g in range(len(c["gps"])) if c["b"][g]]


def _errors(pair, st, g, kd):
    m, v = pair
    em = float(np.max(np.abs(m - st["mean_ld"][g])) / np.max(np.abs(st["mean_ld"][g])))
    ev = float(np.max(np.abs(v - st["var_ld"][g])) / kd)
    return em, ev


@pytest.mark.parametrize("name", sorted(B.RANKB_CASES))
def test_tail_row_formula_reproduces_the_refit(name):
    """mean += sum_j t_j gamma_j, var -= sum_j t_j^2 with t_j = (row n0 + j of L'^-1) . k(X', x)
    and gamma_j = (row n0 + j) . y', in long double, against ``RefGP.append`` b times."""
    ref = B.rankb_reference(name)
    for t, st in enumerate(ref["steps"]):
        for g in _flagged(name):
            em, ev = _errors(st["tail"][g], st, g, ref["kdiag"][g])
            print("%s step %d GP %d: mean %.2e  var %.2e" % (name, t, g, em, ev))
            assert em < FORMULA_TOL and ev < FORMULA_TOL


@pytest.mark.parametrize("name", sorted(B.RANKB_CASES))
def test_cases_tell_a_missing_cross_term(name):
    """The b rows as independent rank-1 corrections of the OLD GP: off by at least 100 x the
    tolerance for every flagged GP (b >= 2), or the case could not tell a missing cross term."""
    ref = B.rankb_reference(name)
    for t, st in enumerate(ref["steps"]):
        for g in _flagged(name):
            assert B.RANKB_CASES[name]["b"][g] >= 2
            em, ev = _errors(st["naive"][g], st, g, ref["kdiag"][g])
            print("%s step %d GP %d: naive mean %.2e  var %.2e" % (name, t, g, em, ev))
            assert max(em / MEAN_TOL, ev / VAR_TOL) >= 100.0


@pytest.mark.parametrize("name", sorted(B.RANKB_CASES))
def test_few_rows_are_excluded_from_S(name):
    ref = B.rankb_reference(name)
    for st in ref["steps"]:
        n_ex = int(np.count_nonzero(st["excluded"]))
        print("%s: %d of %d rows excluded" % (name, n_ex, st["excluded"].size))
        assert n_ex <= 0.01 * st["excluded"].size


def test_case_tables_are_what_the_issue_lists():
    for name, (n0, n1) in B.APPEND_BLOCK_CASES.items():
        assert R.APPEND_CASES[name][2] == n0 and 1 <= n1 - n0 <= B.MAX_BLOCK
    assert sorted(n1 - n0 for n0, n1 in B.APPEND_BLOCK_CASES.values()) == [1, 3, 4, 4, 4, 4, 4, 16]
    assert B.RANKB_CASES["g1_mat52_d8_lds"]["gps"][0][2] == 668
    assert B.RANKB_CASES["b16_mat52_d2_N4099"]["gps"][0][2] == 56


def test_constants_match_the_header():
    text = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    assert int(re.search(r"#define SGP_MAX_BLOCK (\d+)", text).group(1)) == _hip.MAX_BLOCK == 16
    for name in ("sgp_gp_append_block", "sgp_grid_rankb_update"):
        assert name in _hip.PROTOTYPES and re.search(r"\b%s\s*\(" % name, text)


# ---- add_new_data_points with stub GP handles ------------------------------------------------
class StubGP(object):
    """Host-only handle that records how its data arrived."""

    def __init__(self, X, Y, kernel):
        self.kern = kernel
        self.input_dim = np.atleast_2d(X).shape[1]
        self.calls = []
        self.set_XY(X, Y)
        self.calls = []

    def set_XY(self, X, Y):
        self.X = np.array(np.atleast_2d(X), dtype=float)
        self.Y = np.array(np.atleast_2d(Y), dtype=float)
        self.calls.append(("set_XY", self.X.shape[0]))

    def append_XY(self, X, Y):
        X, Y = np.atleast_2d(X), np.atleast_2d(Y)
        assert X.shape[0] == Y.shape[0] and Y.shape[1] == 1
        self.X, self.Y = np.vstack([self.X, X]), np.vstack([self.Y, Y])
        self.calls.append(("append_XY", X.shape[0]))

    def remove_data(self, index):
        self.set_XY(np.delete(self.X, index, axis=0), np.delete(self.Y, index, axis=0))


def _opts(num_contexts=0):
    d = 2 + num_contexts
    out = []
    for _ in range(2):
        gps = [StubGP(np.zeros((1, d)), [[1.0 + g]], gpy.kern.RBF(d)) for g in range(3)]
        out.append(GaussianProcessOptimization(gps, fmin=[0.0] * 3, num_contexts=num_contexts))
    return out


def test_add_new_data_points_routes_nan_columns_and_logs_like_single_calls():
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, size=(5, 2))
    Y = rng.normal(size=(5, 3))
    Y[1, 1] = Y[3, 1] = np.nan              # GP 1 misses two rows
    Y[:, 2] = np.nan                        # GP 2 observes nothing
    a, b = _opts()
    a.add_new_data_points(X, Y)
    for x, y in zip(X, Y):
        b.add_new_data_point(x, y)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y, equal_nan=True)
    assert a.t == b.t == 6 and a.data[0] is a.x
    for ga, gb in zip(a.gps, b.gps):
        assert np.array_equal(ga.X, gb.X) and np.array_equal(ga.Y, gb.Y)
    assert [g.calls for g in a.gps] == [[("append_XY", 5)], [("append_XY", 3)], []]
    assert np.array_equal(a.gps[1].X[1:], X[[0, 2, 4]])
    assert np.array_equal(a.gps[1].Y[1:, 0], Y[[0, 2, 4], 1])
    # ... and the removals work on the result as before
    a.remove_last_data_point()
    b.remove_last_data_point()
    a.remove_data_point(2)
    b.remove_data_point(2)
    assert np.array_equal(a.x, b.x) and np.array_equal(a.y, b.y, equal_nan=True)
    for ga, gb in zip(a.gps, b.gps):
        assert np.array_equal(ga.X, gb.X) and np.array_equal(ga.Y, gb.Y)


def test_add_new_data_points_with_contexts_and_bad_shapes():
    a, b = _opts(num_contexts=1)
    X = np.array([[0.1, 0.2], [0.3, 0.4]])
    Y = np.array([[1.0, 2.0, 3.0], [4.0, np.nan, 6.0]])
    a.add_new_data_points(X, Y, context=[0.7])
    for x, y in zip(X, Y):
        b.add_new_data_point(x, y, context=[0.7])
    assert np.array_equal(a.x, b.x) and a.x.shape == (3, 3) and np.all(a.x[1:, 2] == 0.7)
    assert np.array_equal(a.y, b.y, equal_nan=True)
    for ga, gb in zip(a.gps, b.gps):
        assert np.array_equal(ga.X, gb.X) and np.array_equal(ga.Y, gb.Y)
    with pytest.raises(ValueError):
        a.add_new_data_points(X, Y[:, :2], context=[0.7])
    with pytest.raises(ValueError):
        a.add_new_data_points(X[:1], Y, context=[0.7])
    assert a.t == 3


def test_a_handle_without_append_XY_is_refitted():
    class Plain(object):
        def __init__(self):
            self.kern, self.input_dim = gpy.kern.RBF(1), 1
            self.X, self.Y = np.zeros((1, 1)), np.ones((1, 1))

        def set_XY(self, X, Y):
            self.X, self.Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)

    opt = GaussianProcessOptimization(Plain(), fmin=0.0)
    opt.add_new_data_points([[1.0], [2.0]], [[3.0], [4.0]])
    assert np.array_equal(opt.gp.X[:, 0], [0.0, 1.0, 2.0])
    assert np.array_equal(opt.gp.Y[:, 0], [1.0, 3.0, 4.0])


# ---- the backend's choice ---------------------------------------------------------------------
class StubDev(object):
    def __init__(self, serial):
        self.serial, self.version = serial, 1
        self.appended = self.removed = False
        self.block = 0

    def _fitted(self):
        return self

    def append(self):
        self.version += 1
        self.appended, self.removed, self.block = True, False, 0

    def append_block(self, b):
        self.version += 1
        self.appended, self.removed, self.block = False, False, b

    def remove(self):
        self.version += 1
        self.appended, self.removed, self.block = False, True, 0


class StubGrid(object):
    def __init__(self):
        self.log = []

    def confidence(self, devs, beta, fmin, defer=False):
        self.log.append(("sweep", None))

    def rank1_update(self, devs, which, beta, fmin, defer=False):
        self.log.append(("rank1", list(which)))

    def rank1_remove(self, devs, which, beta, fmin, defer=False):
        self.log.append(("remove", list(which)))

    def rankb_update(self, devs, which, beta, fmin, defer=False):
        self.log.append(("block", list(which)))


def _backend(G=2):
    be = object.__new__(_HipGridBackend)
    be.gps = [StubDev(10 + g) for g in range(G)]
    be.grid = StubGrid()
    be._seen = [None] * G
    be._rank1_streak = 0
    be.incremental = True
    be.refresh_every = 16
    be.confidence(2.0, [0.0] * G)
    assert be.grid.log.pop() == ("sweep", None) and be._rank1_streak == 0
    return be


def _step(be):
    be.confidence(2.0, [0.0] * len(be.gps))
    return be.grid.log[-1], be._rank1_streak


def test_backend_one_block_is_a_block_refresh():
    be = _backend()
    for dv in be.gps:
        dv.append_block(4)
    assert _step(be) == (("block", [1, 1]), 4)


def test_backend_blocks_of_different_size_and_a_current_gp():
    be = _backend(3)
    be.gps[0].append_block(3)
    be.gps[2].append_block(2)
    assert _step(be) == (("block", [1, 0, 1]), 3)          # the streak counts max_g b_g


def test_backend_block_after_a_single_append_is_a_sweep():
    be = _backend()
    for dv in be.gps:
        dv.append()
        dv.append_block(4)                                  # two versions behind
    assert _step(be) == (("sweep", None), 0)
    # ... and mixed kinds one version behind each
    be.gps[0].append()
    be.gps[1].append_block(2)
    assert _step(be) == (("sweep", None), 0)
    be.gps[0].remove()
    be.gps[1].append_block(2)
    assert _step(be) == (("sweep", None), 0)


def test_backend_two_chunks_are_a_sweep():
    be = _backend()
    for dv in be.gps:
        dv.append_block(16)
        dv.append_block(4)                                  # a block of 20 arrives in two chunks
    assert _step(be) == (("sweep", None), 0)


def test_backend_streak_counts_rows():
    be = _backend()
    for expect in (8, 16):
        for dv in be.gps:
            dv.append_block(8)
        assert _step(be) == (("block", [1, 1]), expect)
    for dv in be.gps:
        dv.append_block(1)                                  # 16 + 1 > refresh_every
    assert _step(be) == (("sweep", None), 0)
    for dv in be.gps:
        dv.append_block(16)                                 # a whole budget in one block
    assert _step(be) == (("block", [1, 1]), 16)
    for dv in be.gps:
        dv.append()
    assert _step(be) == (("sweep", None), 0)


def test_backend_single_appends_behave_as_before():
    be = _backend()
    for t in range(16):
        for dv in be.gps:
            dv.append()
        assert _step(be) == (("rank1", [1, 1]), t + 1)
    for dv in be.gps:
        dv.append()
    assert _step(be) == (("sweep", None), 0)
    be.gps[0].remove()
    assert _step(be) == (("remove", [1, 0]), 1)
    be.gps[1].append_block(4)
    assert _step(be) == (("block", [0, 1]), 5)
    be.incremental = False
    be.gps[1].append_block(4)
    assert _step(be) == (("sweep", None), 0)
