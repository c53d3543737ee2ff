"""Max-value entropy search without a GPU: the yardstick (tests/_mes_ref.py: the float64
restatement of the device's stable form against a 50-digit evaluation of the definition), the
host logic of ``SafeOpt.mes_point``, the record merge of ``dist.py`` and the declarations."""
import functools
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _mes_ref as ref                                                     # noqa: E402


@functools.lru_cache(maxsize=None)
def _reference():
    """(gamma, the restatement, its error in units of EPS (1 + gamma^2 / 2)), once."""
    g = ref.gamma_set()
    got = ref.term(g)
    return g, got, ref.units(got, g, ref.term_mp(g))


# ---- 1. the restatement against mpmath ---------------------------------------------------------

def test_restatement_is_finite_and_within_four_units():
    g, got, u = _reference()
    assert g.size == 5201 and np.all(np.isfinite(got))
    print("restatement: max error %.3f units of EPS (1 + g^2 / 2), at gamma = %r"
          % (u.max(), g[np.argmax(u)]))
    assert u.max() <= 4.0


def test_restatement_is_monotone_on_the_right_and_zero_from_39():
    g = np.linspace(0.0, 40.0, 1601)
    t = ref.term(g)
    assert np.all(np.diff(t) <= 0.0) and np.all(t >= 0.0)
    far = np.array([39.0, 40.0, 100.0, 1e8, 1e300, np.inf])
    assert np.all(ref.term(far) == 0.0)
    assert ref.term(np.array([38.0]))[0] > 0.0
    # both zeros: ln 2
    assert ref.term(np.array([0.0]))[0] == ref.term(np.array([-0.0]))[0] == np.log(2.0)


def test_restatement_survives_where_the_naive_form_does_not():
    from scipy.special import ndtr
    g = np.array([-40.0, -39.0])
    with np.errstate(all='ignore'):
        naive = g * np.exp(-0.5 * g * g) / np.sqrt(2 * np.pi) / (2 * ndtr(g)) - np.log(ndtr(g))
    assert not np.all(np.isfinite(naive))
    assert np.all(np.isfinite(ref.term(g)))


def test_alpha_applies_floor_and_order():
    mean, var = np.array([0.3, -1.0, 2.0]), np.array([0.5, 1e-30, 4.0])
    ys = np.array([0.1, 1.7, 0.9])
    a = ref.alpha(mean, var, ys, floor=1.0)
    sig = np.sqrt(np.maximum(var, 1e-15))
    want = (ref.term((1.0 - mean) / sig) + ref.term((1.7 - mean) / sig)
            + ref.term((1.0 - mean) / sig)) / 3.0
    assert np.array_equal(a, want)
    assert np.all(ref.alpha(mean, var, ys, floor=np.inf) == 0.0)


# ---- 2. the host logic of mes_point ------------------------------------------------------------

def _oracle_opt():
    import safeopt_amd
    from oracle import gp_numpy as gpn
    from _oracle_backend import use_oracle_backend
    use_oracle_backend()
    x = np.linspace(-1.0, 1.0, 5)[:, None]
    gp = gpn.GPRegression(x, np.cos(x) + 1.0, gpn.RBF(1, 1.0, 0.5), noise_var=1e-4)
    return safeopt_amd.SafeOpt(gp, np.linspace(-2.0, 2.0, 50)[:, None], 0.0)


@pytest.mark.parametrize("kw", [dict(within='M'), dict(within=None), dict(paths=0),
                                dict(paths=65), dict(floor='max'), dict(floor=float('nan'))])
def test_mes_point_refuses_bad_arguments(kw):
    opt = _oracle_opt()
    with pytest.raises(ValueError):
        opt.mes_point(**kw)


def test_mes_point_needs_a_backend_with_mes():
    from _oracle_backend import OracleGridBackend
    assert not hasattr(OracleGridBackend, 'mes')
    opt = _oracle_opt()
    with pytest.raises(NotImplementedError):
        opt.mes_point()


def test_mes_point_needs_collectives_on_several_ranks():
    opt = _oracle_opt()

    class Mute(object):
        rank, world = 0, 2
    opt._comm = Mute()
    with pytest.raises(NotImplementedError, match="allreduce_max and allgather"):
        opt.mes_point()


@pytest.mark.parametrize("name", ["line", "plane"])
def test_seeds_of_the_end_to_end_picks_are_decided(name):
    """tests/test_gpu_mes.py compares ``mes_point``'s pick with the arg-max of the restatement:
    for its seeds the two largest alpha over S are more than 1e-9 apart (oracle posterior,
    NumPy paths), the pick is not the row of the smallest sigma -- and maxima pushed far below
    the mean, without a floor, do pick that row."""
    import _mes_problems as P
    mean, var, S = P.host_state(name)
    ids = np.flatnonzero(S)
    smallest = ids[np.argmin(var[S])]
    assert 1 < S.sum() < S.size
    for seed in P.SEEDS[name]:
        ystar = P.host_ystar(name, seed, S)
        a = ref.alpha(mean, var, ystar, floor=mean[S].max())
        assert P.top_two_gap(a, S) > 1e-9
        assert ids[np.argmax(a[S])] != smallest
    low = ref.alpha(mean, var, np.full(P.PATHS, mean[S].min() - 50.0))
    assert ids[np.argmax(low[S])] == smallest


# ---- 3. the record merge -----------------------------------------------------------------------

def test_merge_mes_records():
    from safeopt_amd.dist import merge_mes_records
    inf = np.inf
    # the lowest global row among equal values, whatever the rank order
    assert merge_mes_records([[0.5, 40.0], [0.5, 7.0], [0.2, 90.0]]) == (0.5, 7)
    assert merge_mes_records([[0.5, 7.0], [0.5, 40.0]]) == (0.5, 7)
    # the largest value
    assert merge_mes_records([[0.1, 3.0], [0.9, 800.0]]) == (0.9, 800)
    # a record without a row never wins: not with -inf, not with a value left in it
    assert merge_mes_records([[-inf, -1.0], [0.0, 12.0]]) == (0.0, 12)
    assert merge_mes_records([[5.0, -1.0], [0.0, 12.0]]) == (0.0, 12)
    assert merge_mes_records([[-inf, 12.0], [-inf, -1.0]]) == (-inf, 12)
    # no rank has a row
    assert merge_mes_records([[-inf, -1.0], [-inf, -1.0]]) == (-inf, -1)
    v, i = merge_mes_records(np.array([[0.25, 2.0 ** 40]]))
    assert (v, i) == (0.25, 2 ** 40) and isinstance(i, int)


# ---- 4. the declarations -----------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sgp_mes_eval", "sgp_grid_mes", "sgp_grid_mes_comm"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"#define\s+SGP_MAX_MES\s+64\b", code)
    for name, val in (("SGP_MES_ALL", 0), ("SGP_MES_S", 1), ("SGP_MES_MG", 2),
                      ("SGP_MES_FLOOR_NONE", 0), ("SGP_MES_FLOOR_MEAN", 1),
                      ("SGP_MES_FLOOR_VALUE", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), code), name
    from safeopt_amd import _hip
    assert (_hip.MES_ALL, _hip.MES_S, _hip.MES_MG) == (0, 1, 2)
    assert (_hip.MES_FLOOR_NONE, _hip.MES_FLOOR_MEAN, _hip.MES_FLOOR_VALUE) == (0, 1, 2)
    assert _hip.MAX_MES == 64 == _hip.MAX_PATHS
    for name in ("sgp_mes_eval", "sgp_grid_mes", "sgp_grid_mes_comm"):
        assert name in _hip.PROTOTYPES


def test_mes_source_is_built_without_contraction():
    from safeopt_amd import build
    assert "mes.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA["mes.hip"]
