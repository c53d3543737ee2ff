"""Cases, maxima and the NumPy reference of the max-value entropy search swarm
(tests/test_gpu_swarm_mes.py, tests/test_swarm_mes_host.py).

The problems are those of tests/_swarm_thompson_ref.py -- n = 5 / 60 / 300 (one per posterior
kernel family), P = 1 / 37 / 5000 (a partial workgroup; below and above kSmallPoints = 4096, the
few-points / sweep split), d = 1 / 3, three kernel kinds -- de-duplicated over ``(kind, d, n,
P)``: a case differs from another in the number of path features m too, which MES ignores.  A
case keeps the five entries ``(kind, d, n, m, P)`` that ``problem(*case)`` takes.

The maxima of a case: ``ystar = linspace(min mean, max mean + 2, K)`` over the reference
posterior mean of GP 0 at the case's particles, with ``(K, floor)`` in ``MAXIMA``: one maximum,
a count that is no multiple of 4 under a floor at the median of that mean, and the cap
SGP_MAX_MES.  The reference alpha is ``_mes_ref.alpha``.
"""
import functools

import numpy as np

import _mes_ref
import _swarm_thompson_ref as tref
from _swarm_thompson_ref import (BETA, NOISE, SCALING, constraint_kernel, fmin_of,  # noqa: F401
                                 lower_bounds, make_kernel, near_band_edge, posterior, problem)

_seen, CASES, IDS = set(), [], []
for _c in tref.CASES:
    _key = (_c[0], _c[1], _c[2], _c[4])
    if _key not in _seen:
        _seen.add(_key)
        CASES.append(_c)
        IDS.append("%s-d%d-n%d-P%d" % _key)
PENALTY_CASES = [c for c in CASES if c[4] > 1]
PENALTY_IDS = [i for c, i in zip(CASES, IDS) if c[4] > 1]
assert sorted(set(c[4] for c in CASES)) == [1, 37, 5000]
assert sorted(set(c[2] for c in CASES)) == [5, 60, 300]

#: (K, floor): floor is -inf or 'median' (of the reference mean of GP 0 at the particles)
MAXIMA = [(1, -np.inf), (5, 'median'), (64, -np.inf)]
MAXIMA_IDS = ["K1-nofloor", "K5-median", "K64-nofloor"]


@functools.lru_cache(maxsize=None)
def posterior0(case):
    """(mean, var) of GP 0 at the particles of a case, in NumPy; computed once, read-only."""
    kern0, _, X, Y, particles = problem(*case)[:5]
    mean, var = posterior(kern0, X, Y[:, 0], particles)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


@functools.lru_cache(maxsize=None)
def maxima(case, K, floor):
    """``(ystar (K,), floor)`` of a case, the floor as a float."""
    mean = posterior0(case)[0]
    ystar = np.linspace(mean.min(), mean.max() + 2.0, K)
    ystar.setflags(write=False)
    return ystar, float(np.median(mean)) if isinstance(floor, str) else float(floor)


def gammas(case, K, floor):
    """(K, P) gamma_k = (max(ystar_k, floor) - mean) / sigma on the reference posterior."""
    mean, var = posterior0(case)
    ystar, fl = maxima(case, K, floor)
    sigma = np.sqrt(np.maximum(var, 1e-15))
    return (np.maximum(ystar, fl)[:, None] - mean[None, :]) / sigma[None, :]


def alpha(case, K, floor):
    """The reference alpha at the particles of a case, from the reference posterior."""
    mean, var = posterior0(case)
    ystar, fl = maxima(case, K, floor)
    return _mes_ref.alpha(mean, var, ystar, fl)
