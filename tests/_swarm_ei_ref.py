"""Cases, incumbents and the NumPy reference of the expected-improvement swarm
(tests/test_gpu_swarm_ei.py, tests/test_swarm_ei_host.py).

The cases are the de-duplicated ``CASES`` of tests/_swarm_mes_ref.py (shapes from
tests/_swarm_thompson_ref.py): n = 5 / 60 / 300 (one per posterior kernel family), P = 1 / 37 /
5000 (a lone particle, a partial workgroup; below and above kSmallPoints = 4096, the few-points
/ sweep split), d = 1 / 3.  A case keeps the five entries ``(kind, d, n, m, P)`` that
``problem(*case)`` takes.

The incumbents of a case come from the reference posterior mean ``m`` of GP 0 at the case's
particles, the margin is ``XI = 0``, and each aims at one branch of ``ei_log_h`` (csrc/ei_term.h)
through ``z = (m - tau) / sigma``:

    'median'   tau = median(m)      particles on both sides of z = -1: the direct form and the
                                    middle form (see below for the cases where one side is empty)
    'max+2'    tau = max(m) + 2     every particle in the middle form, -1e6 <= z < -1
    'max+1e7'  tau = max(m) + 1e7   every particle in the asymptotic form, z < -1e6

tests/test_swarm_ei_host.py asserts these claims on the NumPy posterior, so the GPU tests cannot
silently miss a branch.  The last two hold in every case.  'median' has particles on both sides
of z = -1 in five of the nine cases -- all three with 5000 particles, RBF-d3-n300-P37 (25 / 12)
and product-d3-n5-P37 (36 / 1) -- which is every n, both posterior routes and d = 1 and 3.  It
cannot in the three lone-particle cases (a particle sits on its own median: z = 0, the direct
form), and it does not in Matern52-d3-n60-P37, where sigma >= 0.2 at every particle and z spans
[-0.38, 0.96]: all 37 in the direct form.  ``BOTH_SIDES`` lists the five; the CPU test asserts
both sides for them, the direct form alone for the other four, and that the five cover every n
and both routes.  (The term is a function of a particle's (mean, var) alone -- one device
function -- so a branch reached in one case is the branch every case would take.)  The reference
alpha is ``_ei_ref.alpha``.
"""
import functools

import numpy as np

import _ei_ref
import _swarm_mes_ref as mref
from _swarm_mes_ref import (BETA, NOISE, SCALING, CASES, IDS, PENALTY_CASES,  # noqa: F401
                            PENALTY_IDS, constraint_kernel, fmin_of, lower_bounds, make_kernel,
                            near_band_edge, posterior, problem)

XI = 0.0
INCUMBENTS = ['median', 'max+2', 'max+1e7']
#: the incumbents under which the penalty identity is asserted (|alpha| ~ 5e13 under the third:
#: the rounding of alpha + pen swamps the penalty there)
PENALTY_INCUMBENTS = INCUMBENTS[:2]
KINDS = ['ei', 'pi']
#: the cases in which 'median' puts particles on both sides of z = -1 (module docstring)
BOTH_SIDES = ["product-d3-n300-P5000", "RBF-d3-n300-P37", "Matern52-d1-n5-P5000",
              "RBF-d1-n60-P5000", "product-d3-n5-P37"]
assert set(BOTH_SIDES) <= set(IDS)


@functools.lru_cache(maxsize=None)
def posterior_all(case):
    """(mean, var), each (2, P), of both GPs at the particles of a case, in NumPy; computed
    once, read-only."""
    kern0, kern1, X, Y, particles = problem(*case)[:5]
    out = [posterior(k, X, Y[:, g], particles) for g, k in enumerate((kern0, kern1))]
    mean, var = np.array([m for m, _ in out]), np.array([v for _, v in out])
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


@functools.lru_cache(maxsize=None)
def incumbent(case, which):
    """tau of a case: 'median', 'max+2' or 'max+1e7' of the reference mean of GP 0."""
    m = posterior_all(case)[0][0]
    return {'median': float(np.median(m)), 'max+2': float(m.max() + 2.0),
            'max+1e7': float(m.max() + 1e7)}[which]


def z_of(case, which):
    """(P,) z = (mean_0 - tau - XI) / sigma_0 on the reference posterior."""
    mean, var = posterior_all(case)
    return (mean[0] - incumbent(case, which) - XI) / np.sqrt(np.maximum(var[0], 1e-15))


def alpha(case, which, kind, fmin=None, G=2):
    """The reference alpha at the particles of a case, from the reference posterior of its
    first ``G`` GPs; ``fmin`` (G): the feasibility weights, ``None``: none."""
    mean, var = posterior_all(case)
    return _ei_ref.alpha(mean[:G], var[:G], incumbent(case, which), XI,
                         _ei_ref.EI if kind == 'ei' else _ei_ref.PI,
                         None if fmin is None else np.asarray(fmin, dtype=float)[:G])
