"""Cases and the NumPy reference of the hallucinated swarm fitness (tests/test_swarm_batch_cpu.py,
tests/test_gpu_swarm_batch.py).  Data, kernels, ``posterior``, ``fmin_of`` and
``near_band_edge`` are those of tests/_swarm_thompson_ref.py.

A case is ``(kind, d, n, b, P, G)``.  The values of every axis are the smallest at which the code
takes another path: n = 5 / 60 / 300 (one per posterior kernel family; with the pending picks
more than one staged chunk of 128 training points of the downdate kernel), b = 1 / 5 / 63 (one
pass of 16 tail rows, a partial one, four with a partial last one), P = 1 / 37 / 5000 (a partial
workgroup; below and above kSmallPoints = 4096), d = 1 / 3, the three kernels, G = 2 and one
case with G = 3 whose GPs 1 and 2 share inputs and kernel (one factor).  The 37 particles are
the rows 100..136 of the 5000, the single one is row 100.

Pending picks of a case (``pending``): the first equals a particle (row 100 of the 5000), the others lie near rows
100..136 of the 5000 (offsets of 0.05), the one before last repeats the first (the noise 0.05^2 keeps the
pivot positive), the last lies 1000 units -- 400 of the longest lengthscale -- from everything.
b = 1 keeps the first only.  ``var_h`` is stated the slow way: the posterior refitted on the
data plus the pending picks.
"""
import functools

import numpy as np

import _paths_numpy as pn
import _swarm_thompson_ref as tref
from _gpu_common import smooth

NOISE, BETA, EDGE_GAP = tref.NOISE, tref.BETA, tref.EDGE_GAP
near_band_edge = tref.near_band_edge
SCALING = np.array([1.3, 0.9, 1.1])
FAR = 1000.0
FEATURES = 3          # the `m` of the Thompson cases whose data these cases reuse

CASES = [("RBF", 1, 5, 1, 1, 2), ("Matern52", 3, 60, 5, 37, 2), ("product", 3, 300, 63, 5000, 2),
         ("RBF", 3, 300, 5, 37, 3), ("Matern52", 1, 5, 63, 5000, 2), ("product", 1, 60, 1, 1, 2),
         ("RBF", 1, 60, 63, 5000, 2), ("Matern52", 3, 300, 1, 1, 2), ("product", 3, 5, 5, 37, 2)]
IDS = ["%s-d%d-n%d-b%d-P%d-G%d" % c for c in CASES]
for _ax, _vals in ((0, ["Matern52", "RBF", "product"]), (1, [1, 3]), (2, [5, 60, 300]),
                   (3, [1, 5, 63]), (4, [1, 37, 5000]), (5, [2, 3])):
    assert sorted(set(c[_ax] for c in CASES)) == _vals
#: the cases of the whole-formula test: those with more than one particle (a single particle
#: sits on its own median: slack 0, a band edge)
FORMULA_CASES = [c for c in CASES if c[4] > 1]
FORMULA_IDS = [i for c, i in zip(CASES, IDS) if c[4] > 1]


def tcase(case):
    """The Thompson case whose data, kernels and particles this case uses."""
    kind, d, n, b, P, G = case
    return (kind, d, n, FEATURES, P)


@functools.lru_cache(maxsize=None)
def problem(case):
    """``(kerns (G tuples), X, Y (n, G), particles)``; computed once, never modified.  GP 2 of a
    G = 3 case has the inputs and the kernel of GP 1 and observations of its own."""
    kind, d, n, b, P, G = case
    kern0, kern1, X, Y, particles = tref.problem(*tcase(case))[:5]
    kerns = (kern0, kern1)
    if G == 3:
        rng = np.random.RandomState(5 * n + d)
        Y = np.hstack([Y, smooth(X, n + 13) + 0.05 * rng.standard_normal((n, 1))])
        Y.setflags(write=False)
        kerns = (kern0, kern1, kern1)
    return kerns, X, Y, particles


@functools.lru_cache(maxsize=None)
def pending(case, far_only=False):
    """The (b, d) pending picks of a case; ``far_only``: the far one alone (b = 1)."""
    kind, d, n, b, P, G = case
    far = np.full((1, d), FAR)
    big = np.random.RandomState(77 + d).uniform(-3, 3, (5000, d))
    first = big[100:101]
    if far_only:
        out = far
    elif b == 1:
        out = first.copy()
    else:
        rng = np.random.RandomState(31 * b + d)
        rows = 100 + rng.randint(0, 37, size=b - 3)
        near = big[rows] + 0.05 * rng.standard_normal((b - 3, d))
        out = np.vstack([first, near, first, far])
        assert out.shape == (b, d)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def real_posterior(case, dtype=np.float64):
    """mean, var (G, P) of the real GPs at the particles."""
    kerns, X, Y, particles = problem(case)
    mv = [posterior(kerns[g], X, Y[:, g], particles, dtype) for g in range(case[5])]
    return np.array([m for m, _ in mv]), np.array([v for _, v in mv])


def posterior(kern, X, y, Xnew, dtype=np.float64):
    """``tref.posterior`` in ``dtype`` (float64: that function itself)."""
    if dtype == np.float64:
        return tref.posterior(kern, X, y, Xnew)
    Ky = pn.gram(kern, NOISE, X, dtype)
    Kx = pn.kernel_matrix(kern, Xnew, X, dtype)
    sol = pn._cholesky_solve(Ky, np.column_stack([np.asarray(y, dtype=dtype).reshape(-1), Kx.T]),
                             dtype)
    mean = Kx.dot(sol[:, 0])
    var = dtype(pn.prior_variance(kern)) - np.einsum("ij,ji->i", Kx, sol[:, 1:])
    return mean, np.clip(var, dtype(1e-15), np.inf)


def refit_var_h(case, pend, dtype=np.float64, particles=None):
    """(G, P) hallucinated variances the slow way: every GP refitted on its inputs plus the
    pending picks (any observations: the variance does not read them)."""
    kerns, X, Y, pts = problem(case)
    pts = pts if particles is None else particles
    Xp = np.vstack([X, pend])
    y = np.zeros(Xp.shape[0])
    return np.array([posterior(kerns[g], Xp, y, pts, dtype)[1] for g in range(case[5])])


def tail_row_var_h(case, pend):
    """``(var, down, var_h)``, each (G, P), by the identity of DESIGN.md 4.13 in float64: with
    L' the Cholesky factor of the bordered Ky', t_j = (row n + j of L'^-1) . k(X', x), down =
    sum_j t_j^2 in the order j = 0 .. b-1, var_h = max(var - down, 1e-15)."""
    from scipy.linalg import solve_triangular
    kerns, X, Y, particles = problem(case)
    n, b = X.shape[0], pend.shape[0]
    Xp = np.vstack([X, pend])
    out = []
    for g in range(case[5]):
        L = np.linalg.cholesky(pn.gram(kerns[g], NOISE, Xp))
        T = solve_triangular(L, pn.kernel_matrix(kerns[g], Xp, particles), lower=True)  # (n+b, P)
        var = np.clip(pn.prior_variance(kerns[g]) - (T[:n] ** 2).sum(0), 1e-15, np.inf)
        down = np.zeros(particles.shape[0])
        for j in range(b):
            down = down + T[n + j] ** 2
        out.append((var, down, np.maximum(var - down, 1e-15)))
    return tuple(np.array([o[i] for o in out]) for i in range(3))


def penalty(scaled_slack):
    from safeopt_amd.gp_opt import SafeOptSwarm
    return SafeOptSwarm._compute_penalty(None, scaled_slack)


def hall_fitness(swarm_type, mean, var, var_h, fmin, scaling, best_lower_bound, beta=BETA):
    """The fitness of DESIGN.md 4.13 restated: ``(values, safe, scaled slacks (G, P), parts)``
    from the real ``mean`` / ``var`` and the hallucinated ``var_h``, all (G, P); ``parts =
    (width, total_pen, interest)``."""
    from scipy.special import expit
    from scipy.stats import norm
    assert swarm_type in ("maximizers", "expanders")
    G, P = mean.shape
    fmin = np.asarray(fmin, dtype=float)
    sd = np.sqrt(var)
    lower, upper = mean - beta * sd, mean + beta * sd
    width = np.max(np.sqrt(var_h) / scaling[:G, None], axis=0)
    if swarm_type == "maximizers":
        interest = expit(10 * (upper[0] - best_lower_bound) / scaling[0])
    else:
        interest = np.full(P, float(G))
    total_pen = np.zeros(P)
    safe = np.ones(P, dtype=bool)
    scaled = np.full((G, P), np.inf)
    for g in range(G):
        if fmin[g] == -np.inf:
            continue
        slack = lower[g] - fmin[g]
        safe &= slack >= 0
        scaled[g] = slack / scaling[g]
        total_pen += penalty(scaled[g])
        if swarm_type == "expanders":
            interest = interest * norm.pdf(scaled[g], scale=0.2)
    return (width + total_pen) * interest, safe, scaled, (width, total_pen, interest)


def fmin_of(case):
    """``tref.fmin_of`` for the first two GPs; GP 2 of a G = 3 case: the median of its own
    NumPy lower bounds, capped the same way."""
    f = list(tref.fmin_of(tcase(case)))
    if case[5] == 3:
        mean, var = real_posterior(case)
        low = np.sort(mean[2] - BETA * np.sqrt(var[2]))
        k = low.shape[0] // 2
        f.append(float(min(0.5 * (low[k - 1] + low[k]), low[0] + 0.9 * SCALING[2])))
    return np.array(f)


def best_lower_bound_of(case):
    """The maximizers' ``best_lower_bound``: the median lower bound of GP 0 (half the interests
    above 1/2, half below)."""
    return float(np.median(tref.lower_bounds(tcase(case))[0]))


def batch_choice_reference(sd_maxi, sd_exp, scaling, fmin, threshold, ucb):
    """Step 3 of ``SafeOptSwarm.optimize_batch`` restated with plain loops."""
    if ucb:
        return None if sd_maxi is None else "maximizers"
    if sd_maxi is None or sd_exp is None:
        return None if sd_maxi is None and sd_exp is None else \
            ("maximizers" if sd_exp is None else "expanders")
    v_exp = 0.0
    for g in range(len(scaling)):
        if fmin[g] != -np.inf and sd_exp[g] >= threshold:
            v_exp = max(v_exp, sd_exp[g] / scaling[g])
    return "maximizers" if sd_maxi[0] / scaling[0] > v_exp else "expanders"
