"""Cases and the NumPy reference of the Thompson-swarm fitness (tests/test_gpu_swarm_thompson.py,
tests/test_swarm_thompson_host.py): the path term from tests/_paths_numpy.py, the posterior
stated with its kernel matrices, the penalty from ``SafeOptSwarm._compute_penalty``.

A case is ``(kind, d, n, m, P)``.  The values of every axis are the smallest at which the code
takes another path: n = 5 / 60 / 300 (one per posterior kernel family, below and above 48 and
256 observations), m = 3 / 130 (not a multiple of 4 or 16; more than one LDS stage of the grid
kernel), P = 1 / 37 / 5000 (a partial workgroup; below and above kSmallPoints = 4096).  The 37
particles are the rows 100..136 of the 5000, the single one is row 100.
"""
import functools

import numpy as np

import _paths_numpy as pn
from _gpu_common import smooth

NOISE = 0.05 ** 2
BETA = 2.0
SCALING = np.array([1.3, 0.9])
BAND_EDGES = (0.0, -0.001, -0.1, -1.0)
EDGE_GAP = 1e-9

CASES = [("RBF", 1, 5, 3, 1), ("Matern52", 3, 60, 130, 37), ("product", 3, 300, 3, 5000),
         ("RBF", 3, 300, 130, 37), ("Matern52", 1, 5, 130, 5000), ("product", 1, 60, 3, 1),
         ("RBF", 1, 60, 130, 5000), ("Matern52", 3, 300, 3, 1), ("product", 3, 5, 130, 37)]
IDS = ["%s-d%d-n%d-m%d-P%d" % c for c in CASES]
for _ax, _vals in ((0, ["Matern52", "RBF", "product"]), (1, [1, 3]), (2, [5, 60, 300]),
                   (3, [3, 130]), (4, [1, 37, 5000])):
    assert sorted(set(c[_ax] for c in CASES)) == _vals
#: the cases of the penalty test: those with more than one particle (a single particle sits
#: on its own median: slack 0, a band edge)
PENALTY_CASES = [c for c in CASES if c[4] > 1]
PENALTY_IDS = [i for c, i in zip(CASES, IDS) if c[4] > 1]


def make_kernel(ns, kind, d):
    """The objective's kernel; "product": two parts (Matern-5/2 x RBF), overlapping for d = 1."""
    if kind == "product":
        a, b = ([0], [0]) if d == 1 else ([0, 1], [1, 2])
        return (ns.Matern52(len(a), variance=1.3, lengthscale=np.linspace(0.9, 1.7, len(a)),
                            ARD=True, active_dims=a, name="pa") *
                ns.RBF(len(b), variance=0.9, lengthscale=np.linspace(0.7, 1.4, len(b)), ARD=True,
                       active_dims=b, name="pb"))
    ls = np.linspace(0.5, 2.5, d) if kind == "Matern52" else np.linspace(0.8, 1.6, d)
    return getattr(ns, kind)(d, variance=1.7, lengthscale=ls, ARD=True)


def constraint_kernel(ns, d):
    return ns.RBF(d, variance=0.8, lengthscale=np.linspace(1.0, 1.5, d), ARD=True)


def kern_tuple(k, d):
    desc = k._desc(d)
    return ([int(x) for x in desc[1]], [float(v) for v in desc[2]], np.array(desc[3], dtype=float))


@functools.lru_cache(maxsize=None)
def problem(kind, d, n, m, P):
    """Data, the random numbers of ONE path and the particles of a case; computed once, never
    modified.  ``(kern0, kern1, X, Y (n, 2), particles, Omega, phase, W (m, 1), E (n, 1))``."""
    from safeopt_amd import paths as paths_mod
    import safeopt_amd.gpy as gpy
    rng = np.random.RandomState(1000 * n + 10 * m + d)
    X = rng.uniform(-2.5, 2.5, (n, d))
    Y = np.hstack([smooth(X, n), smooth(X, n + 7)]) + 0.05 * rng.standard_normal((n, 2))
    big = np.random.RandomState(77 + d).uniform(-3, 3, (5000, d))
    particles = {1: big[100:101], 37: big[100:137], 5000: big}[P].copy()
    kern0 = kern_tuple(make_kernel(gpy.kern, kind, d), d)
    kern1 = kern_tuple(constraint_kernel(gpy.kern, d), d)
    Om, b, W, E = paths_mod.draw_path_inputs((kern0[0], kern0[2]), NOISE, n, d, 1, m, rng=rng)
    for a in (X, Y, particles, Om, b, W, E, kern0[2], kern1[2]):
        a.setflags(write=False)
    return kern0, kern1, X, Y, particles, Om, b, W, E


def posterior(kern, X, y, Xnew):
    """mean, var (GPy's clip at 1e-15) of the noiseless posterior at the rows of Xnew."""
    Ky = pn.gram(kern, NOISE, X)
    Kx = pn.kernel_matrix(kern, Xnew, X)
    sol = np.linalg.solve(Ky, np.column_stack([np.asarray(y, dtype=float).reshape(-1), Kx.T]))
    mean = Kx.dot(sol[:, 0])
    var = pn.prior_variance(kern) - np.einsum("ij,ji->i", Kx, sol[:, 1:])
    return mean, np.clip(var, 1e-15, np.inf)


@functools.lru_cache(maxsize=None)
def lower_bounds(case):
    """(2, P) lower confidence bounds of the two GPs at the particles, in NumPy."""
    kern0, kern1, X, Y, particles = problem(*case)[:5]
    out = []
    for g, kern in enumerate((kern0, kern1)):
        mean, var = posterior(kern, X, Y[:, g], particles)
        out.append(mean - BETA * np.sqrt(var))
    out = np.array(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fmin_of(case):
    """Constraints that split the particles and keep every scaled slack above -0.9: per GP the
    midpoint of the two middle NumPy lower bounds (no particle sits ON the constraint), but at
    most 0.9 scaling above their minimum."""
    low = np.sort(lower_bounds(case), axis=1)
    k = low.shape[1] // 2
    return tuple(float(min(0.5 * (low[g, k - 1] + low[g, k]), low[g, 0] + 0.9 * SCALING[g]))
                 for g in range(2))


def near_band_edge(scaled_slack):
    """Particles (columns of the (G, P) scaled slacks) within EDGE_GAP of an edge of a band of
    the penalty: there the reference and the device may land on different sides."""
    s = np.atleast_2d(scaled_slack)
    near = np.zeros(s.shape[1], dtype=bool)
    for edge in BAND_EDGES:
        near |= np.any(np.abs(s - edge) <= EDGE_GAP, axis=0)
    return near
