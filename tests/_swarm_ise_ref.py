"""Cases and the long-double reference of the information-theoretic safe exploration swarm
(tests/test_swarm_ise_cpu.py, tests/test_gpu_swarm_ise.py).

A case is ``(kind, d, n, P, T, variant)``, built on the problems of
tests/_swarm_thompson_ref.py (its data generator, kernels, noise, beta and scaling):

* n = 5 / 64 / 65 / 300: one per posterior family, and both sides of the 64-row LDS stage of
  k_swarm_ise;
* P = 1 / 37 / 64 / 65 / 5000: a partial tile, the tile edge, both sides of kSmallPoints = 4096
  (rows 100.. of the 5000 particles of the Thompson problems);
* T = 1 / 15 / 16 / 17 / 64 / 65 / 130: the 16- and 64-column block edges;
* d = 1 / 3; RBF, Matern-5/2 and a product kernel;
* variant ``'mid'``: three GPs with ``fmin = [0.2, -inf, -0.3]``, an inactive GP in the middle;
  ``'twin'``: two GPs with the same inputs, kernel and noise (``GpDev::share``); ``''``: the
  objective and the constraint GP of the Thompson problems.

Target ``t`` is particle ``t mod P`` plus 0.4 standard normal per coordinate: every target is
correlated with a particle, so the covariances are not all negligible.  Except in the
``'mid'`` case ``fmin_g`` of the "open" tests is the smallest reference lower bound of the
particles minus 0.05: finite -- the GP is active -- with every particle safe and no penalty.

The reference is the long-double GP of tests/_incremental_ref.py with ``_ise_ref.ref_cov`` and
``_ise_ref.term``.
"""
import functools

import numpy as np

import _incremental_ref as inc
import _ise_ref
import _swarm_thompson_ref as tref
from _gpu_common import smooth
from _swarm_thompson_ref import BETA, NOISE, near_band_edge  # noqa: F401

SCALING = np.array([1.3, 0.9, 1.1])
FMIN_MID = (0.2, -np.inf, -0.3)
OPEN_MARGIN = 0.05

CASES = [("RBF", 1, 5, 1, 1, ""), ("Matern52", 3, 64, 37, 15, ""),
         ("product", 3, 300, 5000, 17, ""), ("RBF", 3, 65, 64, 16, ""),
         ("Matern52", 1, 5, 5000, 64, ""), ("product", 1, 64, 65, 65, ""),
         ("RBF", 1, 300, 37, 130, ""), ("Matern52", 3, 300, 1, 17, ""),
         ("product", 3, 5, 37, 64, ""), ("RBF", 3, 65, 65, 130, "mid"),
         ("Matern52", 3, 64, 64, 65, "twin"), ("RBF", 3, 300, 5000, 130, "")]
IDS = ["%s-d%d-n%d-P%d-T%d%s" % (c[:5] + (("-" + c[5]) if c[5] else "",)) for c in CASES]
for _ax, _vals in ((0, ["Matern52", "RBF", "product"]), (1, [1, 3]), (2, [5, 64, 65, 300]),
                   (3, [1, 37, 64, 65, 5000]), (4, [1, 15, 16, 17, 64, 65, 130])):
    assert sorted(set(c[_ax] for c in CASES)) == _vals
assert len(CASES) == 12
#: the cases of the penalty test: more than one particle, and a derived fmin
PENALTY_CASES = [c for c in CASES if c[3] > 1 and c[5] != "mid"]
PENALTY_IDS = [i for c, i in zip(CASES, IDS) if c[3] > 1 and c[5] != "mid"]


def spec_of(kind, d):
    """The kernel of ``tref.make_kernel`` as a spec of tests/_incremental_ref.py."""
    if kind == "product":
        a, b = ((0,), (0,)) if d == 1 else ((0, 1), (1, 2))
        return (("Matern52", a, 1.3, tuple(np.linspace(0.9, 1.7, len(a)))),
                ("RBF", b, 0.9, tuple(np.linspace(0.7, 1.4, len(b)))))
    ls = np.linspace(0.5, 2.5, d) if kind == "Matern52" else np.linspace(0.8, 1.6, d)
    return ((kind, tuple(range(d)), 1.7, tuple(ls)),)


def constraint_spec(d):
    return (("RBF", tuple(range(d)), 0.8, tuple(np.linspace(1.0, 1.5, d))),)


def third_spec(d):
    return (("Matern52", tuple(range(d)), 1.1, tuple(np.linspace(0.9, 1.3, d))),)


def specs(case):
    kind, d, variant = case[0], case[1], case[5]
    if variant == "twin":
        return (spec_of(kind, d), spec_of(kind, d))
    if variant == "mid":
        return (spec_of(kind, d), constraint_spec(d), third_spec(d))
    return (spec_of(kind, d), constraint_spec(d))


@functools.lru_cache(maxsize=None)
def problem(case):
    """``(X (n, d), Y (n, G), particles (P, d), targets (T, d))`` of a case; computed once,
    read-only."""
    kind, d, n, P, T, variant = case
    X, Y2, big = tref.problem(kind, d, n, 3, 5000)[2:5]
    Y = Y2 if variant != "mid" else np.hstack(
        [Y2, smooth(X, n + 13) + 0.05 * np.random.RandomState(n + d).standard_normal((n, 1))])
    particles = big.copy() if P == 5000 else big[100:100 + P].copy()
    rng = np.random.RandomState(31 * T + 7 * P + d)
    targets = particles[np.arange(T) % P] + 0.4 * rng.standard_normal((T, d))
    for a in (Y, particles, targets):
        a.setflags(write=False)
    return X, Y, particles, targets


@functools.lru_cache(maxsize=None)
def ref_gps(case):
    X, Y = problem(case)[:2]
    return tuple(inc.RefGP(spec, X, Y[:, g], noise=NOISE) for g, spec in enumerate(specs(case)))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The long-double posterior at particles and targets and their covariances, as float64:
    ``dict(mean, var (G, P), zmean, zvar (G, T), cov (G, P, T), kdiag (G,))``; the variances
    clipped at 1e-15.  Computed once, read-only."""
    _, _, particles, targets = problem(case)
    out = dict(mean=[], var=[], zmean=[], zvar=[], cov=[], kdiag=[])
    for gp in ref_gps(case):
        m, v = gp.predict(particles)
        zm, zv = gp.predict(targets)
        out["mean"].append(inc.f64(m))
        out["var"].append(inc.clip_var(v))
        out["zmean"].append(inc.f64(zm))
        out["zvar"].append(inc.clip_var(zv))
        out["cov"].append(inc.f64(_ise_ref.ref_cov(gp, particles, targets)))
        out["kdiag"].append(inc.kdiag(gp.spec))
    out = {k: np.array(v) for k, v in out.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


def lower_bounds(case):
    r = reference(case)
    return r["mean"] - BETA * np.sqrt(r["var"])


def fmin_open(case):
    """fmin of the "open" tests: every GP active, every particle safe, no penalty (``'mid'``:
    the case's own fmin)."""
    if case[5] == "mid":
        return np.array(FMIN_MID)
    return lower_bounds(case).min(axis=1) - OPEN_MARGIN


def fmin_split(case):
    """Constraints that split the particles and keep every scaled slack above -0.9
    (``tref.fmin_of``'s rule on the reference lower bounds)."""
    low = np.sort(lower_bounds(case), axis=1)
    k = low.shape[1] // 2
    return np.array([min(0.5 * (low[g, k - 1] + low[g, k]), low[g, 0] + 0.9 * SCALING[g])
                     for g in range(low.shape[0])])


def pairs(case, fmin):
    """``(pairs (P, T), alpha (P,), target (P,))`` of the reference: the in-order sum over the
    active GPs of ``_ise_ref.term``, its row maximum and the first column attaining it."""
    r = reference(case)
    s = NOISE + 1e-8
    out = np.zeros(r["cov"].shape[1:])
    for g in range(len(fmin)):
        if np.isfinite(fmin[g]):
            out = out + _ise_ref.term((r["zmean"][g] - fmin[g])[None, :], r["zvar"][g][None, :],
                                      r["var"][g][:, None], r["cov"][g], s)
    return out, out.max(axis=1), out.argmax(axis=1)


def host_pairs(ise_eval, post, cov, zmean, zvar, fmin, s):
    """The sum, in the order of g, of ``ise_eval(mu, vz, vx, c, s_g)`` over the active GPs on
    the outputs of ONE fitness call: ``post (G, 2, P)``, ``cov (G, P, T)``."""
    G, P, T = cov.shape
    out = np.zeros((P, T))
    for g in range(G):
        if not np.isfinite(fmin[g]):
            continue
        mu = np.broadcast_to((zmean[g] - fmin[g])[None, :], (P, T))
        vz = np.broadcast_to(zvar[g][None, :], (P, T))
        vx = np.broadcast_to(post[g, 1][:, None], (P, T))
        out = out + ise_eval(mu.ravel(), vz.ravel(), vx.ravel(), cov[g].ravel(),
                             s[g]).reshape(P, T)
    return out
