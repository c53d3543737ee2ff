"""The swarm fitness in ``np.longdouble`` and the case table of the band-by-band tests
(tests/test_swarm_fitness_ref_cpu.py, tests/test_gpu_swarm_fitness.py).

Posterior: ``RefGP`` of tests/_incremental_ref.py (kernels from differences, column Cholesky,
substitutions; nothing of ``oracle/``).  On top of it ``shape`` restates
``SafeOptSwarm._compute_penalty`` (gp_opt.py:874-899) and ``_compute_particle_fitness``
(gp_opt.py:925-1013) in long double and also returns what the tests sort the particles by: the
scaled slack of every active GP, its band, and the parts of ``(values + total_pen) * interest``.

Bands of a scaled slack s (``band``):

    0   s >= 0                 no penalty
    1   -0.001 <  s <  0       2 s
    2   -0.1   <  s <= -0.001  5 s
    3   -1     <  s <= -0.1    10 s
    4   s < -1                 -300 s^2      (designed particles: -3 <= s, slope <= 1800)
    5   s == -1                s             (neither ``> -1`` nor ``< -1``: no factor)

A case is ``(kind, d, n per GP, fmin pattern, route)``: ``fmin pattern`` holds one flag per GP
(0: ``fmin = -inf``, an inactive GP), ``route`` names the posterior route of a fitness call on
the case's particles -- 'tiny' (n = 10: the VALU sweep for up to 48 observations, which takes
every launch of GPs with up to 10), 'classic' (n = 20: below 1536 n particles the 4-wave
matrix-core sweep), 'few' (n = 130, P <= 4096: the few-points path), 'sweep' (n = 130 and 4097
particles: the 4-wave sweep again).

Particles: 257 random ones, uniform in [-3, 3]^d, then for every active GP and every band 0 .. 4
eight designed ones whose scaled slack of that GP lies at a chosen place inside the band
(``TARGETS``), found by bisecting the reference lower bound along a segment between two random
particles; a 'sweep' case is filled up with random particles to 4097.  ``fmin`` and ``scaling``
of GP g come from the 5 % and 90 % quantiles of its reference lower bound over the 257 random
particles, which land on the scaled slacks -3 and +0.5.
"""
import functools

import numpy as np

import _incremental_ref as R
from _gpu_common import MEAN_TOL, VAR_TOL, smooth

LD = R.LD
BETA = 2.0
N_RANDOM = 257
N_SWEEP = 4097
EDGES = (0.0, -0.001, -0.1, -1.0)
PER_BAND = 8

#: where the designed particles sit, per band
TARGETS = {0: np.linspace(0.05, 0.45, PER_BAND),
           1: -0.001 * np.linspace(0.15, 0.85, PER_BAND),
           2: -np.geomspace(0.002, 0.08, PER_BAND),
           3: -np.linspace(0.15, 0.9, PER_BAND),
           4: -np.linspace(1.1, 2.9, PER_BAND)}

PROD4 = (("RBF", (0, 1), R.VARIANCE, (1.2, 1.6)), ("Matern52", (2, 3), 1.0, (1.6, 1.2)))


def spec_of(kind, d):
    return PROD4 if kind == "prod" else R.single(kind, d)


CASES = {
    "rbf_d2_g1_n20": ("RBF", 2, 20, (1,), "classic"),
    "rbf_d2_g2_n130": ("RBF", 2, 130, (1, 1), "few"),
    "mat52_d3_g2_n20": ("Matern52", 3, 20, (1, 1), "classic"),
    "mat52_d3_g3_n130": ("Matern52", 3, 130, (1, 0, 1), "few"),
    "prod_d4_g3_n20": ("prod", 4, 20, (1, 1, 0), "classic"),
    "prod_d4_g1_n130": ("prod", 4, 130, (1,), "few"),
    "rbf_d2_g3_n130_sweep": ("RBF", 2, 130, (1, 1, 0), "sweep"),
    "tiny_rbf_d2_g2_n10": ("RBF", 2, 10, (1, 1), "tiny"),
}
#: what ``Context.last_sweep()`` names after a fitness call on the case's particles
SWEEP_OF = {"tiny": "tiny", "classic": "classic", "sweep": "classic"}
NAMES = sorted(CASES)


# ---------------------------------------------------------------------------------------
# the shaping, gp_opt.py:874-899 and 925-1013
# ---------------------------------------------------------------------------------------
def band(s):
    """Band index of every scaled slack (any float type)."""
    s = np.asarray(s)
    return np.select([s >= 0, s > -0.001, s > -0.1, s > -1, s == -1], [0, 1, 2, 3, 5], default=4)


def penalty(s):
    """``_compute_penalty`` on an array of any float type, statement for statement."""
    s = np.atleast_1d(np.asarray(s))
    pen = np.minimum(s, s.dtype.type(0))
    pen[(s < 0) & (s > -0.001)] *= 2
    pen[(s <= -0.001) & (s > -0.1)] *= 5
    pen[(s <= -0.1) & (s > -1)] *= 10
    far = s < -1
    pen[far] = -300 * pen[far] ** 2
    return pen


def norm_pdf(s, scale):
    """scipy.stats.norm.pdf(s, scale=scale) in the type of ``s``."""
    z = s / s.dtype.type(scale)
    return np.exp(-z * z / 2) / np.sqrt(2 * np.pi * np.ones((), dtype=s.dtype)) / s.dtype.type(scale)


def expit(z):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-z))


def shape(kind, mean, var, fmin, scaling, best_lower_bound, beta=BETA, var_w=None):
    """Fitness of P particles from the posterior ``mean`` / ``var`` (G, P) in long double.

    ``kind``: 'greedy' | 'maximizers' | 'expanders' | 'safe_set', or 'penalty' -- the branch the
    thompson, mes and ise swarms share: ``values = total_pen``, the maximizers' safety flag.
    ``var_w`` (G, P): the variance the width term is formed from (a hallucinated swarm's).
    Returns a dict: ``values``, ``safe``, ``slack`` (G, P; NaN for an inactive GP), ``band`` (G,
    P; -1 for an inactive GP), ``width``, ``total_pen``, ``interest``, ``lower`` (G, P)."""
    mean = np.asarray(mean, dtype=LD)
    var = np.asarray(var, dtype=LD)
    G, P = mean.shape
    fmin = np.asarray(fmin, dtype=float)
    scaling = np.asarray(scaling, dtype=LD)
    sd = np.sqrt(var)
    sd_w = sd if var_w is None else np.sqrt(np.asarray(var_w, dtype=LD))
    lower_all = mean - LD(beta) * sd
    out = dict(lower=lower_all, slack=np.full((G, P), np.nan, dtype=LD),
               band=np.full((G, P), -1, dtype=int))
    if kind == "greedy":
        out.update(values=lower_all[0], safe=np.ones(P, dtype=bool))
        return out
    upper = mean[0] + LD(beta) * sd[0]
    width = sd_w[0] / scaling[0]
    if kind == "expanders":
        interest = LD(G) * np.ones(P, dtype=LD)
    elif kind == "maximizers":
        out["z"] = LD(10) * (upper - LD(best_lower_bound)) / scaling[0]
        interest = expit(out["z"])
    else:
        interest = np.ones(P, dtype=LD)
    safe = np.ones(P, dtype=bool)
    total_pen = np.zeros(P, dtype=LD)
    lower = lower_all[0]
    for g in range(G):
        if g > 0:
            lower = lower_all[g]
            width = np.maximum(width, sd_w[g] / scaling[g])
        if fmin[g] == -np.inf:
            continue
        slack = lower - LD(fmin[g])
        safe &= slack >= 0
        slack = slack / scaling[g]
        out["slack"][g] = slack
        out["band"][g] = band(slack)
        if kind == "safe_set":
            continue
        total_pen += penalty(slack)
        if kind == "expanders":
            interest = interest * norm_pdf(slack, 0.2)
    out.update(width=width, total_pen=total_pen, interest=interest, safe=safe)
    if kind == "safe_set":
        out["values"] = lower
    elif kind == "penalty":
        out["values"] = total_pen
    else:
        out["values"] = (width + total_pen) * interest
    return out


# ---------------------------------------------------------------------------------------
# the margin of the comparison with a device
# ---------------------------------------------------------------------------------------
def sd_bound(var, kdiag, factor=1):
    """|d sd| of a variance held to ``factor * VAR_TOL * k(x, x)``: min(sqrt(dv), dv / sd)."""
    dv = factor * VAR_TOL * kdiag
    sd = np.sqrt(np.asarray(var, dtype=float))
    return np.minimum(np.sqrt(dv), dv / sd)


def slack_margin(mean, var, kdiags, scaling, beta=BETA):
    """D (G, P): what a posterior within MEAN_TOL / VAR_TOL of the truth can move the scaled
    slack of GP g by (and its scaled upper bound): (MEAN_TOL max|mean_g| + beta min(sqrt(dv),
    dv / sd)) / scaling_g, dv = VAR_TOL k(x, x)."""
    mean = np.asarray(mean, dtype=float)
    D = np.empty(mean.shape)
    for g in range(mean.shape[0]):
        D[g] = (MEAN_TOL * np.abs(mean[g]).max() + beta * sd_bound(var[g], kdiags[g])) / float(
            scaling[g])
    return D


def edge_distance(slack):
    """Distance of every scaled slack to the closest band edge (NaN stays NaN)."""
    s = np.asarray(slack, dtype=float)
    return np.min([np.abs(s - e) for e in EDGES], axis=0)


def left_out(slack, D):
    """Particles with an active GP's scaled slack within its margin of a band edge."""
    with np.errstate(invalid="ignore"):
        return np.any(edge_distance(slack) <= D, axis=0)         # (NaN <= D is False)


def near_zero(slack, D):
    with np.errstate(invalid="ignore"):
        return np.any(np.abs(np.asarray(slack, dtype=float)) <= D, axis=0)


EPS = 2.0 ** -53
SLOPE = np.array([0.0, 2.0, 5.0, 10.0, 0.0, 1.0])        # band -> slope (band 4: 600 |s|)


def penalty_tol(slack, bands, D):
    """|d total_pen| <= sum_g slope_g D_g for slacks that keep their band: slope 2, 5, 10 in the
    linear bands, 600 (|s| + D) in the quadratic one, nothing for an inactive GP."""
    s = np.abs(np.nan_to_num(np.asarray(slack, dtype=float)))
    slope = np.where(bands == 4, 600.0 * (s + D), SLOPE[np.maximum(bands, 0)])
    return np.sum(np.where(bands >= 0, slope * D, 0.0), axis=0)


def value_tol(kind, ref, mean, var, kdiags, scaling, beta=BETA, var_w=None):
    """What ``values`` of ``kind`` may differ by from the long-double ``ref`` = shape(kind, ...)
    when the posterior behind it meets MEAN_TOL / VAR_TOL and no slack changes its band.  The
    derivation: docstring of tests/test_gpu_swarm_fitness.py.  ``var_w``: a hallucinated swarm,
    whose width variance (real variance minus downdate) is held to 2 VAR_TOL k(x, x)."""
    G = len(kdiags)
    scaling = np.asarray(scaling, dtype=float)
    D = slack_margin(mean, var, kdiags, scaling, beta)
    val = np.abs(np.asarray(ref["values"], dtype=float))
    if kind == "greedy":
        return D[0] * scaling[0] + 4 * EPS * val
    if kind == "safe_set":
        return D[G - 1] * scaling[G - 1] + 4 * EPS * val
    d_pen = penalty_tol(ref["slack"], ref["band"], D)
    pen = np.abs(np.asarray(ref["total_pen"], dtype=float))
    if kind == "penalty":
        return d_pen + 8 * EPS * pen
    wv, factor = (var, 1) if var_w is None else (var_w, 2)
    d_width = np.max([sd_bound(wv[g], kdiags[g], factor) / scaling[g] for g in range(G)], axis=0)
    width = np.asarray(ref["width"], dtype=float)
    I = np.asarray(ref["interest"], dtype=float)
    if kind == "maximizers":
        dz = 10.0 * D[0]
        d_I = I * (1.0 - I) * dz * np.exp(dz)
        arg = np.abs(np.asarray(ref["z"], dtype=float))
    else:
        s = np.abs(np.nan_to_num(np.asarray(ref["slack"], dtype=float)))
        act = ref["band"] >= 0
        d_I = I * np.expm1(np.sum(np.where(act, s * D / 0.04 + D * D / 0.08, 0.0), axis=0))
        arg = np.sum(np.where(act, 0.5 * (s / 0.2) ** 2, 0.0), axis=0)
    rounding = 8 * EPS * (width + pen) * I * (1.0 + arg)
    both = np.abs(np.asarray(ref["width"] + ref["total_pen"], dtype=float))
    return (d_width + d_pen) * (I + d_I) + both * d_I + rounding + 1e-300


# ---------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------
def _seed(name):
    return 1000 + 17 * NAMES.index(name)


def _lower(gp, pts):
    m, v = gp.predict(pts)
    return m - LD(BETA) * np.sqrt(v)


def _design(gp, fmin, scaling, rand, rand_lower, rng):
    """Eight particles per band whose scaled slack of ``gp`` sits at TARGETS: bisection of the
    reference lower bound on segments between random particles."""
    targets = np.concatenate([TARGETS[b] for b in range(5)])
    want = LD(fmin) + np.asarray(targets, dtype=LD) * LD(scaling)
    A = np.empty((targets.size, rand.shape[1]))
    B = np.empty_like(A)
    for i, w in enumerate(want):
        below, above = np.flatnonzero(rand_lower < w), np.flatnonzero(rand_lower > w)
        assert below.size and above.size, "no random particle on one side of slack %g" % targets[i]
        A[i], B[i] = rand[rng.choice(below)], rand[rng.choice(above)]
    for _ in range(56):
        M = 0.5 * (A + B)
        low = np.asarray(_lower(gp, M) < want)
        A[low], B[~low] = M[low], M[~low]
    return 0.5 * (A + B)


@functools.lru_cache(maxsize=None)
def problem(name):
    """Everything of a case: ``specs``, ``X``, ``Y`` (per GP), ``gps`` (RefGP), ``particles``
    (float64), ``fmin``, ``scaling``, ``best_lower_bound``, the reference posterior ``mean`` /
    ``var`` (G, P, long double), ``kdiag`` (G) and ``designed`` = (GP, band, first row) of
    every group of eight designed particles."""
    kind, d, n, pattern, route = CASES[name]
    rng = np.random.default_rng(_seed(name))
    G = len(pattern)
    spec = spec_of(kind, d)
    X = [rng.uniform(-2, 2, size=(n, d)) for _ in range(G)]
    Y = [smooth(X[g], _seed(name) + g)[:, 0] + 0.3 for g in range(G)]
    gps = [R.RefGP(spec, X[g], Y[g]) for g in range(G)]
    rand = rng.uniform(-3, 3, size=(N_RANDOM, d))
    fmin, scaling, parts, designed = np.empty(G), np.empty(G), [rand], []
    row = N_RANDOM
    for g in range(G):
        lo = _lower(gps[g], rand)
        q5, q90 = np.quantile(np.asarray(lo, dtype=float), [0.05, 0.9])
        scaling[g] = (q90 - q5) / 3.5
        fmin[g] = q90 - 0.5 * scaling[g]
        if pattern[g]:
            parts.append(_design(gps[g], fmin[g], scaling[g], rand, lo, rng))
            designed += [(g, b, row + PER_BAND * b) for b in range(5)]
            row += 5 * PER_BAND
        else:
            fmin[g] = -np.inf
    if route == "sweep":
        parts.append(rng.uniform(-3, 3, size=(N_SWEEP - row, d)))
    particles = np.ascontiguousarray(np.vstack(parts))
    post = [gp.predict(particles) for gp in gps]
    mean = np.array([m for m, _ in post], dtype=LD)
    var = np.array([v for _, v in post], dtype=LD)
    lo0 = np.asarray(mean[0] - LD(BETA) * np.sqrt(var[0]), dtype=float)[:N_RANDOM]
    return dict(name=name, kind=kind, d=d, n=n, G=G, route=route, specs=[spec] * G, X=X, Y=Y,
                gps=gps, particles=particles, fmin=fmin, scaling=scaling,
                best_lower_bound=float(np.median(lo0)), mean=mean, var=var,
                kdiag=[R.kdiag(spec)] * G, designed=designed)


def reference(name, kind, var_w=None):
    p = problem(name)
    return shape(kind, p["mean"], p["var"], p["fmin"], p["scaling"], p["best_lower_bound"],
                 var_w=var_w)


def tolerance(name, kind, ref=None, var_w=None):
    p = problem(name)
    ref = reference(name, kind, var_w) if ref is None else ref
    return value_tol(kind, ref, p["mean"], p["var"], p["kdiag"], p["scaling"], var_w=var_w)


def margin(name):
    p = problem(name)
    return slack_margin(p["mean"], p["var"], p["kdiag"], p["scaling"])


def pending(name):
    """The one pending pick of the case's hallucinated swarm: inside the data box."""
    p = problem(name)
    return np.random.default_rng(_seed(name) + 5).uniform(-1.5, 1.5, size=p["d"])


@functools.lru_cache(maxsize=None)
def hall_variance(name):
    """(G, P) long double: the variance with ``pending(name)`` appended to every GP."""
    p = problem(name)
    x = pending(name)
    out = []
    for g in range(p["G"]):
        gp = R.RefGP(p["specs"][g], p["X"][g], p["Y"][g])
        gp.append(x, 0.0)
        out.append(np.maximum(gp.predict(p["particles"])[1], LD(1e-15)))
    return np.array(out, dtype=LD)
