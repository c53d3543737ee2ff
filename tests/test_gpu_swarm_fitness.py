"""The swarm fitness shaping (``shape_particle``, csrc/fitness.h) band by band against a
long-double reference (tests/_swarm_fitness_ref.py), through the C ABI (needs an MI355X).

``shape_particle`` is compiled into k_fitness_small (behind both posterior routes of a fitness
call and of a large run), k_fitness_hall (hallucinated swarms) and k_pso_small_step (a swarm of
up to 64 particles in one workgroup).  Cases, particles and bands: the reference module's
docstring; tests/test_swarm_fitness_ref_cpu.py shows without a GPU that every band of every
active GP holds at least eight compared particles.  The file also passes with ``SGP_POISON=1``
and ``=2`` in front of it.

Tolerances (``_swarm_fitness_ref.value_tol``).  No number here is measured: everything follows
from ``MEAN_TOL`` and ``VAR_TOL`` of tests/_gpu_common.py, the bounds ``check_posterior`` holds
the device posterior to, AGAINST THE TRUTH -- the reference is long double, so they enter once.

* Per GP g, dv = VAR_TOL k(x, x) and |d sd| <= min(sqrt(dv), dv / sd), so lower = mean - beta sd
  (and upper) moves by at most MEAN_TOL max|mean_g| + beta min(sqrt(dv), dv / sd_g); divided by
  scaling_g that is D_g, the margin of the scaled slack (``slack_margin``).
* A slack farther than D_g from 0 keeps its sign: ``safe`` is compared for every particle whose
  slacks all are.  A slack farther than D_g from every band edge (0, -0.001, -0.1, -1) keeps its
  band: ``values`` is compared for every particle whose slacks all are; the others, at most
  1 % of a case, are the ones the CPU test counted (``left_out``).
* 'greedy' and 'safe_set' return a lower bound: D_g scaling_g, no band involved.
* values = (W + pen) I with W = max_g sd_g / scaling_g, pen = sum_g penalty(s_g):
    |d W|   <= max_g min(sqrt(dv), dv / sd_g) / scaling_g
               (a hallucinated swarm: dv = 2 VAR_TOL k(x, x), the variance and the downdate),
    |d pen| <= sum_g slope_g D_g, slope 2, 5, 10 in the linear bands, 600 (|s_g| + D_g) in the
               quadratic one (-300 s^2), 0 for a satisfied constraint,
    maximizers, I = expit(z), z = 10 (upper_0 - best lower bound) / scaling_0, |d z| <= 10 D_0:
               expit' = I (1 - I) and |d ln expit'| <= |d z|, so |d I| <= I (1 - I) 10 D_0 e^(10 D_0),
    expanders, I = G prod_g pdf(s_g), pdf the normal density at scale 0.2:
               ln pdf(s + e) - ln pdf(s) = -(2 s e + e^2) / 0.08, so
               |d I| <= I expm1(sum_g |s_g| D_g / 0.04 + D_g^2 / 0.08),
    |d values| <= (|d W| + |d pen|) (I + |d I|) + |W + pen| |d I| + roundings,
  roundings = 8 x 2^-53 (|W| + |pen|) I (1 + |argument of exp|): sqrt, exp and the last three
  operations at an ulp or two each, and the rounding of the argument of exp, which exp turns
  into a relative error of |argument| ulps.  1e-300 absolute covers an interest that the
  device flushes to 0 where the logistic is a denormal.
* A 'mes' swarm returns alpha + total_pen; with every fmin = -inf it returns alpha.  The
  difference is held to |d pen| + 4 x 2^-53 (|v_c| + |v_u|); alpha cancels.

Exact edges.  'greedy' returns the device's own lower bound of GP 0, 'safe_set' that of the last
GP.  swarm.hip is compiled without contraction and fp64 ``-`` and ``/`` round correctly, so
NumPy computes the device's scaled slack ``(lower - fmin) / scaling`` bit for bit: the band of
EVERY particle is known, nothing is left out, and the 'mes' difference is the float64 penalty of
that slack, bit for bit -- in the order of the reference, gp_opt.py:874-899: ``-300 * pen ** 2``.
A scaling is searched that lands a chosen particle exactly on an edge, and on the doubles next
to it.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _incremental_ref as R
import _swarm_fitness_ref as F
from _gpu_common import mods  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ["greedy", "maximizers", "expanders", "safe_set"]
LD = F.LD
PER_BAND_IN_RUN = 8         # particles of every band in the swarms of the run test
_GPS = {}


def _gp(gpy, spec, X, Y):
    return gpy.models.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpy.kern, spec),
                                   noise_var=R.NOISE)


def device_gps(mods, name):
    """The case's GPs on the device, built once."""
    if name not in _GPS:
        p = F.problem(name)
        _GPS[name] = [_gp(mods[1], p["specs"][g], p["X"][g], p["Y"][g]) for g in range(p["G"])]
    return [g._fitted() for g in _GPS[name]]


def fitness_raw(devs, kind, particles, fmin, scaling, blb, pad=64):
    """``sgp_swarm_fitness`` with outputs ``pad`` elements longer than the swarm: nothing may
    be written behind particle P - 1."""
    from safeopt_amd import _hip
    ctx = devs[0].ctx
    particles = _hip.f64(particles).reshape(-1, devs[0].d)
    P = particles.shape[0]
    values = np.full(P + pad, -7.25)
    safe = np.full(P + pad, 0xA5, dtype=np.uint8)
    ctx.check(_hip.lib().sgp_swarm_fitness(
        ctx.h, _hip._gp_array(devs), len(devs), _hip.SWARM_TYPES[kind], _hip.dptr(particles), P,
        float(F.BETA), _hip.dptr(_hip.f64(fmin)), _hip.dptr(_hip.f64(scaling)), float(blb),
        _hip.dptr(values), safe.ctypes.data_as(_hip.c_u8_p)))
    assert np.all(values[P:] == -7.25) and np.all(safe[P:] == 0xA5), "written past P = %d" % P
    assert np.all(safe[:P] <= 1)
    return values[:P].copy(), safe[:P].astype(bool)


def _check(name, what, got, safe, ref, tol, keep, keep0):
    """values within tol on ``keep``, safe equal on ``keep0``; returns max err / tol."""
    want = np.asarray(ref["values"], dtype=float)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want) / tol
    worst = float(err[keep].max())
    print("%s %s: max err / tol %.3e, left out %d of %d" % (name, what, worst,
                                                           np.count_nonzero(~keep), keep.size))
    assert_array_equal(safe[keep0], ref["safe"][keep0], err_msg=what)
    assert worst <= 1.0, what
    return worst


# ---- 3. bands with a margin ---------------------------------------------------------------------

@pytest.mark.parametrize("name", F.NAMES)
def test_base_types_band_by_band(mods, name):
    """k_fitness_small behind the VALU sweep (n = 10), the 4-wave sweep (n = 20; n = 130 with
    4097 particles) and the few-points path (n = 130): the four base types."""
    p = F.problem(name)
    devs = device_gps(mods, name)
    D = F.margin(name)
    slack = F.reference(name, "maximizers")["slack"]
    out, zero = F.left_out(slack, D), F.near_zero(slack, D)
    assert out.sum() <= 0.01 * out.size
    every = np.ones(out.size, dtype=bool)
    for kind in KINDS:
        v, s = fitness_raw(devs, kind, p["particles"], p["fmin"], p["scaling"],
                           p["best_lower_bound"])
        ref = F.reference(name, kind)
        banded = kind in ("maximizers", "expanders")
        _check(name, kind, v, s, ref, F.tolerance(name, kind, ref), ~out if banded else every,
               every if kind == "greedy" else ~zero)
        if kind == "greedy":
            assert s.all()
    if p["route"] != "few":
        assert devs[0].ctx.last_sweep() == F.SWEEP_OF[p["route"]]


@pytest.mark.parametrize("name", F.NAMES)
def test_hallucinated_swarm_band_by_band(mods, name):
    """k_fitness_hall: clones with one pending pick; the width term from the clone's variance,
    everything else from the real GPs."""
    from safeopt_amd import _hip
    p = F.problem(name)
    devs = device_gps(mods, name)
    D = F.margin(name)
    var_w = F.hall_variance(name)
    # the pending pick really narrows the width somewhere
    assert np.min(np.asarray(var_w / p["var"], dtype=float)) < 0.9
    clones = [g.clone() for g in devs]
    try:
        for c in clones:
            assert c.append(F.pending(name), 0.0)
        for kind in ("maximizers", "expanders"):
            ref = F.reference(name, kind, var_w)
            out, zero = F.left_out(ref["slack"], D), F.near_zero(ref["slack"], D)
            assert out.sum() <= 0.01 * out.size
            v, s = _hip.swarm_fitness_hall(devs[0].ctx, devs, clones, kind, p["particles"], F.BETA,
                                           p["fmin"], p["scaling"], p["best_lower_bound"])
            _check(name, "hall " + kind, v, s, ref, F.tolerance(name, kind, ref, var_w), ~out,
                   ~zero)
    finally:
        for c in clones:
            c.destroy()


def _mes_pen(devs, particles, fmin, scaling, ystar):
    """(v_c, v_u, safe): a 'mes' swarm's values with ``fmin`` and with every fmin = -inf."""
    from safeopt_amd import _hip
    ctx = devs[0].ctx
    vc, safe = _hip.swarm_fitness_mes(ctx, devs, particles, F.BETA, fmin, scaling, ystar)
    vu, open_ = _hip.swarm_fitness_mes(ctx, devs, particles, F.BETA, np.full(len(devs), -np.inf),
                                       scaling, ystar)
    assert open_.all()
    return vc, vu, safe


@pytest.mark.parametrize("name", F.NAMES)
def test_penalty_only_branch_band_by_band(mods, name):
    """The branch the thompson, mes and ise swarms share (``*value = total_pen``), the quadratic
    band included: the 'mes' value with the case's fmin minus the one with every fmin = -inf."""
    p = F.problem(name)
    devs = device_gps(mods, name)
    D = F.margin(name)
    ref = F.reference(name, "penalty")
    out, zero = F.left_out(ref["slack"], D), F.near_zero(ref["slack"], D)
    vc, vu, safe = _mes_pen(devs, p["particles"], p["fmin"], p["scaling"],
                            [float(p["Y"][0].max()) + 0.5])
    tol = F.tolerance(name, "penalty", ref) + 4 * F.EPS * (np.abs(vc) + np.abs(vu))
    want = np.asarray(ref["total_pen"], dtype=float)
    err = np.abs((vc - vu) - want)
    print("%s mes penalty: max err / tol %.3e, left out %d of %d, deepest penalty %.1f"
          % (name, (err / np.maximum(tol, 1e-300))[~out].max(), out.sum(), out.size, want.min()))
    assert_array_equal(safe[~zero], ref["safe"][~zero])
    assert np.all(err[~out] <= tol[~out])          # (a satisfied constraint at alpha = 0: 0 <= 0)
    assert want.min() < -300.0                     # the quadratic band is really there


# ---- 4. the edges themselves, exactly -----------------------------------------------------------

def _landing(lower, fmin, edge, order):
    """(p, scalings) with (lower[p] - fmin) / scalings[k] == edge, the double above it (towards
    0) and the double below it, for the first particle of ``order`` that has all three."""
    want = (edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf))
    found = 0
    for p in order:
        num = lower[p] - fmin
        cands = [num / edge]
        for _ in range(8):
            cands = [np.nextafter(cands[0], -np.inf)] + cands + [np.nextafter(cands[-1], np.inf)]
        cands = np.array(cands)
        q = num / cands
        hits = [cands[q == w] for w in want]
        found += hits[0].size > 0
        if all(h.size for h in hits):
            return p, [float(h[0]) for h in hits], found
    return None, None, found


def _configs(p):
    """GP 0 of the case alone, first of two and last of two, the other GP inactive."""
    yield "alone", [0], 0
    if p["G"] >= 2:
        yield "first", [0, 1], 0
        yield "last", [1, 0], 1


@pytest.mark.parametrize("name", F.NAMES)
def test_band_edges_exactly(mods, name):
    """Particles exactly on -0.001, -0.1, -1 and 0 and on the doubles next to them."""
    from safeopt_amd import _hip
    p = F.problem(name)
    all_devs = device_gps(mods, name)
    parts, P = p["particles"], p["particles"].shape[0]
    ystar = [float(p["Y"][0].max()) + 0.5]
    triples = 0
    for what, idx, t in _configs(p):
        devs = [all_devs[i] for i in idx]
        G, ctx = len(devs), all_devs[0].ctx
        mean, var = p["mean"][idx], p["var"][idx]
        kdiag = [p["kdiag"][i] for i in idx]
        scal0 = p["scaling"][idx].copy()
        f_t = float(p["fmin"][0])
        blb = p["best_lower_bound"]

        def fmin_vec(f):
            v = np.full(G, -np.inf)
            v[t] = f
            return v

        # the device's own lower bound of the GP under test
        if t == 0:
            lower, _ = fitness_raw(devs, "greedy", parts, fmin_vec(f_t), scal0, blb)
        last, _ = fitness_raw(devs, "safe_set", parts, fmin_vec(f_t), scal0, blb)
        if t == G - 1:
            if t == 0:
                assert_array_equal(lower, last)      # G = 1: both are GP 0's
            lower = last
        else:
            # 'safe_set' returns the lower bound of the last GP, an inactive one here
            lo_ref = np.asarray(mean[-1] - LD(F.BETA) * np.sqrt(var[-1]), dtype=float)
            D_last = F.slack_margin(mean, var, kdiag, scal0)[-1] * scal0[-1]
            assert np.all(np.abs(last - lo_ref) <= D_last)

        def check(f, scaling, tag, p_on, band_on):
            """Every call on these GPs against the band NumPy derives from the device's bits.
            The best lower bound is the upper bound of particle ``p_on``: its interest as a
            maximizer is the logistic's midpoint whatever the scaling, never saturated."""
            blb = float(mean[0, p_on] + LD(F.BETA) * np.sqrt(var[0, p_on]))
            num = lower - f
            s_bits = num / scaling[t]
            pen = F.penalty(s_bits.copy())
            bands = F.band(s_bits)
            assert bands[p_on] == band_on, (tag, s_bits[p_on])
            vc, vu, safe = _mes_pen(devs, parts, fmin_vec(f), scaling, ystar)
            assert_array_equal(safe, num >= 0, err_msg=tag)
            assert_array_equal(vc, vu + pen, err_msg=tag + ": total_pen, bit for bit")
            got = {}
            for kind in ("maximizers", "expanders"):
                v, s = fitness_raw(devs, kind, parts, fmin_vec(f), scaling, blb)
                assert_array_equal(s, num >= 0, err_msg=tag + " " + kind)
                ref = F.shape(kind, mean, var, fmin_vec(f), scaling, blb)
                ref["band"][t] = bands
                ref["total_pen"] = pen.astype(LD)
                ref["values"] = (ref["width"] + ref["total_pen"]) * ref["interest"]
                tol = F.value_tol(kind, ref, mean, var, kdiag, scaling)
                err = np.abs(v - np.asarray(ref["values"], dtype=float)) / tol
                assert err.max() <= 1.0, (tag, kind, float(err.max()), int(err.argmax()))
                got[kind] = (v, tol, np.asarray(ref["interest"], dtype=float), float(err.max()))
            _, s = fitness_raw(devs, "safe_set", parts, fmin_vec(f), scaling, blb)
            assert_array_equal(s, num >= 0, err_msg=tag + " safe_set")
            return pen, got

        # particles with a negative slack; for an edge, those first whose scaled slack is
        # closest to it under the case's scaling: the scaling that lands them stays close to it
        unsafe = np.flatnonzero(lower < f_t)
        s_case = (lower[unsafe] - f_t) / scal0[t]
        worst = 0.0
        for edge, b_on, b_above, b_below in ((-0.001, 2, 1, 2), (-0.1, 3, 2, 3), (-1.0, 5, 3, 4)):
            order = unsafe[np.argsort(np.abs(np.log(s_case / edge)))][:24]
            q, scalings, exact = _landing(lower, f_t, edge, order)
            assert q is not None, "%s %s: no particle lands on %g and both neighbours" % (
                name, what, edge)
            triples += 1
            res = []
            for sc, b in zip(scalings, (b_on, b_above, b_below)):
                scaling = scal0.copy()
                scaling[t] = sc
                res.append(check(f_t, scaling, "%s %s edge %g band %d" % (name, what, edge, b),
                                 q, b))
            (pen_on, on), (pen_ab, ab), (pen_be, be) = res
            if edge == -1.0:
                assert pen_on[q] == -1.0           # exactly -1: no factor
            # across the edge the value moves by the jump of the penalty
            for kind in ("maximizers", "expanders"):
                for (pa, a), (pb, b_) in (((pen_ab, ab), (pen_on, on)), ((pen_on, on), (pen_be, be))):
                    jump = (pa[q] - pb[q]) * a[kind][2][q]
                    tol = a[kind][1][q] + b_[kind][1][q]
                    assert abs((a[kind][0][q] - b_[kind][0][q]) - jump) <= tol
                jump = abs(pen_ab[q] - pen_on[q]) * on[kind][2][q]
                assert jump > 100 * (ab[kind][1][q] + on[kind][1][q]), (kind, edge)
                worst = max(worst, on[kind][3], ab[kind][3], be[kind][3])
        # edge 0: fmin on the particle's own lower bound and on the doubles next to it
        q = int(unsafe[np.argmax(s_case)])
        for f, b, ok in ((lower[q], 0, True), (np.nextafter(lower[q], np.inf), 1, False),
                         (np.nextafter(lower[q], -np.inf), 0, True)):
            pen, got = check(float(f), scal0, "%s %s edge 0 band %d" % (name, what, b), q, b)
            assert (pen[q] == 0.0) == ok
            if not ok:
                assert pen[q] == 2.0 * ((lower[q] - f) / scal0[t]) < 0.0
            worst = max(worst, got["maximizers"][3], got["expanders"][3])
        print("%s %s: exact landings on all three edges, every particle's band known: "
              "max err / tol %.3e" % (name, what, worst))
    print("%s: %d exact-edge triples" % (name, triples))


# ---- 5. structure and routes --------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in F.NAMES if len(F.CASES[n][3]) == 3])
def test_greedy_looks_at_gp_0_only(mods, name):
    p = F.problem(name)
    devs = device_gps(mods, name)
    args = (p["particles"], p["fmin"], p["scaling"], p["best_lower_bound"])
    v3, s3 = fitness_raw(devs, "greedy", *args)
    v1, s1 = fitness_raw(devs[:1], "greedy", p["particles"], p["fmin"][:1], p["scaling"][:1],
                         p["best_lower_bound"])
    assert_array_equal(v3, v1)
    fmin, scaling = p["fmin"].copy(), p["scaling"].copy()
    fmin[1:], scaling[1:] = np.nan, np.nan
    vn, sn = fitness_raw(devs, "greedy", p["particles"], fmin, scaling, p["best_lower_bound"])
    assert_array_equal(vn, v1)
    assert s3.all() and s1.all() and sn.all()


def test_an_inactive_gp_widens_values_and_nothing_else(mods):
    """[GP 0, wide, GP 1] with fmin = -inf for the wide GP against [GP 0, GP 1]: the wide GP
    (prior variance 60) has the largest sd / scaling at most particles."""
    name = "mat52_d3_g2_n20"
    p = F.problem(name)
    devs = device_gps(mods, name)
    spec = (("Matern52", (0, 1, 2), 60.0, tuple(R.lengthscales(3))),)
    wide_ref = R.RefGP(spec, p["X"][0], p["Y"][1])
    wide = _gp(mods[1], spec, p["X"][0], p["Y"][1])
    parts = p["particles"]
    m, v = wide_ref.predict(parts)
    mean = np.array([p["mean"][0], m, p["mean"][1]], dtype=LD)
    var = np.array([p["var"][0], v, p["var"][1]], dtype=LD)
    fmin = np.array([p["fmin"][0], -np.inf, p["fmin"][1]])
    scaling = np.array([p["scaling"][0], 1.0, p["scaling"][1]])
    kdiag = [p["kdiag"][0], 60.0, p["kdiag"][1]]
    blb = p["best_lower_bound"]
    three = [devs[0], wide._fitted(), devs[1]]
    D = F.slack_margin(mean, var, kdiag, scaling)
    ystar = [float(p["Y"][0].max()) + 0.5]
    for kind in ("maximizers", "expanders", "safe_set"):
        ref3 = F.shape(kind, mean, var, fmin, scaling, blb)
        ref2 = F.reference(name, kind)
        out, zero = F.left_out(ref3["slack"], D), F.near_zero(ref3["slack"], D)
        assert out.sum() <= 0.01 * out.size
        v3, s3 = fitness_raw(three, kind, parts, fmin, scaling, blb)
        v2, s2 = fitness_raw(devs, kind, parts, p["fmin"], p["scaling"], blb)
        assert_array_equal(s3, s2)                                  # it leaves `safe` alone
        tol = F.value_tol(kind, ref3, mean, var, kdiag, scaling)
        banded = kind != "safe_set"
        _check(name, "with a wide inactive GP, " + kind, v3, s3, ref3, tol,
               ~out if banded else ~np.zeros_like(out), ~zero)
        if banded:
            # the reference itself: wider at most particles, same penalty, interest G = 3 not 2
            w3, w2 = (np.asarray(r["width"], dtype=float) for r in (ref3, ref2))
            assert np.mean(w3 > 1.5 * w2) > 0.5
            assert_array_equal(np.asarray(ref3["total_pen"]), np.asarray(ref2["total_pen"]))
        if kind == "expanders":
            ratio = np.asarray(ref3["interest"] / ref2["interest"], dtype=float)
            assert np.allclose(ratio, 1.5, rtol=1e-15)
    # it adds no penalty: the penalty-only branch gives the two GPs' penalty
    ref = F.reference(name, "penalty")
    out = F.left_out(ref["slack"], F.margin(name))
    vc, vu, safe = _mes_pen(three, parts, fmin, scaling, ystar)
    tol = F.tolerance(name, "penalty", ref) + 4 * F.EPS * (np.abs(vc) + np.abs(vu))
    err = np.abs((vc - vu) - np.asarray(ref["total_pen"], dtype=float))
    assert np.all(err[~out] <= tol[~out])


@pytest.mark.parametrize("name", ["rbf_d2_g2_n130", "prod_d4_g3_n20"])
def test_maximizers_interest_at_saturation(mods, name):
    p = F.problem(name)
    devs = device_gps(mods, name)
    D = F.margin(name)
    ref = F.reference(name, "maximizers")
    out = F.left_out(ref["slack"], D)
    args = (p["particles"], p["fmin"], p["scaling"])
    # interest 0: (W + pen) * 0
    v, _ = fitness_raw(devs, "maximizers", *args, 1e6)
    assert np.all(np.abs(v) <= 1e-300)
    # interest 1: W + pen itself
    v, s = fitness_raw(devs, "maximizers", *args, -1e6)
    one = F.shape("maximizers", p["mean"], p["var"], p["fmin"], p["scaling"], -1e6)
    assert np.all(np.asarray(one["interest"], dtype=float) == 1.0)
    tol = F.value_tol("maximizers", one, p["mean"], p["var"], p["kdiag"], p["scaling"])
    _check(name, "interest 1", v, s, one, tol, ~out, ~F.near_zero(ref["slack"], D))
    # the midpoint: best lower bound = a particle's own upper bound
    q = int(np.flatnonzero(~out)[7])
    upper = float(p["mean"][0, q] + LD(F.BETA) * np.sqrt(p["var"][0, q]))
    v, s = fitness_raw(devs, "maximizers", *args, upper)
    mid = F.shape("maximizers", p["mean"], p["var"], p["fmin"], p["scaling"], upper)
    assert abs(float(mid["interest"][q]) - 0.5) < 1e-12
    tol = F.value_tol("maximizers", mid, p["mean"], p["var"], p["kdiag"], p["scaling"])
    _check(name, "interest 1/2", v, s, mid, tol, ~out, ~F.near_zero(ref["slack"], D))
    half = float(mid["width"][q] + mid["total_pen"][q]) / 2
    assert abs(v[q] - half) <= tol[q] and abs(half) > 100 * tol[q]


def test_prefixes_of_a_swarm_return_the_same_bits(mods):
    """P = 1 .. 4096 on n = 130 take the few-points path: a prefix call returns the bits of the
    4096-particle call; 4097 take a sweep and meet the reference; nothing is written past P."""
    name = "rbf_d2_g3_n130_sweep"
    p = F.problem(name)
    devs = device_gps(mods, name)
    D = F.margin(name)
    assert p["particles"].shape[0] == 4097
    for kind in KINDS:
        whole = fitness_raw(devs, kind, p["particles"][:4096], p["fmin"], p["scaling"],
                            p["best_lower_bound"])
        for P in (1, 64, 65, 256, 257):
            v, s = fitness_raw(devs, kind, p["particles"][:P], p["fmin"], p["scaling"],
                               p["best_lower_bound"])
            assert_array_equal(v, whole[0][:P], err_msg="%s P = %d" % (kind, P))
            assert_array_equal(s, whole[1][:P])
        ref = F.reference(name, kind)
        out, zero = F.left_out(ref["slack"], D), F.near_zero(ref["slack"], D)
        banded = kind in ("maximizers", "expanders")
        tol = F.tolerance(name, kind, ref)
        for P, (v, s) in ((4096, whole), (4097, fitness_raw(devs, kind, p["particles"], p["fmin"],
                                                            p["scaling"], p["best_lower_bound"]))):
            cut = {k: (a[..., :P] if isinstance(a, np.ndarray) else a) for k, a in ref.items()}
            every = np.ones(P, dtype=bool)
            _check(name, "%s P = %d" % (kind, P), v, s, cut, tol[:P],
                   ~out[:P] if banded else every, every if kind == "greedy" else ~zero[:P])


@pytest.mark.parametrize("name,P", [("mat52_d3_g2_n20", 64), ("mat52_d3_g3_n130", 64),
                                    ("mat52_d3_g3_n130", 65), ("mat52_d3_g2_n20", 65)])
def test_the_run_shapes_as_the_fitness_call_does(mods, name, P):
    """``sgp_swarm_run(init=1, iters=0)``: ``best_values`` is the fitness of the positions.  Up
    to 64 particles the shaping is the copy inside k_pso_small_step, behind a sweep (n = 20) and
    behind the few-points posterior (n = 130); 65 take the general launches.  The particles are
    the case's last P: the designed ones of every band among them."""
    from safeopt_amd import _hip
    p = F.problem(name)
    devs = device_gps(mods, name)
    d = p["d"]
    pos = np.ascontiguousarray(p["particles"][-P:])
    bands = F.reference(name, "maximizers")["band"][:, -P:]
    assert all(np.count_nonzero(bands == b) >= PER_BAND_IN_RUN for b in range(5))
    for kind in KINDS:
        want, _ = fitness_raw(devs, kind, pos, p["fmin"], p["scaling"], p["best_lower_bound"])
        state = [pos.copy(), np.empty((P, d)), np.empty((P, d)), np.empty(P), np.empty(d)]
        rand = np.random.default_rng(P).random(P * d)
        _hip.swarm_run(devs[0].ctx, devs, kind, F.BETA, p["fmin"], p["scaling"],
                       p["best_lower_bound"], *state, np.full(d, 0.3), None, 1, 0, 1.0, 0.0, rand)
        assert_array_equal(state[3], want, err_msg=kind)
        assert_array_equal(state[2], pos)
        assert_array_equal(state[0], pos)
        assert_array_equal(state[1], rand.reshape(P, d) * 0.3)
        assert_array_equal(state[4], pos[np.argmax(want)])
