"""The long-double swarm fitness and its case table (tests/_swarm_fitness_ref.py) leave
nothing out -- checked without a GPU.

Per case: every band of every active GP holds at least eight particles farther than the margin
D from every band edge, at most 1 % of the particles lie within D of an edge (the ones, and the
only ones, tests/test_gpu_swarm_fitness.py may leave out), and the reference agrees with the
float64 oracle to float64 rounding on the random particles.  ``SafeOptSwarm._compute_penalty``
gives the reference's penalties on the designed slacks and on the band edges themselves."""
import numpy as np
import pytest

import _incremental_ref as R
import _swarm_fitness_ref as F

KINDS = ["greedy", "maximizers", "expanders", "safe_set"]


@pytest.mark.parametrize("name", F.NAMES)
def test_every_band_is_filled_and_few_particles_sit_on_an_edge(name):
    p = F.problem(name)
    ref = F.reference(name, "maximizers")
    D = F.margin(name)
    kind, d, n, pattern, route = F.CASES[name]
    P = p["particles"].shape[0]
    assert P == (F.N_SWEEP if route == "sweep" else F.N_RANDOM + 40 * sum(pattern))
    assert P <= 4096 or route == "sweep"
    out = F.left_out(ref["slack"], D)
    print("%s: %d particles, %d left out, max D %.2e" % (name, P, out.sum(), D.max()))
    assert out.sum() <= 0.01 * P
    assert D.max() < 1e-6                      # a margin far below the narrowest band
    far = F.edge_distance(ref["slack"]) > D
    for g, active in enumerate(pattern):
        if not active:
            assert np.all(ref["band"][g] == -1) and np.all(np.isnan(ref["slack"][g]))
            continue
        for b in range(5):
            assert np.count_nonzero((ref["band"][g] == b) & far[g]) >= F.PER_BAND, (g, b)
        # the designed ones sit where they were put, the quadratic ones above -3
        for gg, b, row in p["designed"]:
            if gg != g:
                continue
            s = np.asarray(ref["slack"][g, row:row + F.PER_BAND], dtype=float)
            np.testing.assert_allclose(s, F.TARGETS[b], rtol=1e-6, atol=0)
            assert np.all(ref["band"][g, row:row + F.PER_BAND] == b)
            assert np.all(s >= -3.0)
    # the random particles spread over the bands as the quantiles were chosen
    s0 = np.asarray(ref["slack"][0, :F.N_RANDOM], dtype=float)
    assert np.quantile(s0, 0.9) == pytest.approx(0.5, abs=1e-9)
    assert np.quantile(s0, 0.05) == pytest.approx(-3.0, abs=1e-9)
    assert 0 < ref["safe"].sum() < P


@pytest.mark.parametrize("name", F.NAMES)
def test_reference_agrees_with_the_float64_oracle(name):
    from oracle import gp_numpy as gpn, safeopt_numpy as son
    p = F.problem(name)
    gos = [gpn.GPRegression(p["X"][g], p["Y"][g][:, None], R.make_kernel(gpn, p["specs"][g]),
                            noise_var=R.NOISE) for g in range(p["G"])]
    parts = p["particles"][:F.N_RANDOM]
    D = F.margin(name)[:, :F.N_RANDOM]
    for kind in KINDS:
        ref = F.reference(name, kind)
        v, s = son.swarm_fitness(gos, parts, kind, F.BETA, p["fmin"], p["scaling"],
                                 p["best_lower_bound"])
        keep = ~F.left_out(ref["slack"][:, :F.N_RANDOM], D)
        want = np.asarray(ref["values"][:F.N_RANDOM], dtype=float)
        np.testing.assert_array_equal(s[keep], ref["safe"][:F.N_RANDOM][keep])
        # a float64 implementation of the same formulas has to stay within 1 % of the bound the
        # device is held to (F.value_tol: MEAN_TOL, VAR_TOL and the slopes), as in
        # tests/test_incremental_ref_cpu.py
        tol = F.tolerance(name, kind)[:F.N_RANDOM]
        err = (np.abs(v - want) / tol)[keep]
        print("%s %s: max |oracle - reference| / tol %.2e" % (name, kind, err.max()))
        assert err.max() < 0.01


def test_compute_penalty_on_the_designed_slacks_and_on_the_edges():
    from safeopt_amd import SafeOptSwarm
    inf = np.inf
    pts = [0.0, -0.0, 5e-324, -5e-324, 1.0, -3.0, -2.5]
    for e in (-0.001, -0.1, -1.0):
        pts += [e, np.nextafter(e, inf), np.nextafter(e, -inf)]
    pts += [np.nextafter(0.0, inf), np.nextafter(0.0, -inf)]
    s = np.concatenate([np.array(pts)] + [F.TARGETS[b] for b in range(5)])
    got = SafeOptSwarm._compute_penalty(None, s)
    want = F.penalty(s.copy())
    np.testing.assert_array_equal(got, want)
    lin = s >= -1            # (2 s, 5 s and 10 s are exact in long double: one rounding)
    np.testing.assert_array_equal(got[lin], np.asarray(F.penalty(s.astype(F.LD)), dtype=float)[lin])
    # the rule itself, spelled out at the edges
    rule = {0.0: 0.0, -0.001: 5 * -0.001, np.nextafter(-0.001, inf): 2 * np.nextafter(-0.001, inf),
            -0.1: 10 * -0.1, np.nextafter(-0.1, inf): 5 * np.nextafter(-0.1, inf),
            -1.0: -1.0, np.nextafter(-1.0, inf): 10 * np.nextafter(-1.0, inf),
            np.nextafter(-1.0, -inf): -300 * np.nextafter(-1.0, -inf) ** 2}
    for x, y in rule.items():
        assert SafeOptSwarm._compute_penalty(None, x)[0] == y, x
    assert list(F.band(np.array([0.0, -5e-324, -0.001, -0.1, -1.0, np.nextafter(-1.0, -inf)]))) == [
        0, 1, 2, 3, 5, 4]
