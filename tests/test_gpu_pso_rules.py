"""The PSO update on the device, rule by rule (needs an MI355X).

The update exists twice: k_pso_move / k_pso_best / k_pso_gbest (csrc/swarm.hip) and again
inside k_pso_small_step, the one-workgroup iteration of a swarm of up to 64 particles.  Each
test hands ``sgp_swarm_run`` a hand-made state (``init=0``, an explicit ``rand`` array) that is
built to reach one rule of safeopt/swarm.py:98-143 -- the +-10 velocity_scale clamp, the clip
to the bounds, "an unsafe improvement is not kept", "an equal value is not an improvement",
the first index among equal personal bests -- and compares all five state arrays, bit for
bit, with ``restate`` below, a NumPy restatement of those lines on the same numbers whose
fitness is the device's fitness call on the moved positions.

P = 64 runs in k_pso_small_step (its first move is a k_pso_move launch, every later move is
its own), 65, 1025 and 3000 take the general launches: one, two and three strides of
k_pso_gbest's 1024-thread scan.  d = 1 and 8 sit on GPs of 20 observations (posterior by a
sweep), d = 3 on GPs of 130 (few-points posterior)."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _incremental_ref as R
from _gpu_common import mods, smooth  # noqa: F401

pytestmark = pytest.mark.gpu

BETA = 2.0
SCALING = np.array([1.0, 1.2])
OPEN = np.array([-np.inf, -np.inf])
SHAPES = [(P, d) for d in (1, 3, 8) for P in (64, 65, 1025, 3000)]
_GPS = {}


def device_gps(mods, d):
    """Two GPs on d inputs, built once."""
    if d not in _GPS:
        n = 130 if d == 3 else 20
        rng = np.random.default_rng(70 + d)
        gps = []
        for g in range(2):
            X = rng.uniform(-2, 2, size=(n, d))
            gps.append(mods[1].models.GPRegression(
                X, smooth(X, 3 + g) + 0.3, R.make_kernel(mods[1].kern, R.single("Matern52", d)),
                noise_var=R.NOISE))
        _GPS[d] = gps
    return [g._fitted() for g in _GPS[d]]


def fitness(devs, kind, fmin, pos, blb=0.0):
    from safeopt_amd import _hip
    return _hip.swarm_fitness(devs[0].ctx, devs, kind, pos, BETA, fmin, SCALING, blb)


def run(devs, kind, fmin, state, vscale, bounds, rand, iters=1, step=0.0, blb=0.0):
    """``sgp_swarm_run(init=0)`` on a copy of ``state``."""
    from safeopt_amd import _hip
    st = [np.ascontiguousarray(a, dtype=float).copy() for a in state]
    _hip.swarm_run(devs[0].ctx, devs, kind, BETA, fmin, SCALING, blb, *st, vscale, bounds, 0, iters,
                   1.0, step, rand)
    return st


def restate(devs, kind, fmin, state, vscale, bounds, rand, iters=1, step=0.0, blb=0.0):
    """safeopt/swarm.py:98-143 on the same numbers (c1 = c2 = 1)."""
    pos, vel, best, bv, gb = (np.array(a, dtype=float) for a in state)
    P, d = pos.shape
    inertia = 1.0
    for it in range(iters):
        r = rand[2 * P * d * it:2 * P * d * (it + 1)].reshape(2 * P, d)
        to_global, to_own = gb - pos, best - pos
        vel = vel * inertia
        vel = vel + (r[:P] * to_own + r[P:] * to_global) / vscale
        vel = np.clip(vel, -(10 * vscale), 10 * vscale)
        pos = pos + vel
        if bounds is not None:
            pos = np.clip(pos, bounds[:, 0], bounds[:, 1])
        inertia += step
        values, safe = fitness(devs, kind, fmin, pos, blb)
        take = (values > bv) & safe
        bv[take], best[take] = values[take], pos[take]
        gb = best[np.argmax(bv)].copy()
    return [pos, vel, best, bv, gb]


def same(got, want, what=""):
    for name, a, b in zip(("positions", "velocities", "best_positions", "best_values",
                           "global_best"), got, want):
        assert_array_equal(a, b, err_msg="%s %s" % (what, name))


def random_state(P, d, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, size=(P, d))
    vel = rng.uniform(-0.3, 0.3, size=(P, d))
    best = rng.uniform(-1, 1, size=(P, d))
    bv = rng.uniform(-2, -1, size=P)
    vscale = rng.uniform(0.2, 0.5, size=d)
    return [pos, vel, best, bv, best[np.argmax(bv)].copy()], vscale, rng


@pytest.mark.parametrize("P,d", SHAPES)
def test_velocity_clamp(mods, P, d):
    devs = device_gps(mods, d)
    state, vscale, rng = random_state(P, d, P + d)
    sign = np.where(rng.random((P, d)) < 0.5, -1.0, 1.0)
    state[1] = sign * 1e3 * vscale
    rand = rng.random(2 * P * d)
    got = run(devs, "maximizers", OPEN, state, vscale, None, rand)
    assert_array_equal(got[1], sign * (10 * vscale))
    assert_array_equal(got[0], state[0] + sign * (10 * vscale))
    same(got, restate(devs, "maximizers", OPEN, state, vscale, None, rand))


@pytest.mark.parametrize("P,d", SHAPES)
def test_clip_to_the_bounds(mods, P, d):
    devs = device_gps(mods, d)
    state, vscale, rng = random_state(P, d, 2 * P + d)
    bounds = np.stack([-rng.uniform(0.5, 1.0, size=d), rng.uniform(0.5, 1.0, size=d)], axis=1)
    side = rng.integers(0, 2, size=(P, d))
    state[0] = np.where(side == 1, bounds[:, 1], bounds[:, 0])
    state[1] = np.where(side == 1, 0.5, -0.5) * vscale          # outward
    rand = np.zeros(2 * P * d)                                  # no pull
    got = run(devs, "maximizers", OPEN, state, vscale, bounds, rand)
    assert_array_equal(got[0], state[0])
    assert_array_equal(got[1], state[1])
    same(got, restate(devs, "maximizers", OPEN, state, vscale, bounds, rand))
    free = run(devs, "maximizers", OPEN, state, vscale, None, rand)
    assert_array_equal(free[0], state[0] + state[1])
    assert np.all(free[0] != state[0])
    same(free, restate(devs, "maximizers", OPEN, state, vscale, None, rand))
    # with a pull: particles inside, some of which a large step takes across a bound
    state, vscale, rng = random_state(P, d, 3 * P + d)
    state[1] *= 10
    rand = rng.random(2 * P * d)
    got = run(devs, "maximizers", OPEN, state, vscale, bounds, rand)
    on = (got[0] == bounds[:, 0]) | (got[0] == bounds[:, 1])
    assert 0 < on.sum() < on.size
    same(got, restate(devs, "maximizers", OPEN, state, vscale, bounds, rand))


@pytest.mark.parametrize("P,d", SHAPES)
def test_an_unsafe_improvement_is_not_kept(mods, P, d):
    devs = device_gps(mods, d)
    state, vscale, rng = random_state(P, d, 4 * P + d)
    state[3] = np.full(P, -1e300)
    state[4] = state[2][0].copy()
    rand = rng.random(2 * P * d)
    unsafe = np.array([1e6, -np.inf])
    got = run(devs, "maximizers", unsafe, state, vscale, None, rand)
    values, safe = fitness(devs, "maximizers", unsafe, got[0])
    assert not safe.any() and np.all(values > -1e300)
    assert_array_equal(got[2], state[2])
    assert_array_equal(got[3], state[3])
    assert_array_equal(got[4], state[2][0])
    same(got, restate(devs, "maximizers", unsafe, state, vscale, None, rand))
    got = run(devs, "maximizers", OPEN, state, vscale, None, rand)
    values, safe = fitness(devs, "maximizers", OPEN, got[0])
    assert safe.all()
    assert_array_equal(got[2], got[0])
    assert_array_equal(got[3], values)
    same(got, restate(devs, "maximizers", OPEN, state, vscale, None, rand))


@pytest.mark.parametrize("P,d", SHAPES)
def test_an_equal_value_is_not_an_improvement(mods, P, d):
    devs = device_gps(mods, d)
    state, vscale, rng = random_state(P, d, 5 * P + d)
    state[1] = np.zeros((P, d))
    state[2] = state[0] + 1.0
    state[3], safe = fitness(devs, "maximizers", OPEN, state[0])
    assert safe.all()
    state[4] = state[2][np.argmax(state[3])].copy()
    rand = np.zeros(2 * P * d)
    got = run(devs, "maximizers", OPEN, state, vscale, None, rand)
    assert_array_equal(got[0], state[0])                    # nothing moved
    assert_array_equal(got[2], state[2])
    assert_array_equal(got[3], state[3])
    same(got, restate(devs, "maximizers", OPEN, state, vscale, None, rand))


@pytest.mark.parametrize("P,d", SHAPES)
def test_first_index_among_equal_personal_bests(mods, P, d):
    """Equal maxima in one wave, in two waves, on both sides of a 1024 stride (in two threads
    and in one thread of k_pso_gbest's scan), at both ends."""
    devs = device_gps(mods, d)
    plants = [(5, 37), (5, 69), (70, 1027), (3, 1027), (1023, 1024), (0, P - 1), (P - 1,)]
    ran = 0
    for plant in plants:
        if max(plant) >= P:
            continue
        state, vscale, rng = random_state(P, d, 6 * P + d + ran)
        state[3][list(plant)] = 1e300
        rand = rng.random(2 * P * d)
        got = run(devs, "maximizers", OPEN, state, vscale, None, rand)
        assert len(np.unique(got[2], axis=0)) == P          # distinct best positions
        assert np.count_nonzero(got[3] == 1e300) == len(plant)
        assert int(np.argmax(got[3])) == plant[0]
        assert_array_equal(got[4], got[2][plant[0]], err_msg=str(plant))
        same(got, restate(devs, "maximizers", OPEN, state, vscale, None, rand), str(plant))
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("kind", ["greedy", "maximizers", "expanders"])
@pytest.mark.parametrize("P,d", SHAPES)
def test_whole_step(mods, P, d, kind):
    """A random state with half of the particles unsafe: one iteration, and two with a falling
    inertia (at P = 64 the second move is k_pso_small_step's own)."""
    devs = device_gps(mods, d)
    state, vscale, rng = random_state(P, d, 7 * P + d)
    bounds = np.array([[-1.5, 1.5]] * d)
    rand2 = rng.random(4 * P * d)
    # (the first move does not depend on the fitness: fmin is the median lower bound of GP 0 at
    # the positions the particles move to)
    moved = restate(devs, "greedy", OPEN, state, vscale, bounds, rand2)[0]
    lower, _ = fitness(devs, "greedy", OPEN, moved)
    fmin = np.array([float(np.median(lower)), -np.inf])
    state[3], _ = fitness(devs, kind, fmin, state[2], 0.2)
    u = rng.random(P)
    state[3][u < 0.3] = -1e300                  # these improve wherever they are safe
    state[3][u > 0.7] = 1e300                   # these never do (and tie for the global best)
    state[4] = state[2][np.argmax(state[3])].copy()
    for iters, step in ((1, 0.0), (2, -0.45)):
        rand = rand2[:2 * P * d * iters]
        got = run(devs, kind, fmin, state, vscale, bounds, rand, iters, step, 0.2)
        want = restate(devs, kind, fmin, state, vscale, bounds, rand, iters, step, 0.2)
        same(got, want, "%d iterations" % iters)
        kept = np.any(got[2] != state[2], axis=1)
        assert 0 < kept.sum() < P                           # some improved, some did not
