"""A whole config-5 ``SafeOptSwarm.optimize()`` on one GPU: d = 4, two GPs of 2000
observations, 1e5 particles per swarm, the device generator.  What the reference cannot
run at this size (the 80 GB ``K(B, [S; B])`` of gp_opt.py:1093): the swarms, the growth of
the safe set by 1e5 candidates at a time and the recheck of the grown set."""
import numpy as np
import pytest

from _gpu_common import mods  # noqa: F401

pytestmark = pytest.mark.gpu


def _optimize(sa, gpy, cfg, build_gps):
    np.random.seed(11)
    gps = build_gps(cfg, gpy)
    opt = sa.SafeOptSwarm(gps, cfg["fmin"], bounds=[(-5., 5.)] * cfg["d"],
                          threshold=cfg["threshold"], swarm_size=100_000, pso="device-rng")
    m0 = opt.S.shape[0]
    x = opt.optimize()
    return opt, m0, np.array(x)


@pytest.mark.timeout(900)
def test_config5_optimize_full_size(mods):
    sa, gpy, gpn, _ = mods
    from bench import make_config, build_gps
    cfg = make_config(5, side=1000)
    opt, m0, x = _optimize(sa, gpy, cfg, build_gps)
    assert x.shape == (4,) and np.all(np.isfinite(x))
    assert np.all(x >= -5.0) and np.all(x <= 5.0)
    _, safe = opt._compute_particle_fitness("safe_set", x[None, :])
    assert bool(safe[0])
    S = opt.S
    assert S.shape[0] > m0                                  # the safe set grew
    # appended rows: at most 0.95-correlated with every earlier row (GP 0's kernel)
    ko = build_gps(cfg, gpn)[0].kern
    scale2 = float(opt.scaling[0]) ** 2
    rng = np.random.default_rng(0)
    rows = rng.choice(np.arange(m0, S.shape[0]), size=min(40, S.shape[0] - m0), replace=False)
    for r in rows:
        c = ko.K(S[r:r + 1], S[:r]) / scale2
        assert np.max(c) <= 0.95 + 1e-9, (r, np.max(c))
    # a second seeded run gives the same bits
    opt2, _, x2 = _optimize(sa, gpy, cfg, build_gps)
    assert np.array_equal(x, x2)
    assert np.array_equal(opt.S, opt2.S)
    assert np.array_equal(opt.greedy_point, opt2.greedy_point)
