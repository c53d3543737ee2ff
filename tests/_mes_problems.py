"""The two grids of the max-value entropy search tests, in the form ``_gpu_common.build_opt``
takes (``z``, ``meta``), and their host restatement: oracle posterior, safe set, sample paths in
NumPy (tests/_paths_numpy.py) and alpha (tests/_mes_ref.py).

  * ``line``: 1000 rows on [-3, 3], RBF, 8 observations -- four workgroups of the grid kernel,
    the last one ragged;
  * ``plane``: 70 x 70 = 4900 rows on [-2, 2]^2, Matern-5/2 (ARD), 30 observations -- twenty
    workgroups, the last one ragged; in 2 and 4 shards rows that are no multiple of 256.
"""
import numpy as np

PATHS, FEATURES = 16, 256
#: seeds of ``np.random.seed`` for the end-to-end picks (tests/test_mes_cpu.py verifies on the
#: host that the two largest alpha over S differ by more than 1e-9 for every one of them)
SEEDS = {"line": (3, 11), "plane": (5, 8)}
BETA, FMIN, NOISE = 2.0, 0.0, 0.05 ** 2


def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


def problem(name):
    """``(z, meta)``: the data as ``it0_*`` arrays, the kernel as a fixture spec."""
    from safeopt_amd import linearly_spaced_combinations
    if name == "line":
        d, n, shape, lim = 1, 8, [1000], 3.0
        spec = [dict(kind="RBF", input_dim=1, variance=1.7, lengthscale=[0.6], ARD=True,
                     active_dims=[0])]
        rng = np.random.default_rng(17)
        X = rng.uniform(-1.2, 1.2, size=(n, d))
    else:
        d, n, shape, lim = 2, 30, [70, 70], 2.0
        spec = [dict(kind="Matern52", input_dim=2, variance=1.5, lengthscale=[0.7, 0.9],
                     ARD=True, active_dims=[0, 1])]
        rng = np.random.default_rng(7)
        X = rng.uniform(-1.5, 1.5, size=(n, d))
    Y = _smooth(X, 41)
    Y = Y - Y.min() + 0.5
    z = {"it0_X0": X, "it0_Y0": Y, "beta_all": np.array([BETA]),
         "parameter_set": linearly_spaced_combinations([[-lim, lim]] * d, shape)}
    meta = {"kernels": [spec], "noise_vars": [NOISE], "lipschitz": None, "fmin": [FMIN],
            "threshold": 0.1, "num_contexts": 0}
    return z, meta


def host_state(name):
    """Oracle posterior ``(mean (N,), var (N,))`` of the objective and the safe set ``S``."""
    from oracle import gp_numpy as gpn
    from _golden import make_kernel
    z, meta = problem(name)
    gp = gpn.GPRegression(z["it0_X0"], z["it0_Y0"], make_kernel(gpn, meta["kernels"][0]),
                          noise_var=NOISE)
    mean, var = gp.predict_noiseless(z["parameter_set"])
    mean, var = mean[:, 0], np.maximum(var[:, 0], 1e-15)
    return mean, var, mean - BETA * np.sqrt(var) > FMIN


def host_ystar(name, seed, S):
    """The maxima over ``S`` of the paths ``mes_point`` draws under ``np.random.seed(seed)``."""
    import _paths_numpy as pn
    from safeopt_amd.paths import draw_path_inputs
    z, meta = problem(name)
    part = meta["kernels"][0][0]
    kinds = [dict(RBF=pn.RBF, Matern32=pn.MATERN32, Matern52=pn.MATERN52)[part["kind"]]]
    inv_ls = 1.0 / np.asarray(part["lengthscale"], dtype=float)[None, :]
    kern = (kinds, [part["variance"]], inv_ls)
    X, Y = z["it0_X0"], z["it0_Y0"]
    rng = np.random.RandomState(seed)
    Om, b, W, E = draw_path_inputs((kinds, inv_ls), NOISE, X.shape[0], X.shape[1], PATHS,
                                   FEATURES, rng=rng)
    V = pn.path_weights(kern, NOISE, X, Y, Om, b, W, E)
    f = pn.paths_eval(kern, X, Om, b, W, V, z["parameter_set"][S])
    return f.max(0)


def top_two_gap(alpha, S):
    """The two largest alpha over the rows of ``S``: their difference."""
    a = np.sort(alpha[S])
    return a[-1] - a[-2]
