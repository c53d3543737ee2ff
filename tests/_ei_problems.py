"""The converged run of the expected-improvement tests, in the form ``_gpu_common.build_opt``
takes (``z``, ``meta``), and its host restatement (oracle posterior, safe set).

``converged``: 1000 rows on [-1, 1], RBF, 12 observations spread over the interval and 30
repeats at the optimum, noise 1e-3^2 -- sigma is small on every row, and with a margin
``XI = 0.5`` the improvement asked for lies hundreds of sigma above every row: EI is exactly 0
everywhere, ln EI is between -1e4 and -1e8.
"""
import numpy as np

BETA, FMIN, NOISE, XI = 2.0, 0.0, 1e-3 ** 2, 0.5


def _f(x):
    return 1.5 - (x - 0.2) ** 2


def converged():
    from safeopt_amd import linearly_spaced_combinations
    rng = np.random.default_rng(23)
    X = np.concatenate([np.linspace(-0.95, 0.95, 12), np.full(30, 0.2)])[:, None]
    Y = _f(X) + 1e-3 * rng.standard_normal(X.shape)
    spec = [dict(kind="RBF", input_dim=1, variance=1.7, lengthscale=[0.6], ARD=True,
                 active_dims=[0])]
    z = {"it0_X0": X, "it0_Y0": Y, "beta_all": np.array([BETA]),
         "parameter_set": linearly_spaced_combinations([[-1.0, 1.0]], [1000])}
    meta = {"kernels": [spec], "noise_vars": [NOISE], "lipschitz": None, "fmin": [FMIN],
            "threshold": 0.1, "num_contexts": 0}
    return z, meta


def host_state():
    """Oracle posterior ``(mean (N,), var (N,))`` of the objective and the safe set ``S``."""
    from oracle import gp_numpy as gpn
    from _golden import make_kernel
    z, meta = converged()
    gp = gpn.GPRegression(z["it0_X0"], z["it0_Y0"], make_kernel(gpn, meta["kernels"][0]),
                          noise_var=NOISE)
    mean, var = gp.predict_noiseless(z["parameter_set"])
    mean, var = mean[:, 0], np.maximum(var[:, 0], 1e-15)
    return mean, var, mean - BETA * np.sqrt(var) > FMIN


def top_two_gap(alpha, S):
    """The two largest alpha over the rows of ``S``: their difference."""
    a = np.sort(alpha[S])
    return a[-1] - a[-2]
