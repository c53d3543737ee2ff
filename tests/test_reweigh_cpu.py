"""The in-place re-weighting of one observation, stated in float64 NumPy, against
long-double refits (tests/_reweigh_ref.py) on every case of the GPU table
(tests/test_gpu_reweigh.py): the formulas the device runs lose nothing a float64 refit keeps.
Bound: 1e-9 on L^-1 (absolute) and alpha (relative to max |alpha|), a tenth of the GPU
tolerance.  Also here: the new symbols of the C ABI, without a device.
"""
import os
import re

import numpy as np
import pytest

import _reweigh_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9
NEW_SYMBOLS = ("sgp_gp_set_data_w", "sgp_gp_append_w", "sgp_gp_append_block_w", "sgp_gp_reweigh",
               "sgp_gp_get_noise_scale", "sgp_grid_rank1_reweigh")


def reweigh_numpy(M, alpha, i, delta, dy):
    """``(M', alpha', p, P_ii, tau, eta)`` in float64, in the order of the device's sums.

    M = L^-1, c = column i of M, P_ii = |c|^2, p = M^T c, q_k = 1 + delta sum_{i<=j<=k} c_j^2:
    row k of M' = sqrt(q_{k-1} / q_k) M[k] - delta c_k / sqrt(q_{k-1} q_k) S_k with the running
    sum S_k = sum_{i <= j < k} c_j M[j]; alpha' = alpha + eta p."""
    n = M.shape[0]
    c = M[:, i].copy()
    Pii = float(c @ c)
    p = M.T @ c
    q_end = 1.0 + delta * Pii
    assert q_end > 0
    tau = delta / q_end
    eta = (dy - delta * alpha[i]) / q_end
    out = M.copy()
    S = np.zeros(n)
    pre = 0.0
    for k in range(i, n):
        q0 = 1.0 + delta * pre
        pre += c[k] * c[k]
        q1 = 1.0 + delta * pre
        assert q1 > 0
        out[k] = np.sqrt(q0 / q1) * M[k] + (-delta * c[k] / np.sqrt(q0 * q1)) * S
        S = S + c[k] * M[k]
    return out, alpha + eta * p, p, Pii, tau, eta


def recurrence_numpy(c, i, tau):
    """The row coefficients by the recurrence from the last row up: a_{n-1} = -tau, d_k = 1 +
    a_k c_k^2, g_k = a_k c_k / sqrt(d_k), a_{k-1} = a_k / d_k."""
    n = len(c)
    sd, g = np.ones(n), np.zeros(n)
    a = -tau
    for k in range(n - 1, i - 1, -1):
        d = 1.0 + a * c[k] * c[k]
        assert d > 0
        sd[k], g[k] = np.sqrt(d), a * c[k] / np.sqrt(d)
        a = a / d
    return sd, g


@pytest.fixture(scope="module")
def worst():
    w = {"Linv": (0.0, None), "alpha": (0.0, None)}
    yield w
    print("\nworst over the cases: L^-1 %.2e (%s), alpha %.2e (%s)"
          % (w["Linv"] + w["alpha"]))


@pytest.mark.parametrize("name", sorted(R.REWEIGH_CASES))
def test_formulas_against_the_refit(name, worst):
    X, Y, r, Xs, i, y_new, r_new, before, after = R.reweigh_reference(name)
    s = R.NOISE + 1e-8
    delta = s * r_new - s * r[i]
    mode = R.REWEIGH_CASES[name][4]
    assert {"less_noise": delta < 0, "more_noise": delta > 0, "scale_only": y_new == Y[i],
            "value_only": delta == 0}[mode]
    M, alpha, p, Pii, tau, eta = reweigh_numpy(before["Linv"], before["alpha"], i, delta,
                                               y_new - Y[i])
    el = np.max(np.abs(M - after["Linv"]))
    ea = np.max(np.abs(alpha - after["alpha"])) / np.max(np.abs(after["alpha"]))
    print("%s: L^-1 %.2e  alpha %.2e  (1 + delta P_ii = %.3g)" % (name, el, ea, 1 + delta * Pii))
    for key, e in (("Linv", el), ("alpha", ea)):
        if e > worst[key][0]:
            worst[key] = (e, name)
    assert np.all(M[np.triu_indices(len(Y), 1)] == 0.0) and np.all(np.diag(M) > 0.0)
    assert el < BOUND and ea < BOUND
    # the recurrence from the last row up gives the same coefficients as the running sums
    c = before["Linv"][:, i]
    sd, g = recurrence_numpy(c, i, tau)
    pre = np.concatenate([[0.0], np.cumsum(c[i:] ** 2)])
    q = 1.0 + delta * pre
    assert np.allclose(sd[i:], np.sqrt(q[:-1] / q[1:]), rtol=1e-10, atol=0)
    assert np.allclose(g[i:], -delta * c[i:] / np.sqrt(q[:-1] * q[1:]), rtol=1e-9, atol=1e-300)


@pytest.mark.parametrize("name", sorted(n for n, c in R.REWEIGH_CASES.items() if c[2] in (65, 130)))
def test_refresh_record(name):
    """The record in the layout of an append record: x_i, w = -p / P_ii off row i; then
    c~ = k(x, x_i) - k(X, x)^T w = c / P_ii, mean += c~ P_ii eta, var += c~^2 tau P_ii^2 -- the
    refit's posterior at the test rows."""
    spec = R.REWEIGH_CASES[name][0]
    X, Y, r, Xs, i, y_new, r_new, before, after = R.reweigh_reference(name)
    s = R.NOISE + 1e-8
    delta = s * r_new - s * r[i]
    _, _, p, Pii, tau, eta = reweigh_numpy(before["Linv"], before["alpha"], i, delta,
                                           y_new - Y[i])
    w = -p / Pii
    w[i] = 0.0
    Kx = R.f64(R.I.kern(spec, X, Xs))
    ct = Kx[i] - w @ Kx
    mean = before["mean"] + ct * (Pii * eta)
    var = np.maximum(before["var"] + ct * ct * (tau * Pii * Pii), 1e-15)
    kd = R.kdiag(spec)
    em = np.max(np.abs(mean - after["mean"])) / np.max(np.abs(after["mean"]))
    ev = np.max(np.abs(var - after["var"])) / kd
    print("%s: mean %.2e  var %.2e" % (name, em, ev))
    assert em < BOUND and ev < BOUND


# ---- the C ABI -----------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_bound():
    import ctypes
    from safeopt_amd import _hip
    from safeopt_amd.build import build
    header = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    exported = ctypes.CDLL(build())
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(exported, name), "libsafeopt_hip.so lacks " + name
        assert name in _hip.PROTOTYPES, name
        assert getattr(_hip.lib(), name).argtypes == _hip.PROTOTYPES[name][1], name
    assert _hip.PROTOTYPES["sgp_grid_rank1_reweigh"] == _hip.PROTOTYPES["sgp_grid_rank1_update"]


def test_without_a_device_they_raise():
    """No device: creating the context raises ``HipError``, as for every other entry point."""
    from safeopt_amd import _hip
    if _hip.device_count() > 0:
        pytest.skip("a GPU is present")
    import safeopt_amd.gpy as gpy
    with pytest.raises(_hip.HipError):
        gpy.models.GPRegression(np.zeros((2, 1)), np.zeros((2, 1)), gpy.kern.RBF(1),
                                noise_var=0.01, noise_scale=[1.0, 2.0])
