"""A long-double GP with a NOISE VECTOR and the case tables of the per-observation-noise tests
(tests/test_reweigh_cpu.py, tests/test_pooling_cpu.py, tests/test_gpu_reweigh.py,
tests/test_gpu_pooling.py).

``Ky = K + diag((noise + 1e-8) r_i)``: observation ``i`` has the noise scale ``r_i``.  The
Cholesky factorisation, the substitutions, the kernels and the data generators are those of
tests/_incremental_ref.py.  Every expected value is a REFIT of the changed data from scratch:
this module holds no update formula.
"""
import functools

import numpy as np

import _incremental_ref as I
from _incremental_ref import (  # noqa: F401
    LD, NOISE, PROD_CTX, PROD3, S_EXCLUDE, clip_var, f64, kdiag, make_kernel, single)

ROWS = 200                  # test rows of the factor cases
SCALES = (1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0, 2.0, 4.0)

#: the three kernels of the tables: name -> (spec, d)
KERNELS = {"rbf_d1": (single("RBF", 1), 1), "mat52_d2": (single("Matern52", 2), 2),
           "prodctx_d3": (PROD_CTX, 3)}


class ScaledGP(object):
    """Exact GP regression with per-observation noise, zero mean, in long double: a fit."""

    def __init__(self, spec, X, Y, r=None, noise=NOISE):
        self.spec, self.noise = spec, LD(noise)
        self.X = np.array(X, dtype=LD).reshape(len(X), -1)
        self.Y = np.array(Y, dtype=LD).reshape(-1)
        n = self.X.shape[0]
        self.r = np.ones(n, dtype=LD) if r is None else np.array(r, dtype=LD).reshape(n)
        K = I.kern(spec, self.X, self.X)
        K[np.diag_indices(n)] += (self.noise + LD(1e-8)) * self.r
        self.L = I.cholesky(K)
        self.z = I.forward(self.L, self.Y)

    n = property(lambda self: self.X.shape[0])

    def alpha(self):
        return I.backward_t(self.L, self.z)

    def Linv(self):
        return I.forward(self.L, np.eye(self.n, dtype=LD))

    def predict(self, rows):
        """Posterior mean and variance (not clipped) at ``rows``."""
        V = I.forward(self.L, I.kern(self.spec, self.X, rows))
        return self.z @ V, LD(kdiag(self.spec)) - (V * V).sum(0)

    def log_likelihood(self):
        """log N(Y; 0, Ky)."""
        return (-LD(0.5) * (self.z @ self.z) - np.log(np.diag(self.L)).sum()
                - LD(0.5) * self.n * np.log(LD(2) * LD(np.pi)))


def snapshot(spec, X, Y, r, Xs, want_linv=True):
    """The refit of ``(X, Y, r)``: what the device GP must hold after whatever led there."""
    gp = ScaledGP(spec, X, Y, r)
    m, v = gp.predict(Xs)
    out = {"n": gp.n, "alpha": f64(gp.alpha()), "mean": f64(m), "var": clip_var(v),
           "X": f64(gp.X), "Y": f64(gp.Y), "r": f64(gp.r)}
    if want_linv:
        out["Linv"] = f64(gp.Linv())
    return out


def _rng(name):
    return np.random.default_rng(I._seed("reweigh" + name))


def case_data(name, d, n, extra=0):
    """(X, Y, scales, test rows, extra rows, their targets, their scales) of a case: the data
    of tests/_incremental_ref.py, scales drawn from SCALES."""
    X, Y, Xs, E, YE = I.data(name, d, n, extra=extra)
    rng = _rng(name)
    return (X, Y, rng.choice(SCALES, size=n), Xs[:ROWS], E, YE, rng.choice(SCALES, size=extra))


# ---------------------------------------------------------------------------------------
# scaled fits: set_data_w -> append_w -> append_block_w (3 rows) -> remove -> pop
# ---------------------------------------------------------------------------------------
FIT_N = (1, 5, 33, 65, 130, 300)
FIT_CASES = {"%s_n%d" % (k, n): (KERNELS[k][0], KERNELS[k][1], n)
             for k in sorted(KERNELS) for n in FIT_N}
FIT_BLOCK = 3


def fit_script(n):
    """The calls of a chain and the row a removal takes (the middle of the grown data)."""
    return (("set", None), ("append", None), ("block", None), ("remove", (n + 1 + FIT_BLOCK) // 2),
            ("pop", None))


@functools.lru_cache(maxsize=None)
def fit_reference(name):
    """``(X, Y, r, Xs, E, YE, rE, snapshots)``: the refit after every call of the chain."""
    spec, d, n = FIT_CASES[name]
    X, Y, r, Xs, E, YE, rE = case_data(name, d, n, extra=1 + FIT_BLOCK)
    cx, cy, cr = X, Y, r
    snaps = []
    for what, row in fit_script(n):
        if what == "append":
            cx, cy, cr = np.vstack([cx, E[:1]]), np.append(cy, YE[0]), np.append(cr, rE[0])
        elif what == "block":
            cx, cy, cr = np.vstack([cx, E[1:]]), np.append(cy, YE[1:]), np.append(cr, rE[1:])
        elif what == "remove":
            keep = np.arange(len(cy)) != row
            cx, cy, cr = cx[keep], cy[keep], cr[keep]
        elif what == "pop":
            cx, cy, cr = cx[:-1], cy[:-1], cr[:-1]
        snaps.append(snapshot(spec, cx, cy, cr, Xs))
    return X, Y, r, Xs, E, YE, rE, snaps


# ---------------------------------------------------------------------------------------
# reweigh: i first / middle / last at every n; the kinds of change and the kernels cycle
# ---------------------------------------------------------------------------------------
REWEIGH_N = (2, 33, 65, 130, 300)
MODES = ("less_noise", "more_noise", "scale_only", "value_only")


def _reweigh_cases():
    out, c = {}, 0
    kernels = sorted(KERNELS)
    for n in REWEIGH_N:
        for where, i in (("first", 0), ("mid", n // 2), ("last", n - 1)):
            k = kernels[(c + c // 3) % 3]          # (every kernel meets every position)
            mode = MODES[c % 4]
            out["%s_n%d_%s_%s" % (k, n, where, mode)] = (KERNELS[k][0], KERNELS[k][1], n, i, mode)
            c += 1
    return out


REWEIGH_CASES = _reweigh_cases()


def reweigh_change(name):
    """``(X, Y, r, Xs, i, y_new, r_new)`` of a case.  less_noise: delta < 0 (a scale of at
    least 1 drops to 1/16), more_noise: delta > 0 (at most 1/4 rises to 4); both with a new
    value.  scale_only:
    the value stays (dy = 0); value_only: the scale stays (delta = 0)."""
    spec, d, n, i, mode = REWEIGH_CASES[name]
    X, Y, r, Xs, _, _, _ = case_data(name, d, n)
    rng = _rng(name + "change")
    y_new = Y[i] + rng.uniform(0.2, 0.5) * (1 if rng.uniform() < 0.5 else -1)
    if mode == "less_noise":
        r[i] = max(r[i], 1.0)
        r_new = 1 / 16
    elif mode == "more_noise":
        r[i] = min(r[i], 0.25)
        r_new = 4.0
    elif mode == "scale_only":
        r_new, y_new = (4.0 if r[i] < 1 else 1 / 8), Y[i]
    else:
        r_new = r[i]
    return X, Y, r, Xs, i, float(y_new), float(r_new)


@functools.lru_cache(maxsize=None)
def reweigh_reference(name):
    """``(X, Y, r, Xs, i, y_new, r_new, before, after)``: the refits before and after."""
    spec = REWEIGH_CASES[name][0]
    X, Y, r, Xs, i, y_new, r_new = reweigh_change(name)
    Y2, r2 = Y.copy(), r.copy()
    Y2[i], r2[i] = y_new, r_new
    return (X, Y, r, Xs, i, y_new, r_new, snapshot(spec, X, Y, r, Xs),
            snapshot(spec, X, Y2, r2, Xs))


#: reweigh -> append -> reweigh -> remove -> pop on 40 rows of the product kernel
CHAIN_SPEC, CHAIN_D, CHAIN_N = PROD_CTX, 3, 40
CHAIN = (("reweigh", 7, 0.25, 0.3), ("append", None, 2.0, None), ("reweigh", 40, 1 / 8, -0.2),
         ("remove", 11, None, None), ("pop", None, None, None))


@functools.lru_cache(maxsize=None)
def chain_reference():
    """``(X, Y, r, Xs, E, YE, snapshots)`` of CHAIN: (what, row, scale, dy) per call."""
    X, Y, r, Xs, E, YE, _ = case_data("chain", CHAIN_D, CHAIN_N, extra=1)
    cx, cy, cr = X.copy(), Y.copy(), r.copy()
    snaps = []
    for what, row, scale, dy in CHAIN:
        if what == "reweigh":
            cy, cr = cy.copy(), cr.copy()
            cy[row] += dy
            cr[row] = scale
        elif what == "append":
            cx, cy, cr = np.vstack([cx, E[:1]]), np.append(cy, YE[0]), np.append(cr, scale)
        elif what == "remove":
            keep = np.arange(len(cy)) != row
            cx, cy, cr = cx[keep], cy[keep], cr[keep]
        else:
            cx, cy, cr = cx[:-1], cy[:-1], cr[:-1]
        snaps.append(snapshot(CHAIN_SPEC, cx, cy, cr, Xs))
    return X, Y, r, Xs, E, YE, snaps
