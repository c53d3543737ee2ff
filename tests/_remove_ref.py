"""The reference of the removal tests (tests/test_remove_cpu.py, tests/test_gpu_remove.py).

Two things, next to the long-double GP of tests/_incremental_ref.py (imported, not edited):

* the TRUTH of a removal: a long-double refit of the data without the row, its L^-1, alpha
  and posterior, and the record the removal has to leave -- w = Ky_new^-1 k(X_new, x_i),
  alpha_i = (y_i - mu_new(x_i)) / s2 and P_ii = 1 / s2 with s2 = k(x_i, x_i) + noise + 1e-8
  - k^T w, all from the REDUCED GP (the Schur complement of row i);
* a float64 NumPy restatement of the downdate: the algorithm,
  not the device code.  Run on a float64 fit it says what error to expect of a float64
  implementation, case by case.
"""
import functools

import numpy as np

from _gpu_common import smooth
from _incremental_ref import (  # noqa: F401
    LD, NOISE, PROD3, PROD_CTX, RefGP, S_EXCLUDE, _quantile_cut, _seed, clip_var, data, f64,
    kdiag, kern, lengthscales, make_kernel, single)

ROWS = 200                  # test rows of the factor cases


def linv_ld(L):
    """L^-1 of a lower-triangular long-double matrix, column by column of the forward
    substitution, touching the lower triangle only (n^3 / 3 operations)."""
    n = L.shape[0]
    V = np.zeros((n, n), dtype=LD)
    for j in range(n):
        V[j, j] = LD(1)
        V[j, :j + 1] /= L[j, j]
        V[j + 1:, :j + 1] -= L[j + 1:, j][:, None] * V[j, :j + 1][None, :]
    return V


# ---------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------
def downdate_f64(M, alpha, i):
    """Items 1-3 on a dense M = L^-1 (n, n) and alpha (n): ``(M_new, alpha_new, w, alpha_i,
    P_ii)``.  The rotations fold c_k into c_i for k = i+1 .. n-1; row k is touched in its
    columns 0 .. k only, so the strict upper triangle of the result is zero by construction."""
    M = np.array(M, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    n = M.shape[0]
    c = M[:, i].copy()
    P = float(c[i:] @ c[i:])
    p = M.T @ c
    keep = np.arange(n) != i
    w = -p[keep] / P
    alpha_new = alpha[keep] + w * alpha[i]
    rho = M[i].copy()                     # zero behind column i
    g0 = c[i]
    for k in range(i + 1, n):
        g1 = np.sqrt(g0 * g0 + c[k] * c[k])
        cs, sn = g0 / g1, c[k] / g1
        rk = M[k, :k + 1].copy()
        M[k, :k + 1] = -sn * rho[:k + 1] + cs * rk
        rho[:k + 1] = cs * rho[:k + 1] + sn * rk
        g0 = g1
    return M[np.ix_(keep, keep)], alpha_new, w, float(alpha[i]), P


def fit_f64(spec, X, Y, noise=NOISE):
    """L^-1 and alpha of a float64 fit (LAPACK): the input of the restatement."""
    K = f64(kern(spec, X, X))
    K[np.diag_indices(len(X))] += noise + 1e-8
    L = np.linalg.cholesky(K)
    M = np.linalg.inv(L)
    M[np.triu_indices(len(X), 1)] = 0.0
    return M, M.T @ (M @ np.asarray(Y, dtype=np.float64))


# ---------------------------------------------------------------------------------------
# factor cases: name -> (kernel spec, d, n, i)
# ---------------------------------------------------------------------------------------
FACTOR_CASES = {
    "rbf_d1_n2_i0": (single("RBF", 1), 1, 2, 0),                 # smallest legal n
    "mat52_d3_n17_i0": (single("Matern52", 3), 3, 17, 0),        # n_pad 32 -> 16
    "prod_d3_n17_i8": (PROD3, 3, 17, 8),
    "rbf_d8_n17_i16": (single("RBF", 8), 8, 17, 16),             # the last row: no rotation
    "mat52_d1_n33_i5": (single("Matern52", 1), 1, 33, 5),        # n_f 64 -> 32
    "prod_d3_n49_i48": (PROD3, 3, 49, 48),
    "rbf_d3_n130_i64": (single("RBF", 3), 3, 130, 64),
    "mat52_d8_n600_i0": (single("Matern52", 8), 8, 600, 0),      # the recurrence at full length
    "mat52_d3_n1100_i3": (single("Matern52", 3), 3, 1100, 3),    # more columns than 1024
}


def truth(gp_new, x_i, y_i, rows=None):
    """What a removal has to leave, from the long-double GP of the REDUCED data."""
    spec = gp_new.spec
    k = kern(spec, gp_new.X, np.asarray(x_i, dtype=LD).reshape(1, -1))[:, 0]
    w = gp_new.solve(k)
    s2 = LD(kdiag(spec)) + gp_new.noise + LD(1e-8) - k @ w
    alpha = gp_new.alpha()
    out = {"n": gp_new.n, "alpha": f64(alpha), "w": f64(w), "P_ii": float(1 / s2),
           "alpha_i": float((LD(y_i) - k @ alpha) / s2)}
    if rows is not None:
        m, v = gp_new.predict(rows)
        out["mean"], out["var"] = f64(m), clip_var(v)
    return out


@functools.lru_cache(maxsize=None)
def factor_reference(name):
    """``(X, Y, rows, truth)`` of a factor case; the truth includes ``Linv``."""
    spec, d, n, i = FACTOR_CASES[name]
    X, Y, Xs, _, _ = data(name, d, n)
    Xs = Xs[:ROWS]
    keep = np.arange(n) != i
    gp = RefGP(spec, X[keep], Y[keep])
    t = truth(gp, X[i], Y[i], Xs)
    t["Linv"] = f64(linv_ld(gp.L))
    return X, Y, Xs, t


def restatement_errors(name):
    """Errors of the float64 restatement against the long-double refit of a factor case:
    dict of L^-1 (absolute), alpha (relative to max |alpha|), w (relative to max |w|),
    alpha_i (relative to max |alpha|) and P_ii (relative), plus the result itself."""
    spec, d, n, i = FACTOR_CASES[name]
    X, Y, _, t = factor_reference(name)
    M, alpha = fit_f64(spec, X, Y)
    Mn, an, w, ai, P = downdate_f64(M, alpha, i)
    sa = np.max(np.abs(t["alpha"]))
    return {"Linv": float(np.max(np.abs(Mn - t["Linv"]))),
            "alpha": float(np.max(np.abs(an - t["alpha"])) / sa),
            "w": float(np.max(np.abs(w - t["w"])) / max(np.max(np.abs(t["w"])), 1e-300)),
            "alpha_i": abs(ai - t["alpha_i"]) / sa,
            "P_ii": abs(P - t["P_ii"]) / t["P_ii"],
            "result": (Mn, an, w, ai, P)}


# ---------------------------------------------------------------------------------------
# chains: fit 40 rows, then a script of calls; a snapshot of the refit after every call
# ---------------------------------------------------------------------------------------
CHAIN_SPEC, CHAIN_D, CHAIN_N = single("Matern52", 2), 2, 40
#: ("remove", row) | ("append", None) | ("pop", None)
CHAINS = {
    "remove_append_pop": (("remove", 11), ("append", None), ("pop", None)),
    "remove_twice": (("remove", 0), ("remove", 37)),
}


def _snapshot(gp, Xs):
    m, v = gp.predict(Xs)
    return {"n": gp.n, "alpha": f64(gp.alpha()), "mean": f64(m), "var": clip_var(v),
            "Linv": f64(linv_ld(gp.L))}


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    """``(X, Y, rows, extra rows, their targets, [snapshot per call])``."""
    X, Y, Xs, E, YE = data("chain_" + name, CHAIN_D, CHAIN_N, extra=2)
    Xs = Xs[:ROWS]
    Xc, Yc, e, out = X.copy(), Y.copy(), 0, []
    for what, row in CHAINS[name]:
        if what == "remove":
            Xc, Yc = np.delete(Xc, row, axis=0), np.delete(Yc, row)
        elif what == "append":
            Xc, Yc = np.vstack([Xc, E[e]]), np.append(Yc, YE[e])
            e += 1
        else:
            Xc, Yc = Xc[:-1], Yc[:-1]
        out.append(_snapshot(RefGP(CHAIN_SPEC, Xc, Yc), Xs))
    return X, Y, Xs, E, YE, out


#: append past the old n after a removal: fit 12 rows (128 are reserved), remove row 4, then
#: one-row appends to 14 rows -- the capacity of the fit is kept, none of them refits
GROW = (single("RBF", 2), 2, 12, 4, 3)


@functools.lru_cache(maxsize=None)
def grow_reference():
    spec, d, n, row, more = GROW
    X, Y, Xs, E, YE = data("grow_after_removal", d, n, extra=more)
    Xs = Xs[:ROWS]
    Xc, Yc = np.delete(X, row, axis=0), np.delete(Y, row)
    out = [_snapshot(RefGP(spec, Xc, Yc), Xs)]
    for e in range(more):
        Xc, Yc = np.vstack([Xc, E[e]]), np.append(Yc, YE[e])
        out.append(_snapshot(RefGP(spec, Xc, Yc), Xs))
    return X, Y, Xs, E, YE, out


def log_likelihood_ld(spec, X, Y, noise=NOISE):
    """log p(y | X) of the long-double GP."""
    gp = RefGP(spec, X, Y, noise)
    return float(-LD(0.5) * (gp.z @ gp.z) - np.log(np.diag(gp.L)).sum()
                 - LD(0.5) * gp.n * np.log(LD(2) * LD(np.pi)))


# ---------------------------------------------------------------------------------------
# grid cases (sgp_grid_rank1_remove), N = 1000 rows
# ---------------------------------------------------------------------------------------
# gps: (kernel spec, data key, n, row to remove or None) per GP -- GPs with the same key have
# the same X; tensor: the rows are a tensor grid (else scattered); steps: consecutive
# removals + refreshes (row `row` every time); share / ctx_col / betas as in RANK1_CASES.
def _g(d, gps, tensor=False, steps=1, share=None, ctx_col=None, betas=(2.0, 3.0)):
    return dict(d=d, gps=gps, tensor=tensor, steps=steps, share=share, ctx_col=ctx_col,
                betas=betas)


_M2 = single("Matern52", 2)
GRID_N = 1000
GRID_CASES = {
    "g1_rbf_d1_tensor_n17": _g(1, [(single("RBF", 1), "a", 17, 8)], tensor=True),
    "g3_one_d3_n200": _g(3, [(single("RBF", 3), "a", 200, None), (PROD3, "b", 200, 77),
                             (single("Matern52", 3), "c", 60, None)]),
    "g3_all_d2_tensor": _g(2, [(single("RBF", 2), "a", 17, 0), (_M2, "b", 200, 199),
                               (single("Matern32", 2), "c", 33, 5)], tensor=True),
    # 700 -> 699 rows: n_pad 704, 704 * 9 = 6336 doubles do not fit k_rank1's LDS stage
    "g1_mat52_d8_n700": _g(8, [(single("Matern52", 8), "a", 700, 350)]),
    "shared_aa_d2": _g(2, [(_M2, "a", 48, 20), (_M2, "a", 48, 20)], share=True),
    "ctx_prod_d3": _g(3, [(PROD_CTX, "a", 45, 7), (PROD_CTX, "a", 45, 7)], ctx_col=0.4),
    # 8 removals from n = 40 in a row, the oldest row every time (a sliding window)
    "streak_mat52_d2": _g(2, [(_M2, "a", 40, 0), (_M2, "a", 40, 0)], steps=8,
                          betas=(2.0,) + tuple(2.2 + 0.1 * t for t in range(8))),
}


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """``pts`` (N, d), ``X`` / ``Y`` per GP before the removals, ``fmin`` (G,), ``kdiag`` and
    per step ``beta``, ``mean`` / ``var`` (G, N) of the long-double refits of the reduced
    data, ``Q`` (N, 2 G), ``S``, ``excluded`` and ``ret`` -- as ``rank1_reference``."""
    c = GRID_CASES[name]
    d, G, N = c["d"], len(c["gps"]), GRID_N
    rng = np.random.default_rng(_seed("remove_" + name))
    dp = d - (1 if c["ctx_col"] is not None else 0)

    def with_ctx(a):
        if c["ctx_col"] is None:
            return a
        return np.hstack([a, np.full((a.shape[0], 1), c["ctx_col"])])

    if c["tensor"]:
        side = {1: (1000,), 2: (40, 25)}[dp]
        axes = [np.linspace(-3, 3, s) for s in side]
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(N, dp)
    else:
        pts = rng.uniform(-3, 3, size=(N, dp))
    pts = with_ctx(pts)
    Xd = {}
    for _, key, n, _ in c["gps"]:
        if key not in Xd or Xd[key].shape[0] < n:
            Xd[key] = with_ctx(np.random.default_rng(_seed(name + key)).uniform(-2, 2, (n, dp)))
    Xg = [Xd[key][:n].copy() for _, key, n, _ in c["gps"]]
    Yg = [smooth(X, 11 + g)[:, 0] + 0.3 for g, X in enumerate(Xg)]
    if not c["tensor"]:
        # the row that leaves (first step), a row that stays and a row far away are on the grid
        g0 = [g for g in range(G) if c["gps"][g][3] is not None][0]
        pts[N // 2] = Xg[g0][c["gps"][g0][3]]
        pts[0] = Xg[g0][(c["gps"][g0][3] + 1) % len(Xg[g0])]
        far = np.r_[np.full(dp, 60.0), np.zeros(d - dp)]
        pts[1] = pts[N // 2] + far
    kd = [kdiag(spec) for spec, _, _, _ in c["gps"]]
    Xc, Yc = [X.copy() for X in Xg], [Y.copy() for Y in Yg]
    steps = []
    for t in range(c["steps"]):
        mean, var = [], []
        for g, (spec, _, _, row) in enumerate(c["gps"]):
            if row is not None:
                Xc[g], Yc[g] = np.delete(Xc[g], row, axis=0), np.delete(Yc[g], row)
            m, v = RefGP(spec, Xc[g], Yc[g]).predict(pts)
            mean.append(f64(m))
            var.append(clip_var(v))
        steps.append({"beta": c["betas"][1 + t], "mean": np.array(mean), "var": np.array(var)})

    def bounds(st):
        sd = np.sqrt(st["var"])
        return st["mean"] - st["beta"] * sd, st["mean"] + st["beta"] * sd

    lo1 = bounds(steps[0])[0]
    fmin = np.array([_quantile_cut(lo1[g], 1.0 - 0.6 ** (1.0 / G)) for g in range(G)])
    for st in steps:
        lo, up = bounds(st)
        st["Q"] = np.stack([lo, up], axis=2).transpose(1, 0, 2).reshape(N, 2 * G)
        st["S"] = np.all(lo > fmin[:, None], axis=0)
        st["excluded"] = np.any(np.abs(lo - fmin[:, None]) < S_EXCLUDE, axis=0)
        st["ret"] = (float(np.max(lo[0][st["S"]])), True) if st["S"].any() else (-np.inf, False)
    return {"pts": pts, "X": Xg, "Y": Yg, "fmin": fmin, "steps": steps, "kdiag": kd,
            "beta0": c["betas"][0]}
