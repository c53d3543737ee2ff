"""The expander test (gp_opt.py:579-606) as a MARGIN per candidate, and the case matrix of
tests/test_gpu_expander_flags.py.

``son.expander_hits_rank1`` answers "does candidate c lift some unsafe row above fmin_i"; a test
that compares flags needs to know how far from the threshold the answer is.  So

    best[c] = max over the unsafe rows of ( mu2 - beta sqrt(var2) - fmin_i )

in the arithmetic of ``expander_hits_rank1`` (float64, BLAS, chunked: ``margins``), the same in
``np.longdouble`` with an explicit elimination and the kernels evaluated from the differences of
the coordinates (``margins_longdouble``: no LAPACK, no expanded-form distance -- small shapes
only), and the Lipschitz counterpart (``lipschitz_margins``).

The cases (``CASES``) are built from the oracle alone, so that the CPU suite checks what the GPU
module relies on: that nearly every (candidate, GP) entry is decided and that both answers occur
(tests/test_expander_ref.py).  Not a conftest: imported by the two test modules.
"""
import functools

import numpy as np
from scipy.spatial.distance import cdist

from oracle import gp_numpy as gpn

BETA = 2.0
NOISE = 0.05 ** 2


# ---------------------------------------------------------------------------------------------
# margins
# ---------------------------------------------------------------------------------------------
def margins(gp, U, xc, u_c, beta, fmin_i, chunk=512, rows=False):
    """``(best, arg)``: per candidate the largest ``l2 - fmin_i`` over the unsafe rows ``U`` and
    the row (index into ``U``) that attains it; ``best >= 0`` is ``expander_hits_rank1``.  No
    unsafe row: ``best = -inf``, ``arg = -1`` (``np.any([])`` is False).  ``rows``: also the
    largest margin per unsafe row over the candidates."""
    U = np.atleast_2d(np.asarray(U, dtype=float))
    xc = np.atleast_2d(np.asarray(xc, dtype=float))
    u_c = np.asarray(u_c, dtype=float).reshape(-1)
    K = xc.shape[0]
    best = np.full(K, -np.inf)
    arg = np.full(K, -1, dtype=np.int64)
    row_best = np.full(U.shape[0], -np.inf)
    if U.shape[0] == 0:
        return (best, arg, row_best) if rows else (best, arg)
    Wi, alpha = gp.woodbury_inv, gp.woodbury_vector[:, 0]
    KUX = gp.kern.K(U, gp.X)
    mean = KUX.dot(alpha)
    var = gp.kern.Kdiag(U) - np.einsum('ij,ij->i', KUX.dot(Wi), KUX)
    for a in range(0, K, chunk):
        xb = xc[a:a + chunk]
        KcX = gp.kern.K(gp.X, xb)
        W = Wi.dot(KcX)
        var_c = gp.kern.Kdiag(xb) - np.sum(KcX * W, axis=0)
        mu_c = KcX.T.dot(alpha)
        s2 = var_c + gp.noise_var + 1e-8
        C = gp.kern.K(U, xb) - KUX.dot(W)
        mean2 = mean[:, None] + C * ((u_c[a:a + chunk] - mu_c) / s2)[None, :]
        var2 = np.clip(var[:, None] - C * C / s2[None, :], 1e-15, np.inf)
        marg = mean2 - beta * np.sqrt(var2) - fmin_i
        arg[a:a + chunk] = marg.argmax(axis=0)
        best[a:a + chunk] = marg.max(axis=0)
        if rows:
            row_best = np.maximum(row_best, marg.max(axis=1))
    return (best, arg, row_best) if rows else (best, arg)


LD = np.longdouble


def kern_longdouble(kern, A, B):
    """``kern.K(A, B)`` in long double from the coordinate differences (no expanded form)."""
    if isinstance(kern, gpn.Prod):
        out = None
        for p in kern.parts:
            k = kern_longdouble(p, A, B)
            out = k if out is None else out * k
        return out
    A = np.asarray(A, dtype=LD)[:, kern.active_dims]
    B = np.asarray(B, dtype=LD)[:, kern.active_dims]
    ls = np.asarray(kern.lengthscale, dtype=LD) * np.ones(A.shape[1], dtype=LD)
    r2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        diff = (A[:, k][:, None] - B[:, k][None, :]) / ls[k]
        r2 += diff * diff
    v = LD(kern.variance[0])
    if isinstance(kern, gpn.RBF):
        return v * np.exp(-r2 / LD(2))
    r = np.sqrt(r2)
    if isinstance(kern, gpn.Matern32):
        s3 = np.sqrt(LD(3))
        return v * (1 + s3 * r) * np.exp(-s3 * r)
    assert isinstance(kern, gpn.Matern52)
    s5 = np.sqrt(LD(5))
    return v * (1 + s5 * r + LD(5) / LD(3) * r2) * np.exp(-s5 * r)


def solve_longdouble(A, B):
    """``A^-1 B`` by Gauss-Jordan elimination with partial pivoting in long double."""
    n = A.shape[0]
    T = np.concatenate([np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)], axis=1)
    for c in range(n):
        pv = c + int(np.argmax(np.abs(T[c:, c])))
        if pv != c:
            T[[c, pv]] = T[[pv, c]]
        T[c] /= T[c, c]
        f = T[:, c].copy()
        f[c] = 0
        T -= f[:, None] * T[c][None, :]
    return T[:, n:]


def margins_longdouble(gp, U, xc, u_c, beta, fmin_i):
    """``margins`` in ``np.longdouble`` (returned as long double): O(n^2 (n + Nu + K)) in
    software arithmetic -- for the small shapes."""
    U = np.atleast_2d(np.asarray(U, dtype=float))
    xc = np.atleast_2d(np.asarray(xc, dtype=float))
    K = xc.shape[0]
    if U.shape[0] == 0:
        return np.full(K, -np.inf, dtype=LD), np.full(K, -1, dtype=np.int64)
    n = gp.X.shape[0]
    Ky = kern_longdouble(gp.kern, gp.X, gp.X) + (LD(gp.noise_var) + LD(1e-8)) * np.eye(n, dtype=LD)
    KXU = kern_longdouble(gp.kern, gp.X, U)                       # (n, Nu)
    KXc = kern_longdouble(gp.kern, gp.X, xc)                      # (n, K)
    sol = solve_longdouble(Ky, np.concatenate([np.asarray(gp.Y, dtype=LD), KXU, KXc], axis=1))
    alpha, WU, Wc = sol[:, 0], sol[:, 1:1 + U.shape[0]], sol[:, 1 + U.shape[0]:]
    kdiag = LD(gp.kern.Kdiag(U[:1])[0])
    mean = KXU.T.dot(alpha)
    var = kdiag - np.sum(KXU * WU, axis=0)
    var_c = kdiag - np.sum(KXc * Wc, axis=0)
    mu_c = KXc.T.dot(alpha)
    s2 = var_c + LD(gp.noise_var) + LD(1e-8)
    C = kern_longdouble(gp.kern, U, xc) - KXU.T.dot(Wc)
    mean2 = mean[:, None] + C * ((np.asarray(u_c, dtype=LD).reshape(-1) - mu_c) / s2)[None, :]
    var2 = np.maximum(var[:, None] - C * C / s2[None, :], LD(1e-15))
    marg = mean2 - LD(beta) * np.sqrt(var2) - LD(fmin_i)
    return marg.max(axis=0), marg.argmax(axis=0)


def lipschitz_margins(U, xc, u_c, L, fmin, chunk=1024):
    """``best[c, i] = max over the unsafe rows of u_i(x_c) - L_i |x_c - x| - fmin_i``
    (gp_opt.py:558-576, ``cdist``); ``-inf`` without unsafe rows."""
    xc = np.atleast_2d(np.asarray(xc, dtype=float))
    u_c = np.asarray(u_c, dtype=float).reshape(xc.shape[0], -1)
    L, fmin = np.asarray(L, dtype=float), np.asarray(fmin, dtype=float)
    best = np.full(u_c.shape, -np.inf)
    if np.shape(U)[0] == 0:
        return best
    for a in range(0, xc.shape[0], chunk):
        dmin = cdist(xc[a:a + chunk], U).min(axis=1)
        best[a:a + chunk] = u_c[a:a + chunk] - L[None, :] * dmin[:, None] - fmin[None, :]
    return best


# ---------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------
def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


def make_kernel(ns, spec, d, ls_scale):
    """``spec``: a kind (ARD lengthscales 0.5 .. 2.5 times ``ls_scale`` over the columns: a ratio
    of 5) or a list of ``(kind, columns)`` parts of a product (columns may overlap)."""
    if isinstance(spec, str):
        ls = np.geomspace(0.5, 2.5, d) * ls_scale if d > 1 else np.array([1.0 * ls_scale])
        return getattr(ns, spec)(d, variance=1.7, lengthscale=ls, ARD=True)
    k = None
    for j, (kind, cols) in enumerate(spec):
        ls = np.geomspace(0.6, 3.0, len(cols))[::(-1) ** j] * ls_scale
        part = getattr(ns, kind)(len(cols), variance=1.3 - 0.4 * j, lengthscale=ls, ARD=True,
                                 active_dims=list(cols))
        k = part if k is None else k * part
    return k


def tensor_points(sides, lo=-3.0, hi=3.0):
    """Rows of a tensor grid in the order of ``linearly_spaced_combinations``."""
    axes = [np.linspace(lo, hi, s) for s in sides]
    return np.ascontiguousarray(np.stack(np.meshgrid(*axes, indexing='ij'), axis=-1)
                                .reshape(-1, len(sides)))


# name -> what varies.  ``q``: fmin_i is the q-quantile of GP i's lower bound over the rows (None:
# -inf, the GP has no constraint); ``pool``: candidates (safe rows first, then ``off`` points off the
# grid); ``Ks``: the prefixes of the pool that go through pass_test; ``small``: long double too;
# ``walk``: every safe row is a candidate of the device's own selections (expander_batch,
# expander_pass mode 1, expanders_small_all).
CASES = {
    # one observation, one column; ragged groups and the supergroup boundary (128 | 129)
    "rbf_d1_n1": dict(kind="RBF", d=1, ns=[1], N=1007, q=[0.45], pool=129,
                      Ks=[1, 15, 16, 17, 128, 129], small=True, walk=True, ls=1.0, gap=0.03, lip=[0.8]),
    # a tensor grid (set_axes), n = 16: one full row block
    "m32_d2_n16_grid": dict(kind="Matern32", d=2, ns=[16], sides=(33, 31), q=[0.2], pool=129,
                            Ks=[17, 129], small=True, walk=True, ls=0.5),
    # three GPs, the middle one without a constraint; n = 17 / 48: ragged row blocks
    "m52_d3_g3_inf": dict(kind="Matern52", d=3, ns=[17, 17, 48], N=1007, q=[0.5, None, 0.4],
                          pool=128, Ks=[16, 128], small=True, walk=True, ls=1.5, gap=0.1, special=True,
                          lip=[0.5, 0.5, 0.5]),
    # GPs of different sizes in one launch: np_max / ldk against each GP's own n_pad
    "rbf_d5_mixed_n": dict(kind="RBF", d=5, ns=[40, 300, 17], N=1007, q=[0.5, 0.5, 0.5], pool=129,
                           Ks=[129], small=False, walk=True, ls=2.0, gap=0.1),
    # a product of two parts on overlapping columns: no block test; n = 49
    "prod_d3_n49": dict(kind=[("RBF", (0, 1)), ("Matern52", (1, 2))], d=3, ns=[49], N=1007,
                        q=[0.5], pool=129, Ks=[15, 129], small=True, walk=True, ls=1.0, gap=0.3,
                        special=True),
    # d = 8, n = 256: the last n_pad of the row-level block test
    "m52_d8_n256": dict(kind="Matern52", d=8, ns=[256], N=1007, q=[0.5], pool=129, Ks=[129],
                        small=False, walk=True, ls=3.0, gap=0.3),
    # n = 257 on a tensor grid: the pair test; 528 candidates = more than one MODE-2 chunk
    "rbf_d2_n257_grid": dict(kind="RBF", d=2, ns=[257], sides=(64, 63), q=[0.5], pool=528,
                             Ks=[528], small=False, walk=True, ls=1.0, lip=[1.0]),
    "m32_d3_n272": dict(kind="Matern32", d=3, ns=[272], N=2003, q=[0.5], pool=528, Ks=[528],
                        small=False, walk=False, ls=1.5, gap=0.03),
    # all rows unsafe but one: that row and points off the grid are the candidates
    "rbf_d2_one_safe": dict(kind="RBF", d=2, ns=[48], N=1007, q=["one"], pool=1, off=63,
                            Ks=[64], small=True, walk=True, ls=1.0),
    # N = 1: one unsafe row, candidates off the grid
    "m32_d1_one_row": dict(kind="Matern32", d=1, ns=[16], N=1, q=["none"], pool=0, off=33,
                           Ks=[33], small=True, walk=False, ls=1.0, off_near=True),
    # ... and with a product kernel (no block test: the pair test decides) and n = 272 (the pair
    # test behind the block test): a single listed row, nothing else keeps its blocks alive
    "prod_d3_one_row": dict(kind=[("RBF", (0, 1)), ("Matern52", (1, 2))], d=3, ns=[49], N=1,
                            q=["none"], pool=0, off=33, Ks=[33], small=True, walk=False, ls=1.0,
                            off_near=True),
    "m52_d2_n272_one_row": dict(kind="Matern52", d=2, ns=[272], N=1, q=["none"], pool=0, off=33,
                                Ks=[33], small=False, walk=False, ls=1.0, off_near=True),
    # MODE 1 beyond the one-item-per-workgroup form: 4100 candidates, n = 520, 40 000 rows
    "m52_d2_n520_big": dict(kind="Matern52", d=2, ns=[520], sides=(200, 200), q=[0.5],
                            pool=4100, Ks=[4100], small=False, walk=False, ls=0.7),
}


class Case(object):
    pass


def _lower_bounds(gos, pts):
    """(mean, var, mean - beta sd), each (G, N), of the oracle GPs at ``pts``."""
    mean = np.empty((len(gos), pts.shape[0]))
    var = np.empty_like(mean)
    for i, go in enumerate(gos):
        m, v = go.predict_noiseless(pts)
        mean[i], var[i] = m[:, 0], v[:, 0]
    return mean, var, mean - BETA * np.sqrt(var)


def _rows_with_a_gap(cfg, gos, pts, N):
    """``(rows, fmin)`` of an unstructured case with a ``gap``: N of the rows ``pts`` and the
    thresholds (NaN where the quantile is not a number) they were chosen around.

    Unstructured rows are ours to choose: none within ``gap`` below fmin_i.  (Among a thousand rows
    some lie within 1e-4 of any threshold, and nearly every candidate lifts one of THOSE across it:
    every flag would be a hit.)  And a row is below EVERY threshold or above every one: a row that
    only another GP makes unsafe is above fmin_i before any candidate is added, a hit for all."""
    lower = _lower_bounds(gos, pts)[2]
    fq = np.full(len(gos), np.nan)
    above = np.ones(pts.shape[0], dtype=bool)
    below = np.ones(pts.shape[0], dtype=bool)
    for i, q in enumerate(cfg["q"]):
        if isinstance(q, float):
            fq[i] = np.quantile(lower[i], q)
            above &= lower[i] > fq[i]
            below &= lower[i] <= fq[i] - cfg["gap"]
    rows = np.ascontiguousarray(pts[above | below][:N])
    assert rows.shape[0] == N
    return rows, fq


def _thresholds(cfg, lower, fq):
    """fmin per GP from the case's ``q`` (and the thresholds ``fq`` the rows were chosen around)."""
    N = lower.shape[1]
    fmin = np.full(lower.shape[0], -np.inf)
    for i, q in enumerate(cfg["q"]):
        if q is None:
            continue
        srt = np.sort(lower[i])
        if q == "one":                       # only the row with the largest lower bound is safe
            fmin[i] = 0.5 * (srt[-1] + srt[-2])
        elif q == "none":                    # every row is unsafe
            fmin[i] = srt[-1] + 0.002
        elif np.isfinite(fq[i]):             # (rows chosen around it: _rows_with_a_gap)
            fmin[i] = fq[i]
        else:                                # in the widest gap between two rows near the quantile
            k0, w = int(q * N), max(1, N // 32)
            k = k0 - w + 1 + int(np.argmax(np.diff(srt[k0 - w:k0 + w])))
            assert srt[k] - srt[k - 1] > 1e-6
            fmin[i] = 0.5 * (srt[k] + srt[k - 1])
    return fmin


def _candidates(c, cfg, rng):
    """The pool of a case: safe rows, points off the grid, the specials; mu and the value u each
    candidate carries."""
    d, N = c.pts.shape[1], c.pts.shape[0]
    c.rows = np.sort(rng.choice(c.safe_rows, size=min(cfg["pool"], c.safe_rows.size), replace=False))
    off = rng.uniform(-3, 3, size=(cfg.get("off", 0), d))
    if cfg.get("off_near"):                  # ... within a lengthscale of some row
        off = c.pts[rng.integers(N, size=off.shape[0])] + rng.normal(scale=0.3, size=off.shape)
    if cfg.get("special"):                   # a training point | an unsafe row | 50 lengthscales away
        far = np.full((1, d), 3.0 + 50.0 * 3.0 * cfg["ls"])
        off = np.concatenate([off, c.X[0][:1], c.pts[~c.S][:1], far])
    c.n_special = 3 if cfg.get("special") else 0
    c.xc = np.concatenate([c.pts[c.rows], off])
    c.mu_c, var_c, _ = [a.T for a in _lower_bounds(c.gos, c.xc)]
    # The kernels take u - mu as an operand.  With few observations nearly every safe row lifts
    # SOME row that lies just below fmin, so every other candidate of the pool carries a value
    # between the lower bound and the middle of its interval instead of its upper bound: the
    # observation then pulls its neighbours down and both answers occur in every case.
    t = np.where(np.arange(c.xc.shape[0]) % 2 == 1, rng.uniform(-1.5, 0.5, size=c.xc.shape[0]), 1.0)
    if c.n_special:
        t[-c.n_special:] = 1.0
    c.u_c = c.mu_c + t[:, None] * BETA * np.sqrt(var_c)
    assert c.xc.shape[0] >= max(cfg["Ks"]), (c.name, c.xc.shape[0], c.safe_rows.size)
    c.Ks = sorted(set(cfg["Ks"]) | {c.xc.shape[0]})


def safe_row_margins(c, mean, var):
    """Margins (|S|, G) of EVERY safe row as a candidate carrying its upper bound
    ``mean + beta sqrt(var)`` (``mean`` / ``var``: (G, N), the oracle's or the device's)."""
    best = np.full((c.safe_rows.size, c.G), -np.inf)
    for i in np.flatnonzero(c.active):
        u = mean[i, c.safe_rows] + BETA * np.sqrt(var[i, c.safe_rows])
        best[:, i], _ = margins(c.gos[i], c.U, c.pts[c.safe_rows], u, BETA, c.fmin[i])
    return best


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The problem of a case from the oracle alone (cached: shared, never modified)."""
    cfg = CASES[name]
    c = Case()
    c.name, c.cfg = name, cfg
    d, ns = cfg["d"], cfg["ns"]
    seed = sum(ord(ch) for ch in name)
    rng = np.random.default_rng(seed)
    c.axes_sides = cfg.get("sides")
    c.pts = (tensor_points(c.axes_sides) if c.axes_sides
             else rng.uniform(-3, 3, size=(cfg["N"] * (16 if cfg.get("gap") else 1), d)))
    c.G = len(ns)
    c.X = [rng.uniform(-2.5, 2.5, size=(n, d)) for n in ns]
    c.Y = [_smooth(X, seed + 5 + i) + 0.3 + 0.05 * rng.normal(size=(X.shape[0], 1))
           for i, X in enumerate(c.X)]
    c.kernel = lambda nsp: make_kernel(nsp, cfg["kind"], d, cfg["ls"])
    c.gos = [gpn.GPRegression(X, Y, c.kernel(gpn), noise_var=NOISE) for X, Y in zip(c.X, c.Y)]
    c.kdiag = float(c.gos[0].kern.Kdiag(c.pts[:1])[0])
    fq = np.full(c.G, np.nan)
    if cfg.get("gap"):
        c.pts, fq = _rows_with_a_gap(cfg, c.gos, c.pts, cfg["N"])
    c.mean, c.var, lower = _lower_bounds(c.gos, c.pts)
    c.fmin = _thresholds(cfg, lower, fq)
    c.active = np.isfinite(c.fmin)
    c.S = np.all(lower.T > c.fmin, axis=1)
    c.safe_rows = np.flatnonzero(c.S)
    c.U = c.pts[~c.S]
    _candidates(c, cfg, rng)
    c.best = np.full((c.xc.shape[0], c.G), -np.inf)
    c.row_best = {}
    for i in np.flatnonzero(c.active):
        c.best[:, i], _, c.row_best[i] = margins(c.gos[i], c.U, c.xc, c.u_c[:, i], BETA, c.fmin[i],
                                                 rows=True)
    # every safe row as a candidate (the device's own selections)
    c.best_safe = safe_row_margins(c, c.mean, c.var) if cfg["walk"] else None
    return c


TIGHT_WANTS = np.array([1e-2, -1e-2, 1e-3, -1e-3, 1e-4, -1e-4, 1e-5, -1e-5, 1e-6, -1e-6,
                        3e-6, -3e-6, 3e-5, -3e-5, 3e-4, -3e-4])


@functools.lru_cache(maxsize=None)
def tight_group(name):
    """``(x (16, d), mu (16), u (16), fmin', best (16))``: a FULL group of candidates that all sit on
    one unsafe row of a one-GP case -- the row closest to fmin -- where the pruning bounds have no
    slack: ``c(x) = var(x) = sd(x) sd(x_c)``, Cauchy-Schwarz with equality.  ``fmin'`` lies
    1.5 beta sd above the row's lower bound, beyond what the smaller variance alone gives, so the
    mean has to rise and u - mu > 0 is what the bound's |delta| c stands for.  The margin of the
    pair is linear in u; the 16 values of u put it at ``TIGHT_WANTS``, and the row itself is the
    arg-max (checked here, from the reference alone)."""
    c = build_case(name)
    assert c.G == 1
    go = c.gos[0]
    lower = (c.mean - BETA * np.sqrt(c.var))[0][~c.S]
    r = int(np.argmax(lower))
    x = c.U[r:r + 1]
    mu, var = [a[0, 0] for a in go.predict_noiseless(x)]
    fmin = lower[r] + 1.5 * BETA * np.sqrt(var)
    m0, a0 = margins(go, c.U, x, [mu], BETA, fmin)
    m1, a1 = margins(go, c.U, x, [mu + 1.0], BETA, fmin)
    u = mu + (TIGHT_WANTS - m0[0]) / (m1[0] - m0[0])
    xs = np.repeat(x, 16, axis=0)
    best, arg = margins(go, c.U, xs, u, BETA, fmin)
    assert np.all(arg == r) and np.all(u > mu)
    assert np.max(np.abs(best - TIGHT_WANTS)) < 1e-9 and np.all(np.abs(best) > band(c))
    return xs, np.full(16, mu), u, np.array([fmin]), best


@functools.lru_cache(maxsize=None)
def discrepancy(name):
    """D of a small case: max |best_float64 - best_longdouble| over its (candidate, active GP)."""
    c = build_case(name)
    assert c.cfg["small"]
    worst = 0.0
    for i in np.flatnonzero(c.active):
        ld, _ = margins_longdouble(c.gos[i], c.U, c.xc, c.u_c[:, i], BETA, c.fmin[i])
        worst = max(worst, float(np.max(np.abs(ld - c.best[:, i].astype(LD)))))
    return worst


SMALL = [k for k, v in CASES.items() if v["small"]]

# The largest D over the small cases, MEASURED on the CPU (tests/test_expander_ref.py asserts that
# the measurement stays below it; profiles/expander_flags/SUMMARY.txt has D per case).
D_MAX = 1e-11


def band(case):
    """|best| above which a flag is asserted: 100 D for the device's third summation order and
    its own exponential, and the floor the full_sets scenario already uses on the device."""
    return max(100.0 * D_MAX, 1e-9 * np.sqrt(case.kdiag))


def decided(case, best):
    """(decided entries, hits among them) of a margin array (K, G): active GPs only."""
    dec = (np.abs(best) > band(case)) & case.active[None, :]
    return dec, (best >= 0) & dec


def shares(case, best=None):
    """(share of the active entries inside the band, share of hits, of non-hits among decided)."""
    best = case.best if best is None else best
    dec, hit = decided(case, best)
    n_act = best.shape[0] * int(case.active.sum())
    n_dec = int(dec.sum())
    return 1.0 - n_dec / n_act, hit.sum() / max(n_dec, 1), (n_dec - hit.sum()) / max(n_dec, 1)


def lipschitz_case(case):
    """``(L, best (K, G), band (K, G))`` of a case with Lipschitz constants ``lip`` times the
    median of (u - fmin) / (distance to the nearest unsafe row) -- both answers occur."""
    fmin = np.where(case.active, case.fmin, -np.inf)
    dmin = cdist(case.xc, case.U).min(axis=1)
    L = np.ones(case.G)
    for i in np.flatnonzero(case.active):
        L[i] = case.cfg["lip"][i] * np.median((case.u_c[:, i] - fmin[i]) / np.maximum(dmin, 1e-3))
    best = lipschitz_margins(case.U, case.xc, case.u_c, L, np.where(case.active, fmin, 0.0))
    diam = np.linalg.norm(case.pts.max(axis=0) - case.pts.min(axis=0)) + 1.0
    return L, best, 1e-12 * (np.abs(case.u_c) + L[None, :] * diam)
