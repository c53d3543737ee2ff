"""A plain GP in ``np.longdouble`` and the case table of the incremental-path tests
(tests/test_incremental_ref_cpu.py, tests/test_gpu_incremental.py).

The reference is a second, independent statement of the GP the device computes: kernels from
coordinate differences, ``Ky = K + (noise + 1e-8) I``, a column Cholesky, forward / backward
substitution -- loops over NumPy long-double arrays, which never reach BLAS or LAPACK.  It
shares nothing with ``oracle/``.  One more observation is one more row of the Cholesky
factor (a forward substitution): the rows of a Cholesky factor do not depend on the rows
behind them, so that IS the factor of the grown matrix, not an update formula under test.

Inputs: ``smooth()`` targets, noise 0.05^2, variance 1.7, X uniform in [-2, 2]^d, test rows
uniform in [-3, 3]^d, lengthscales ``linspace(0.8, 1.6, d)`` (d <= 5) / ``linspace(2.5, 4.0,
d)`` (d >= 6: with the short ones K is nearly diagonal at d = 8 and a rank-1 correction too
small to show a wrong update vector).  The conditioning stays moderate (cond Ky of a few 1e5);
what varies is what selects code paths: shapes, kernel kinds, the mix of GPs, the order of calls.
"""
import functools

import numpy as np

from _gpu_common import smooth

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble has no 64-bit mantissa on this platform"

NOISE = 0.05 ** 2
VARIANCE = 1.7
ROWS = 300                  # test rows of the append / pop cases
LINV_MAX_N = 520            # the reference L^-1 is formed up to this n
S_EXCLUDE = 1e-8            # |lo - fmin| below this: the row's S is not compared


# ---------------------------------------------------------------------------------------
# kernels: spec = ((kind, columns, variance, lengthscales), ...), a product of its parts
# ---------------------------------------------------------------------------------------
def lengthscales(d):
    return np.linspace(0.8, 1.6, d) if d <= 5 else np.linspace(2.5, 4.0, d)


def single(kind, d):
    return ((kind, tuple(range(d)), VARIANCE, tuple(lengthscales(d))),)


#: RBF x Matern-5/2 on overlapping columns of a 3-column input
PROD3 = (("RBF", (0, 1), VARIANCE, (1.2, 1.6)), ("Matern52", (1, 2), 1.0, (1.6, 1.2)))
#: parameters x context: Matern-3/2 on two parameters times RBF on the context column
PROD_CTX = (("Matern32", (0, 1), VARIANCE, (0.8, 1.6)), ("RBF", (2,), 1.0, (1.5,)))


def make_kernel(ns, spec):
    """The kernel object of ``spec`` in a namespace with GPy's constructors
    (``safeopt_amd.gpy.kern`` or ``oracle.gp_numpy``)."""
    k = None
    for kind, cols, var, ls in spec:
        part = getattr(ns, kind)(len(cols), variance=var, lengthscale=np.array(ls),
                                 ARD=True, active_dims=list(cols))
        k = part if k is None else k * part
    return k


def kdiag(spec):
    return float(np.prod([p[2] for p in spec]))


def kern(spec, A, B):
    """k(A, B) in long double, from differences."""
    A = np.asarray(A, dtype=LD)
    B = np.asarray(B, dtype=LD)
    out = np.ones((A.shape[0], B.shape[0]), dtype=LD)
    for kind, cols, var, ls in spec:
        r2 = np.zeros_like(out)
        for c, l in zip(cols, ls):
            diff = (A[:, c][:, None] - B[:, c][None, :]) / LD(l)
            r2 += diff * diff
        if kind == "RBF":
            k = np.exp(-r2 / LD(2))
        elif kind == "Matern32":
            r = np.sqrt(LD(3) * r2)
            k = (LD(1) + r) * np.exp(-r)
        elif kind == "Matern52":
            r = np.sqrt(LD(5) * r2)
            k = (LD(1) + r + r * r / LD(3)) * np.exp(-r)
        else:
            raise ValueError(kind)
        out *= LD(var) * k
    return out


# ---------------------------------------------------------------------------------------
# linear algebra
# ---------------------------------------------------------------------------------------
def cholesky(A):
    """Lower factor, column by column."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        assert c[0] > 0, "not positive definite at column %d" % j
        L[j:, j] = c / np.sqrt(c[0])
    return L


def forward(L, B):
    """Solve L V = B (B a vector or a matrix of columns)."""
    V = np.array(B, dtype=LD)
    for j in range(L.shape[0]):
        V[j] = V[j] / L[j, j]
        if V.ndim == 1:
            V[j + 1:] -= L[j + 1:, j] * V[j]
        else:
            V[j + 1:] -= L[j + 1:, j][:, None] * V[j][None, :]
    return V


def backward_t(L, b):
    """Solve L^T a = b (a vector)."""
    a = np.array(b, dtype=LD)
    for j in range(L.shape[0] - 1, -1, -1):
        a[j] = a[j] / L[j, j]
        a[:j] -= L[j, :j] * a[j]
    return a


class RefGP(object):
    """Exact GP regression, zero mean, in long double."""

    def __init__(self, spec, X, Y, noise=NOISE):
        self.spec, self.noise = spec, LD(noise)
        self.X = np.array(X, dtype=LD).reshape(len(X), -1)
        self.Y = np.array(Y, dtype=LD).reshape(-1)
        self.L = cholesky(self.Ky())
        self.z = forward(self.L, self.Y)
        self._rows = {}          # key -> [rows, L^-1 k(X, rows)]

    n = property(lambda self: self.X.shape[0])

    def Ky(self):
        K = kern(self.spec, self.X, self.X)
        K[np.diag_indices(self.n)] += self.noise + LD(1e-8)
        return K

    def append(self, x, y):
        """One more observation: the next row of the factor."""
        x = np.asarray(x, dtype=LD).reshape(1, -1)
        k = kern(self.spec, self.X, x)[:, 0]
        t = forward(self.L, k)
        s2 = LD(kdiag(self.spec)) + self.noise + LD(1e-8) - t @ t
        assert s2 > 0
        n = self.n
        L = np.zeros((n + 1, n + 1), dtype=LD)
        L[:n, :n] = self.L
        L[n, :n] = t
        L[n, n] = np.sqrt(s2)
        self.L = L
        self.X = np.vstack([self.X, x])
        self.Y = np.append(self.Y, LD(y))
        self.z = np.append(self.z, (LD(y) - t @ self.z[:n]) / L[n, n])
        for ent in self._rows.values():
            kr = kern(self.spec, x, ent[0])[0]
            ent[1] = np.vstack([ent[1], ((kr - t @ ent[1]) / L[n, n])[None, :]])

    def pop(self):
        n = self.n - 1
        self.L, self.X, self.Y, self.z = self.L[:n, :n], self.X[:n], self.Y[:n], self.z[:n]
        for ent in self._rows.values():
            ent[1] = ent[1][:n]

    def alpha(self):
        return backward_t(self.L, self.z)

    def Linv(self):
        return forward(self.L, np.eye(self.n, dtype=LD))

    def solve(self, b):
        """Ky^-1 b."""
        return backward_t(self.L, forward(self.L, b))

    def predict(self, rows, key=None):
        """Posterior mean and variance (not clipped) at ``rows``; ``key``: keep
        L^-1 k(X, rows) and carry it through later appends / pops."""
        if key is not None and key in self._rows:
            V = self._rows[key][1]
        else:
            V = forward(self.L, kern(self.spec, self.X, rows))
            if key is not None:
                self._rows[key] = [np.asarray(rows, dtype=LD), V]
        return self.z @ V, LD(kdiag(self.spec)) - (V * V).sum(0)

    def rank1(self, rows, x, y, key=None):
        """Closed-form posterior at ``rows`` after one more observation (x, y):
        ``(mean, var, w^T k(X, rows))``, from this GP's state (n rows)."""
        x = np.asarray(x, dtype=LD).reshape(1, -1)
        k = kern(self.spec, self.X, x)[:, 0]
        w = self.solve(k)
        s2 = LD(kdiag(self.spec)) + self.noise + LD(1e-8) - k @ w
        mu_x = k @ self.alpha()
        wk = w @ kern(self.spec, self.X, rows)
        cx = kern(self.spec, x, rows)[0] - wk
        m, v = self.predict(rows, key)
        return m + cx * (LD(y) - mu_x) / s2, v - cx * cx / s2, wk


def f64(a):
    return np.asarray(a, dtype=np.float64)


def clip_var(v):
    return np.maximum(f64(v), 1e-15)


# ---------------------------------------------------------------------------------------
# append / pop cases
# ---------------------------------------------------------------------------------------
#: name -> (kernel spec, d, n_fit, n_end); the sizes cross what the name says
APPEND_CASES = {
    "rbf_d1_16": (single("RBF", 1), 1, 14, 18),
    "mat32_d3_32": (single("Matern32", 3), 3, 30, 34),
    "mat52_d2_64": (single("Matern52", 2), 2, 62, 66),
    "prod_d3_128": (PROD3, 3, 126, 130),
    "mat32_d1_256": (single("Matern32", 1), 1, 254, 258),
    "mat52_d2_512": (single("Matern52", 2), 2, 510, 514),
    "rbf_d2_1024": (single("RBF", 2), 2, 1022, 1026),
    "mat52_d8_lds": (single("Matern52", 8), 8, 670, 674),
}

#: name -> (kernel spec, d, n): fit, pop 7, append 3 other rows, pop 1, append 2
POP_CASES = {
    "mat52_d2_40": (single("Matern52", 2), 2, 40),
    "rbf_d3_70": (single("RBF", 3), 3, 70),
    "mat32_d1_260": (single("Matern32", 1), 1, 260),
}
POP_SCRIPT = (("pop", 7), ("append", 3), ("pop", 1), ("append", 2))

#: test_append_past_capacity: 12 rows, then one-row set_XY calls.  A fit at 12 rows reserves
#: 128 rows ((12 + 64) rounded up to a multiple of 64), so the 117th call is the first one
#: that cannot append; the data go on to 132 rows so that appends are seen to resume.
CAPACITY = (single("Matern52", 2), 2, 12, 132)
CAPACITY_CHECK = (13, 44, 45, 76, 77, 92, 128, 129, 130, 132)


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


#: half-width of the data box where it is not 2.  1026 RBF observations in [-2, 2]^2 leave
#: posterior variances of 1e-5 k(x, x), where the float64 oracle itself is 2e-7 off in relative
#: terms -- 2 % of the 1e-5 clause of check_posterior; in [-4, 4]^2 it keeps the 1 % margin.
BOX = {"rbf_d2_1024": 4.0}


#: The last two rows of this case are a pair of neighbours in a hole of the data (the other
#: rows within two lengthscales of the first of them are moved out to that distance), and the
#: first test row is a copy of the first of them: the last append then moves alpha[1024] -- the
#: second trip of k_append_finish's 1024 threads -- by a good part of max |alpha|, and the
#: mean next to it likewise (tests/test_incremental_ref_cpu.py has the figures).  Among 1024
#: rows spread evenly no single entry of w = Ky^-1 k(X, x*) does.
PAIR = {"rbf_d2_1024": ((1.0, -1.0), (1.5, -0.2))}


def data(name, d, n, extra=0):
    """(X, Y, test rows, extra rows, their targets) of a case."""
    rng = np.random.default_rng(_seed(name))
    box = BOX.get(name, 2.0)
    X = rng.uniform(-box, box, size=(n, d))
    Xs = rng.uniform(-box - 1, box + 1, size=(ROWS, d))
    E = rng.uniform(-box, box, size=(extra, d))
    if name in PAIR:
        P = np.array(PAIR[name][0])
        rho = np.sqrt((((X - P) / lengthscales(d)) ** 2).sum(1))
        near = rho < 2.0
        X[near] = P + (X[near] - P) * (2.0 / rho[near])[:, None]
        X[n - 2:] = PAIR[name]
        Xs[0] = X[n - 2]
    s = _seed(name) % 89
    return X, smooth(X, s)[:, 0], Xs, E, smooth(E, s)[:, 0] if extra else np.zeros(0)


def snapshot(gp, Xs, want_linv=True):
    m, v = gp.predict(Xs, key="rows")
    out = {"n": gp.n, "alpha": f64(gp.alpha()), "mean": f64(m), "var": clip_var(v),
           "X": f64(gp.X), "Y": f64(gp.Y)}
    if want_linv and gp.n <= LINV_MAX_N:
        out["Linv"] = f64(gp.Linv())
    return out


@functools.lru_cache(maxsize=None)
def append_reference(name):
    """The refits at n_fit + 1 .. n_end: a list of snapshots."""
    spec, d, n_fit, n_end = APPEND_CASES[name]
    X, Y, Xs, _, _ = data(name, d, n_end)
    gp = RefGP(spec, X[:n_fit], Y[:n_fit])
    out = []
    for i in range(n_fit, n_end):
        gp.append(X[i], Y[i])
        out.append(snapshot(gp, Xs))
    return out


@functools.lru_cache(maxsize=None)
def pop_reference(name):
    """Snapshots after the fit and after every single call of POP_SCRIPT."""
    spec, d, n = POP_CASES[name]
    X, Y, Xs, E, YE = data(name, d, n, extra=5)
    gp = RefGP(spec, X, Y)
    out, e = [("fit", snapshot(gp, Xs))], 0
    for what, count in POP_SCRIPT:
        for _ in range(count):
            if what == "pop":
                gp.pop()
            else:
                gp.append(E[e], YE[e])
                e += 1
            out.append((what, snapshot(gp, Xs)))
    return out


@functools.lru_cache(maxsize=None)
def capacity_reference():
    spec, d, n0, n_end = CAPACITY
    X, Y, Xs, _, _ = data("capacity", d, n_end)
    gp = RefGP(spec, X[:n0], Y[:n0])
    out = {}
    for i in range(n0, n_end):
        gp.append(X[i], Y[i])
        if gp.n in CAPACITY_CHECK:
            out[gp.n] = snapshot(gp, Xs, want_linv=False)
    return out


# ---------------------------------------------------------------------------------------
# rank-1 cases
# ---------------------------------------------------------------------------------------
# gps: (kernel spec, data key, n_fit) per GP -- GPs with the same data key have the same X
# (their targets differ); which: the GPs that get the new observation and are refreshed;
# steps: consecutive refreshes; share: Context.set_share for the case (None: leave it);
# ctx_col: value of a trailing context column the grid gets through set_context.
def _r1(d, N, gps, which, steps=1, share=None, betas=(2.0, 3.0, 2.5), ctx_col=None, safe=None):
    return dict(d=d, N=N, gps=gps, which=which, steps=steps, share=share, betas=betas,
                ctx_col=ctx_col, safe=safe)


_A2 = (single("Matern32", 2), "a", 48)
_B2 = (single("Matern32", 2), "b", 48)
_A5 = (single("RBF", 5), "a", 60)
_B5 = (single("RBF", 5), "b", 60)
_M2 = single("Matern52", 2)

RANK1_CASES = {
    # one row, once safe and once not (the value returned is -inf and the flag false)
    "g1_rbf_d1_N1_safe": _r1(1, 1, [(single("RBF", 1), "a", 7)], [1], safe=True),
    "g1_rbf_d1_N1_unsafe": _r1(1, 1, [(single("RBF", 1), "a", 7)], [1], safe=False),
    "g1_mat32_d2_N15": _r1(2, 15, [(single("Matern32", 2), "a", 33)], [1]),
    "g3_mixed_d3_N197": _r1(3, 197, [(single("RBF", 3), "a", 40), (single("Matern52", 3), "b", 75),
                                      (PROD3, "c", 50)], [1, 0, 1]),
    "g8_d4_N64": _r1(4, 64, [(single(("RBF", "Matern32", "Matern52")[i % 3], 4), "abcd"[i % 4],
                              25 + 6 * i) for i in range(8)], [1] * 8),
    "chain_aaa_111": _r1(2, 197, [_A2, _A2, _A2], [1, 1, 1], share=True),
    "chain_aaa_011": _r1(2, 197, [_A2, _A2, _A2], [0, 1, 1], share=True),
    "chain_aaa_101": _r1(2, 197, [_A2, _A2, _A2], [1, 0, 1], share=True),
    "chain_aaa_110": _r1(2, 197, [_A2, _A2, _A2], [1, 1, 0], share=True),
    "aba_d5": _r1(5, 197, [_A5, _B5, _A5], [1, 1, 1], share=True),
    # 671 -> 672 -> 673: n_pad 672 is staged in LDS (672 * 9 = 6048 doubles), 688 is not
    "g1_mat52_d8_lds": _r1(8, 197, [(single("Matern52", 8), "a", 671)], [1], steps=2),
    "ctx_prod_d3": _r1(3, 197, [(PROD_CTX, "a", 45), (PROD_CTX, "a", 45)], [1, 1], ctx_col=0.4),
    # the longest run of refreshes a BO loop sees before a forced sweep; crosses n = 64
    "streak_mat52_d2": _r1(2, 4099, [(_M2, "a", 56), (_M2, "a", 56)], [1, 1], steps=15,
                           betas=(2.0,) + tuple(2.2 + 0.1 * t for t in range(15))),
}
CANDIDATES = 64


def _quantile_cut(lo, q):
    """A threshold between two neighbouring values of ``lo``, about a fraction q up."""
    s = np.sort(lo)
    k = min(max(1, int(round(q * s.size))), s.size - 1)
    while k < s.size - 1 and s[k] - s[k - 1] < 1e-6:      # (not between two equal values)
        k += 1
    return 0.5 * (s[k - 1] + s[k])


@functools.lru_cache(maxsize=None)
def rank1_reference(name):
    """Inputs and expected results of a rank-1 case:

    ``pts`` (N, d) grid rows, ``X`` / ``Y`` per GP at n_fit, ``fmin`` (G,), and per step
    ``xstar``, ``ystar`` (G,), ``beta`` and the refits' ``mean`` / ``var`` (G, N), ``Q``
    (N, 2 G), ``S``, ``excluded`` (rows whose S is not compared), ``ret`` (max lo_0 over S,
    any safe) -- plus ``before`` (mean, var at n_fit) and the sensitivity figures
    ``wk`` = max_rows |w^T k(X, x)| / k(x, x) per step and updated GP."""
    c = RANK1_CASES[name]
    d, N, G = c["d"], c["N"], len(c["gps"])
    rng = np.random.default_rng(_seed(name))
    dp = d - (1 if c["ctx_col"] is not None else 0)         # parameter columns

    def with_ctx(a):
        a = np.atleast_2d(a)
        if c["ctx_col"] is None:
            return a
        return np.hstack([a, np.full((a.shape[0], 1), c["ctx_col"])])

    Xd = {}
    for _, key, n in c["gps"]:
        if key not in Xd or Xd[key].shape[0] < n:
            Xd[key] = with_ctx(np.random.default_rng(_seed(name + key)).uniform(-2, 2, (n, dp)))
    Xg = [Xd[key][:n] for _, key, n in c["gps"]]
    Yg = [smooth(X, 11 + g)[:, 0] + 0.3 for g, X in enumerate(Xg)]
    gps = [RefGP(spec, X, Y) for (spec, _, _), X, Y in zip(c["gps"], Xg, Yg)]
    upd = [g for g in range(G) if c["which"][g]]
    kd = [kdiag(spec) for spec, _, _ in c["gps"]]
    ls0 = np.ones(d)
    for _, cols, _, ls in c["gps"][upd[0]][0]:
        ls0[list(cols)] = np.maximum(ls0[list(cols)], ls)

    # x* of every step: of CANDIDATES points inside the data box the one whose prior
    # variance under the updated GPs is closest to 0.3 k(x, x) -- far enough from the data
    # for the refresh to move mean and variance, close enough for w^T k(X, x) to matter.
    # The grid gets a copy of the first x*; the later ones are chosen among the grid's own
    # rows inside the data box, so every step has its x* on the grid.
    steps, pts = [], None
    for t in range(c["steps"]):
        if t == 0:
            cand = with_ctx(rng.uniform(-1.5, 1.5, size=(CANDIDATES, dp)))
            var_c = [f64(gps[g].predict(cand)[1]) for g in upd]
        else:
            inside = np.flatnonzero(np.all(np.abs(pts[:, :dp]) <= 2.0, axis=1))
            cand = pts[inside]
            var_c = [steps[-1]["var"][g][inside] for g in upd]
        score = np.zeros(cand.shape[0])
        for g, v in zip(upd, var_c):
            score = np.maximum(score, np.abs(np.log(np.maximum(v / kd[g], 1e-12) / 0.3)))
        xstar = cand[np.argmin(score)]
        ystar = np.array([smooth(xstar[None, :], 11 + g)[0, 0] + 0.3 + 0.6 for g in range(G)])
        if pts is None:
            pts = with_ctx(rng.uniform(-3, 3, size=(N, dp)))
            if N == 1:
                pts[0] = xstar + 0.25 * ls0 * (1 if c["ctx_col"] is None else
                                               np.r_[np.ones(dp), 0.0])
            elif N >= 15:
                far = 60.0 * ls0
                if c["ctx_col"] is not None:
                    far[-1] = 0.0
                pts[N // 2] = xstar                       # the new observation itself
                pts[0] = Xg[0][0]                         # training rows: r = 0
                pts[N - 1] = Xg[-1][-1]
                pts[1] = xstar + far                      # the covariance underflows
                pts[N - 2] = xstar - far
            before = [gp.predict(pts, key="grid") for gp in gps]
            before = (f64([b[0] for b in before]), clip_var([b[1] for b in before]))
        st = {"xstar": xstar, "ystar": ystar, "beta": c["betas"][1 + t], "wk": {}, "closed": {}}
        for g in upd:
            cm, cv, wk = gps[g].rank1(pts, xstar, ystar[g], key="grid")
            st["wk"][g] = float(np.max(np.abs(wk))) / kd[g]
            st["closed"][g] = (cm, cv)
            gps[g].append(xstar, ystar[g])
        post = [gp.predict(pts, key="grid") for gp in gps]
        st["mean_ld"] = [p[0] for p in post]
        st["var_ld"] = [p[1] for p in post]
        st["mean"] = f64([p[0] for p in post])
        st["var"] = clip_var([p[1] for p in post])
        steps.append(st)

    # fmin from the first step's lower bounds: between two neighbouring values, so that
    # about 0.6 of the rows are safe when the GPs' bounds are independent
    def bounds(st):
        sd = np.sqrt(st["var"])
        return st["mean"] - st["beta"] * sd, st["mean"] + st["beta"] * sd

    lo1 = bounds(steps[0])[0]
    if N == 1:
        fmin = lo1[:, 0] - (0.1 if c["safe"] else -0.1)
    else:
        fmin = np.array([_quantile_cut(lo1[g], 1.0 - 0.6 ** (1.0 / G)) for g in range(G)])
    for st in steps:
        lo, up = bounds(st)
        st["Q"] = np.stack([lo, up], axis=2).transpose(1, 0, 2).reshape(N, 2 * G)
        st["S"] = np.all(lo > fmin[:, None], axis=0)
        st["excluded"] = np.any(np.abs(lo - fmin[:, None]) < S_EXCLUDE, axis=0)
        st["ret"] = (float(np.max(lo[0][st["S"]])), True) if st["S"].any() else (-np.inf, False)
    return {"pts": pts, "X": Xg, "Y": Yg, "fmin": fmin, "steps": steps, "before": before,
            "kdiag": kd, "beta0": c["betas"][0]}


CTX_SECOND = -0.7           # the context of the step after ctx_prod_d3's refresh


@functools.lru_cache(maxsize=None)
def context_switch_reference():
    """After ``ctx_prod_d3``'s step: the context column changes to CTX_SECOND and every GP
    gets one more observation there.  ``(x2, y2 (G,), beta, mean, var (G, N), Q, S, excluded)``
    of the refits at the rows with the new context -- what a sweep gives, and what a refresh
    of the posterior resident for the old context cannot."""
    case, ref = RANK1_CASES["ctx_prod_d3"], rank1_reference("ctx_prod_d3")
    st = ref["steps"][0]
    pts = ref["pts"].copy()
    pts[:, -1] = CTX_SECOND
    x2 = np.r_[-st["xstar"][:-1], CTX_SECOND]
    G = len(case["gps"])
    y2 = np.array([smooth(x2[None, :], 11 + g)[0, 0] + 0.9 for g in range(G)])
    beta = 2.0
    mean, var = [], []
    for g in range(G):
        gp = RefGP(case["gps"][g][0], ref["X"][g], ref["Y"][g])
        gp.append(st["xstar"], st["ystar"][g])
        gp.append(x2, y2[g])
        m, v = gp.predict(pts)
        mean.append(f64(m))
        var.append(clip_var(v))
    mean, var = np.array(mean), np.array(var)
    lo, up = mean - beta * np.sqrt(var), mean + beta * np.sqrt(var)
    return {"x2": x2, "y2": y2, "beta": beta, "pts": pts, "mean": mean, "var": var,
            "Q": np.stack([lo, up], axis=2).transpose(1, 0, 2).reshape(-1, 2 * G),
            "S": np.all(lo > ref["fmin"][:, None], axis=0),
            "excluded": np.any(np.abs(lo - ref["fmin"][:, None]) < S_EXCLUDE, axis=0)}
