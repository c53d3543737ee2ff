"""Case tables and long-double references of the block-append tests
(tests/test_block_ref_cpu.py, tests/test_gpu_block.py), on ``RefGP`` of tests/_incremental_ref.py.

The expected state after a block of ``b`` observations is ``RefGP.append`` applied ``b`` times
-- the next ``b`` rows of the Cholesky factor of the grown matrix -- so no update formula is
under test here.  The new rows of a grid case lie close together (a third of a lengthscale):
their cross terms are then a good part of the correction, and an update that treats them as
independent rank-1 corrections of the old GP is far off (``naive`` in the reference; the CPU
module holds the figures).
"""
import functools

import numpy as np

import _incremental_ref as R
from _gpu_common import smooth

LD = R.LD
MAX_BLOCK = 16

# ---------------------------------------------------------------------------------------
# append_block cases: name (of R.APPEND_CASES: data box, seeds) -> n0 -> n0 + b
# ---------------------------------------------------------------------------------------
APPEND_BLOCK_CASES = {
    "rbf_d1_16": (14, 18),            # crosses n_pad 16
    "mat32_d3_32": (30, 31),          # b = 1
    "mat52_d2_64": (62, 66),
    "prod_d3_128": (126, 142),        # b = 16
    "mat32_d1_256": (254, 258),
    "mat52_d2_512": (510, 513),
    "rbf_d2_1024": (1022, 1026),      # box 4.0 (R.BOX); crosses a 1024-thread trip
    "mat52_d8_lds": (670, 674),
}


@functools.lru_cache(maxsize=None)
def append_block_reference(name):
    """``(spec, X, Y, test rows, n0, snapshot at n0 + b)``.  The data are those of the one-row
    case of the same name; where the block ends inside that case's range the snapshot is the
    one ``R.append_reference`` holds (computed once per session)."""
    spec, d, n_fit, n_end = R.APPEND_CASES[name]
    n0, n1 = APPEND_BLOCK_CASES[name]
    assert n0 == n_fit and 1 <= n1 - n0 <= MAX_BLOCK
    if n1 <= n_end:
        X, Y, Xs, _, _ = R.data(name, d, n_end)
        snap = R.append_reference(name)[n1 - n_fit - 1]
    else:
        X, Y, Xs, _, _ = R.data(name, d, n1)
        gp = R.RefGP(spec, X[:n0], Y[:n0])
        for i in range(n0, n1):
            gp.append(X[i], Y[i])
        snap = R.snapshot(gp, Xs)
    assert snap["n"] == n1
    return spec, X[:n1], Y[:n1], Xs, n0, snap


#: a fit at 12 rows reserves 128: seven blocks of 16 fit (124 rows), the eighth would cross
CAPACITY_N0, CAPACITY_BLOCKS, CAPACITY_END = 12, 7, 12 + 16 * 9


@functools.lru_cache(maxsize=None)
def capacity_reference():
    """``(spec, X, Y, test rows, {n: snapshot})`` at 124 (the last block that fits), 140 (the
    refit of the refused block) and 156 rows (appends resume)."""
    spec, d, _, _ = R.CAPACITY
    X, Y, Xs, _, _ = R.data("capacity_block", d, CAPACITY_END)
    gp = R.RefGP(spec, X[:CAPACITY_N0], Y[:CAPACITY_N0])
    out = {}
    for i in range(CAPACITY_N0, CAPACITY_END):
        gp.append(X[i], Y[i])
        if gp.n in (124, 140, 156):
            out[gp.n] = R.snapshot(gp, Xs, want_linv=False)
    return spec, X, Y, Xs, out


# ---------------------------------------------------------------------------------------
# rank-b cases (the layout of R.RANK1_CASES; b: rows per GP, 0 = the GP is current)
# ---------------------------------------------------------------------------------------
def _rb(d, N, gps, b, steps=1, share=None, betas=(2.0, 3.0, 2.5), ctx_col=None, safe=None):
    return dict(d=d, N=N, gps=gps, b=tuple(b), steps=steps, share=share, betas=betas,
                ctx_col=ctx_col, safe=safe)


_A2, _A5, _B5, _M2 = R._A2, R._A5, R._B5, R._M2
single, PROD3, PROD_CTX = R.single, R.PROD3, R.PROD_CTX

RANKB_CASES = {
    "g1_rbf_d1_N1_safe": _rb(1, 1, [(single("RBF", 1), "a", 7)], [2], safe=True),
    "g1_rbf_d1_N1_unsafe": _rb(1, 1, [(single("RBF", 1), "a", 7)], [2], safe=False),
    "g1_mat32_d2_N15": _rb(2, 15, [(single("Matern32", 2), "a", 33)], [3]),
    "g3_mixed_d3_N197": _rb(3, 197, [(single("RBF", 3), "a", 40), (single("Matern52", 3), "b", 75),
                                      (PROD3, "c", 50)], [3, 0, 2]),
    # the same mix with at most 48 observations per GP before the block: the sweep in front of
    # the refresh is then the thread-per-row kernel, whose bits do not depend on where a row
    # sits in the grid (the matrix-core sweeps fold a row's |L^-1 k|^2 in an order that does)
    "g3_mixed_d3_n48_N197": _rb(3, 197, [(single("RBF", 3), "a", 40), (single("Matern52", 3), "b", 45),
                                          (PROD3, "c", 48)], [3, 0, 2]),
    "g8_d4_N64": _rb(4, 64, [(single(("RBF", "Matern32", "Matern52")[i % 3], 4), "abcd"[i % 4],
                              25 + 6 * i) for i in range(8)], [4] * 8),
    "chain_aaa_444": _rb(2, 197, [_A2, _A2, _A2], [4, 4, 4], share=True),
    "chain_aaa_044": _rb(2, 197, [_A2, _A2, _A2], [0, 4, 4], share=True),
    "chain_aaa_404": _rb(2, 197, [_A2, _A2, _A2], [4, 0, 4], share=True),
    "chain_aaa_440": _rb(2, 197, [_A2, _A2, _A2], [4, 4, 0], share=True),
    "aba_d5": _rb(5, 197, [_A5, _B5, _A5], [4, 4, 4], share=True),
    # 668 -> 672 -> 676: the staging edge R.RANK1_CASES["g1_mat52_d8_lds"] crosses
    "g1_mat52_d8_lds": _rb(8, 197, [(single("Matern52", 8), "a", 668)], [4], steps=2),
    "ctx_prod_d3": _rb(3, 197, [(PROD_CTX, "a", 45), (PROD_CTX, "a", 45)], [3, 3], ctx_col=0.4),
    # a full block; n crosses 64
    "b16_mat52_d2_N4099": _rb(2, 4099, [(_M2, "a", 56), (_M2, "a", 56)], [16, 16]),
}
CLUSTER = 0.35              # the rows of a block lie within this many lengthscales of the first


def tail_rows(gp, b):
    """Rows n - b .. n - 1 of L^-1 in long double: row r is column r of L^-T."""
    n = gp.n
    eye = np.eye(n, dtype=LD)
    return np.array([R.backward_t(gp.L, eye[r]) for r in range(n - b, n)])


@functools.lru_cache(maxsize=None)
def rankb_reference(name):
    """Inputs and expected results of a rank-b case, as ``R.rank1_reference`` lays them out:
    ``pts``, ``X`` / ``Y`` per GP at n_fit, ``fmin``, ``before`` and per step ``xstar`` (bmax, d),
    ``ystar`` (G, bmax), ``beta``, the refits' ``mean`` / ``var`` (G, N) (``mean_ld`` /
    ``var_ld`` in long double), ``Q``, ``S``, ``excluded``, ``ret`` -- plus, per flagged GP,
    ``tail`` = the posterior by the tail-row formula in long double and ``naive`` = the b rows
    taken as independent rank-1 corrections of the old GP (no cross terms)."""
    c = RANKB_CASES[name]
    d, N, G = c["d"], c["N"], len(c["gps"])
    rng = np.random.default_rng(R._seed("block" + name))
    dp = d - (1 if c["ctx_col"] is not None else 0)

    def with_ctx(a):
        a = np.atleast_2d(a)
        if c["ctx_col"] is None:
            return a
        return np.hstack([a, np.full((a.shape[0], 1), c["ctx_col"])])

    Xd = {}
    for _, key, n in c["gps"]:
        if key not in Xd or Xd[key].shape[0] < n:
            Xd[key] = with_ctx(np.random.default_rng(R._seed(name + key)).uniform(-2, 2, (n, dp)))
    Xg = [Xd[key][:n] for _, key, n in c["gps"]]
    Yg = [smooth(X, 11 + g)[:, 0] + 0.3 for g, X in enumerate(Xg)]
    gps = [R.RefGP(spec, X, Y) for (spec, _, _), X, Y in zip(c["gps"], Xg, Yg)]
    upd = [g for g in range(G) if c["b"][g]]
    bmax = max(c["b"])
    kd = [R.kdiag(spec) for spec, _, _ in c["gps"]]
    ls0 = np.ones(d)
    for _, cols, _, ls in c["gps"][upd[0]][0]:
        ls0[list(cols)] = np.maximum(ls0[list(cols)], ls)
    par = np.r_[np.ones(dp), np.zeros(d - dp)]              # parameter columns

    steps, pts = [], None
    for t in range(c["steps"]):
        # the first row of the block as R.rank1_reference picks x*: prior variance closest to
        # 0.3 k(x, x); the others within CLUSTER lengthscales of it
        if t == 0:
            cand = with_ctx(rng.uniform(-1.5, 1.5, size=(R.CANDIDATES, dp)))
            var_c = [R.f64(gps[g].predict(cand)[1]) for g in upd]
        else:
            inside = np.flatnonzero(np.all(np.abs(pts[:, :dp]) <= 2.0, axis=1))
            cand = pts[inside]
            var_c = [steps[-1]["var"][g][inside] for g in upd]
        score = np.zeros(cand.shape[0])
        for g, v in zip(upd, var_c):
            score = np.maximum(score, np.abs(np.log(np.maximum(v / kd[g], 1e-12) / 0.3)))
        x0 = cand[np.argmin(score)]
        xstar = x0[None, :] + CLUSTER * ls0 * par * rng.uniform(-1, 1, size=(bmax, d))
        xstar[0] = x0
        ystar = np.array([smooth(xstar, 11 + g)[:, 0] + 0.3 + 0.6 for g in range(G)])
        if pts is None:
            pts = with_ctx(rng.uniform(-3, 3, size=(N, dp)))
            if N == 1:
                pts[0] = x0 + 0.25 * ls0 * par
            elif N >= 15:
                far = 60.0 * ls0 * par
                pts[N // 2:N // 2 + bmax] = xstar           # the new observations themselves
                pts[0] = Xg[0][0]                           # training rows: r = 0
                pts[N - 1] = Xg[-1][-1]
                pts[1] = x0 + far                           # the covariance underflows
                pts[N - 2] = x0 - far
            before = [gp.predict(pts, key="grid") for gp in gps]
            before = (R.f64([b[0] for b in before]), R.clip_var([b[1] for b in before]))
        st = {"xstar": xstar, "ystar": ystar, "beta": c["betas"][1 + t], "tail": {}, "naive": {}}
        for g in upd:
            b = c["b"][g]
            m0, v0 = gps[g].predict(pts, key="grid")
            nm, nv = m0.copy(), v0.copy()
            for j in range(b):
                cm, cv, _ = gps[g].rank1(pts, xstar[j], ystar[g][j], key="grid")
                nm += cm - m0
                nv += cv - v0
            st["naive"][g] = (nm, nv)
            for j in range(b):
                gps[g].append(xstar[j], ystar[g][j])
            rows = tail_rows(gps[g], b)                     # (b, n)
            tj = rows @ R.kern(gps[g].spec, gps[g].X, pts)  # (b, N)
            gam = rows @ gps[g].Y
            st["tail"][g] = (m0 + gam @ tj, v0 - (tj * tj).sum(0))
        post = [gp.predict(pts, key="grid") for gp in gps]
        st["mean_ld"] = [p[0] for p in post]
        st["var_ld"] = [p[1] for p in post]
        st["mean"] = R.f64([p[0] for p in post])
        st["var"] = R.clip_var([p[1] for p in post])
        steps.append(st)

    def bounds(st):
        sd = np.sqrt(st["var"])
        return st["mean"] - st["beta"] * sd, st["mean"] + st["beta"] * sd

    lo1 = bounds(steps[0])[0]
    if N == 1:
        fmin = lo1[:, 0] - (0.1 if c["safe"] else -0.1)
    else:
        fmin = np.array([R._quantile_cut(lo1[g], 1.0 - 0.6 ** (1.0 / G)) for g in range(G)])
    for st in steps:
        lo, up = bounds(st)
        st["Q"] = np.stack([lo, up], axis=2).transpose(1, 0, 2).reshape(N, 2 * G)
        st["S"] = np.all(lo > fmin[:, None], axis=0)
        st["excluded"] = np.any(np.abs(lo - fmin[:, None]) < R.S_EXCLUDE, axis=0)
        st["ret"] = (float(np.max(lo[0][st["S"]])), True) if st["S"].any() else (-np.inf, False)
    return {"pts": pts, "X": Xg, "Y": Yg, "fmin": fmin, "steps": steps, "before": before,
            "kdiag": kd, "beta0": c["betas"][0]}


# ---------------------------------------------------------------------------------------
# SafeOpt / SafeOptSwarm end to end
# ---------------------------------------------------------------------------------------
E2E_SPECS = (single("Matern52", 2), single("RBF", 2))
E2E_N, E2E_SIDE = 30, 40


def e2e_data():
    """30 observations of two smooth functions on [-2, 2]^2, the first well above fmin = 0
    around the origin."""
    rng = np.random.default_rng(4242)
    X = rng.uniform(-1.0, 1.0, size=(E2E_N, 2))
    return X, np.stack([e2e_f(X, g) for g in range(2)], axis=1)


def e2e_f(X, g):
    X = np.atleast_2d(X)
    return 1.5 - 0.4 * (X ** 2).sum(1) + 0.25 * smooth(X, 21 + g)[:, 0]
