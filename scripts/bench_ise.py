#!/usr/bin/env python
"""Cost of one information-theoretic safe exploration pick (``SafeOpt.ise_point``, csrc/ise.hip).

    python scripts/bench_ise.py [--rows 1000000] [--n 500] [--gps 3] [--K 64,256,1024]
                                [--reps 5] [--out profiles/ise/SUMMARY.txt]

The config-3 shape: a 1000 x 1000 grid, 3 Matern52-ARD GPs at d = 2 with n = 500 observations
each, every fmin finite.  Per K: milliseconds per ``ise_point`` (host clock around the call,
which ends in the read-back of the pick; median, minimum and maximum of ``--reps`` calls after
one warm-up), split into the host-side candidate selection (one download of the variances and of
S, a sort), the device pass (``sgp_grid_ise``: gather, operands, rows, final kernels, one
read-back) on the host clock, and the row kernel alone by the per-launch hipEvents of
``sgp_profile_*``; the operand stage is the device pass minus the row kernel.  Beside the row
kernel the arithmetic floor ``2 N n_pad K G_active`` flop at the fp64 matrix peak, and beside the
whole call the time of a converged ``optimize()`` on the same state (no existing kernel takes part
in ``ise_point``, and ``ise_point`` changes none of them).  One rank.
"""
import argparse, json, os, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_MFMA_F64 = 78.6e12              # flop per second
NOISE = 0.05 ** 2


def spread(ms):
    """(median, minimum, maximum)"""
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def host_ms(ctx, fn, reps):
    ms = []
    for i in range(reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def event_ms(ctx, fn, reps):
    ms = []
    for i in range(reps + 1):
        ctx.sync()
        ctx.profile_enable(True)
        fn()
        t = ctx.profile_read()[0]
        ctx.profile_enable(False)
        if i:
            ms.append(t)
    return spread(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--gps", type=int, default=3)
    ap.add_argument("--K", default="64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    Ks = [int(k) for k in a.K.split(",")]
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    from safeopt_amd.gp_opt import ise_candidates
    side = int(round(a.rows ** 0.5))
    grid_rows = safeopt_amd.linearly_spaced_combinations([(-5., 5.)] * 2, side)
    N = grid_rows.shape[0]
    rng = np.random.RandomState(0)
    X = rng.uniform(-5, 5, (a.n, 2))
    gps = []
    for g in range(a.gps):
        Y = (2.0 + np.sin(X / [0.9 + 0.2 * g, 1.5 - 0.2 * g]).sum(1)
             + 0.05 * rng.standard_normal(a.n))[:, None]
        gps.append(gpy.models.GPRegression(
            X, Y, gpy.kern.Matern52(2, 1.7, [0.9 + 0.1 * g, 1.5], ARD=True), noise_var=NOISE))
    fmin = [0.0] * a.gps
    opt = safeopt_amd.SafeOpt(gps if a.gps > 1 else gps[0], grid_rows,
                              fmin if a.gps > 1 else 0.0, threshold=0.2)
    ctx = opt._backend.ctx
    opt.optimize()
    step = host_ms(ctx, opt.optimize, a.reps)            # converged: no new data in between
    be = opt._backend
    n_safe = int(np.asarray(opt.S).sum())
    n_pad = (a.n + 15) // 16 * 16
    fm = np.asarray(fmin, dtype=float)
    per_k = {}
    for K in Ks:
        x, alpha = opt.ise_point(candidates=K)
        var, S, s = be.ise_state()
        rows = ise_candidates(var, S, s, np.isfinite(fm), K)

        def select():
            v, S_, s_ = be.ise_state()
            return ise_candidates(v, S_, s_, np.isfinite(fm), K)
        r = {"ise_point_ms": host_ms(ctx, lambda: opt.ise_point(candidates=K), a.reps),
             "select_ms": host_ms(ctx, select, a.reps),
             "pass_ms": host_ms(ctx, lambda: be.ise(fm, rows, _hip.ISE_UNSAFE), a.reps),
             "row_kernel_ms": event_ms(ctx, lambda: be.ise(fm, rows, _hip.ISE_UNSAFE), a.reps)}
        r["operands_ms"] = r["pass_ms"][0] - r["row_kernel_ms"][0]
        r["floor_ms"] = 2.0 * N * n_pad * rows.size * a.gps / PEAK_MFMA_F64 * 1e3
        r["candidates"] = int(rows.size)
        r["alpha"], r["x"] = float(alpha), [float(v) for v in x]
        per_k[K] = r
    fmt = lambda t: "%.3f  (%.3f .. %.3f)" % t
    lines = [
        "SafeOpt.ise_point, %d rows (d = 2), %d Matern52-ARD GPs (all active), n = %d, |S| = %d, "
        "about = 'unsafe'; ms, median (minimum .. maximum) of %d calls after one warm-up"
        % (N, a.gps, a.n, n_safe, a.reps),
        "converged optimize() on the same state (host clock)     %s" % fmt(step)]
    for K in Ks:
        r = per_k[K]
        lines += [
            "K = %d candidates" % r["candidates"],
            "  ise_point, whole call (host clock)                    %s" % fmt(r["ise_point_ms"]),
            "    candidate selection on the host (download, sort)    %s" % fmt(r["select_ms"]),
            "    device pass (sgp_grid_ise)                          %s" % fmt(r["pass_ms"]),
            "      k_ise_rows alone (hipEvents)                      %s" % fmt(r["row_kernel_ms"]),
            "      gather, operand kernels, final kernels, read-back %.3f  (pass - rows, medians)"
            % r["operands_ms"],
            "  arithmetic floor 2 N n_pad K G / %.1f TF                %.3f ms;  k_ise_rows / floor"
            " = %.2f" % (PEAK_MFMA_F64 / 1e12, r["floor_ms"], r["row_kernel_ms"][0] / r["floor_ms"])]
    lines.append("counters of k_ise_rows (MFMA busy, VALU busy, stalls): not measured")
    line = json.dumps({"bench": "ise", "rows": N, "n": a.n, "gps": a.gps, "safe": n_safe,
                       "optimize_ms": step, "K": {str(k): v for k, v in per_k.items()}})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
