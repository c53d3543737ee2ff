#!/usr/bin/env python
"""Cost of the leave-one-out diagnostics on the device.

    python scripts/bench_loo.py [--sizes 500,2000] [--dims 2,4] [--out FILE]

Per (n, d), Matern-5/2 ARD: the time of ``DeviceGP.loo()`` (all n leave-one-out predictions
from the resident factor), of ONE ``DeviceGP.loo_lml`` evaluation (factorisation, objective
and gradient), of ONE ``DeviceGP.lml`` evaluation on the same GP -- hipEvents around each of
``--reps`` calls after ``--warmup`` warm ones, median; the host clock around the same calls
next to it -- and of the n refits the closed form replaces: ``--brute-rows`` of them are
timed (the data without row i factorised on the device, row i predicted) and their median is
multiplied by n, an extrapolation.  ``loo_roof_ms`` is arithmetic, not a measurement: the
n (n + 1) / 2 doubles of the lower triangle of L^-1 at ``--hbm-gbs``.  On a package without
``DeviceGP.loo`` only the ``lml`` column is measured (the yardstick of the parent commit).
Prints one JSON line; writes nothing unless ``--out`` is given.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.environ.get("SGP_BENCH_PACKAGE_ROOT") or
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import safeopt_amd.gpy as gpy
from safeopt_amd import _hip


def problem(n, d, seed=0):
    rng = np.random.default_rng(seed + n + d)
    X = rng.uniform(-3, 3, (n, d))
    ls = np.linspace(0.9, 1.5, d)
    Y = (np.sin(X / ls).sum(1) + 0.05 * rng.normal(size=n))[:, None]
    return X, Y, gpy.kern.Matern52(d, 1.5, ls, ARD=True)


def median_ms(fn, ctx, reps, warm):
    ev, wall = [], []
    for i in range(warm + reps):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        fn(i)
        e = ctx.timer_stop()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(e)
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,2000")
    ap.add_argument("--dims", default="2,4")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--brute-rows", type=int, default=4)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0,
                    help="HBM bandwidth the roof of loo() is computed from (achievable, GB/s)")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for d in [int(s) for s in a.dims.split(",")]:
            X, Y, k = problem(n, d)
            noise = 0.1 ** 2
            gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
            dev = gp._fitted()
            desc = k._desc(d)
            row = {"n": n, "d": d, "kernel": "Matern52-ARD"}
            # (theta moves a little every call: nothing can be reused from the last one)
            theta = lambda i: (desc[2] * (1 + 1e-3 * (i % 7)), desc[3], noise)
            ev, wall = median_ms(lambda i: dev.lml(*theta(i)), ctx, a.reps, a.warmup)
            row["lml_event_ms"], row["lml_wall_ms"] = ev, wall
            if hasattr(dev, "loo"):
                ev, wall = median_ms(lambda i: dev.loo_lml(*theta(i)), ctx, a.reps, a.warmup)
                row["loo_lml_event_ms"], row["loo_lml_wall_ms"] = ev, wall
                row["loo_lml_over_lml"] = ev / row["lml_event_ms"]
                ev, wall = median_ms(lambda i: dev.loo(), ctx, a.reps, a.warmup)
                row["loo_event_ms"], row["loo_wall_ms"] = ev, wall
                row["loo_roof_ms"] = n * (n + 1) / 2 * 8 / (a.hbm_gbs * 1e9) * 1e3
                # the refits it replaces, a few of them
                other = gpy.models.GPRegression(X[1:], Y[1:], k.copy(), noise_var=noise)
                odev = other._fitted()
                picks = np.linspace(0, n - 1, a.brute_rows).astype(int)

                def refit(i):
                    r = picks[i % len(picks)]
                    keep = np.arange(n) != r
                    odev.set_data(X[keep], Y[keep, 0])
                    odev.predict(X[r:r + 1])
                ev, wall = median_ms(refit, ctx, a.brute_rows, 1)
                row["one_refit_event_ms"], row["one_refit_wall_ms"] = ev, wall
                row["n_refits_extrapolated_ms"] = wall * n
                row["refits_over_loo"] = wall * n / row["loo_wall_ms"]
            rows.append(row)
    line = json.dumps({"bench": "loo", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
