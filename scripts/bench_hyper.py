#!/usr/bin/env python
"""Cost of fitting hyper-parameters on the device.

    python scripts/bench_hyper.py [--sizes 200,500,2000] [--dims 2,4] [--sklearn] [--out FILE]

Per (n, d, kernel): the time of ONE likelihood + gradient evaluation (``DeviceGP.lml``:
hipEvents around each of 50 evaluations after 5 warm-up ones, median; the host clock around
the same calls next to it), of the refit an edited hyper-parameter costs
(``parameters_changed()``: upload, factor -- the yardstick the evaluation is held against,
and the only part this script measures on a package without ``DeviceGP.lml``), and of a
whole ``optimize()`` from twice / half the generating values.  ``--sklearn`` adds
scikit-learn's time for the same evaluation on the CPU, for orientation.  Prints one JSON
line; writes nothing unless ``--out`` is given.
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.environ.get("SGP_BENCH_PACKAGE_ROOT") or
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import safeopt_amd.gpy as gpy
from safeopt_amd import _hip


def problem(n, d, kind, seed=0):
    rng = np.random.default_rng(seed + n + d)
    X = rng.uniform(-3, 3, (n, d))
    ls = np.linspace(0.9, 1.5, d)
    # a smooth function plus noise: the likelihood has an interior optimum
    Y = (np.sin(X / ls).sum(1) + 0.05 * rng.normal(size=n))[:, None]
    start = np.where(np.arange(d) % 2 == 0, 2.0, 0.5) * ls
    k = getattr(gpy.kern, kind)(d, 3.0, start, ARD=True)
    return X, Y, k


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


def sklearn_ms(kind, X, Y, k, noise, reps=3):
    from sklearn.gaussian_process import GaussianProcessRegressor as GPR
    from sklearn.gaussian_process.kernels import ConstantKernel as C, RBF, Matern, WhiteKernel
    ls = np.asarray(k.lengthscale)
    sk = RBF(ls) if kind == "RBF" else Matern(ls, nu=2.5)
    g = GPR(C(float(k.variance[0])) * sk + WhiteKernel(noise + 1e-8), alpha=0, optimizer=None)
    g.fit(X, Y[:, 0])
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g.log_marginal_likelihood(g.kernel_.theta, eval_gradient=True)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,500,2000")
    ap.add_argument("--dims", default="2,4")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    rows = []
    for n in [int(s) for s in a.sizes.split(",")]:
        for d in [int(s) for s in a.dims.split(",")]:
            for kind in ("Matern52", "RBF"):
                X, Y, k = problem(n, d, kind)
                noise = 0.1 ** 2
                gp = gpy.models.GPRegression(X, Y, k, noise_var=noise)
                row = {"n": n, "d": d, "kernel": kind + "-ARD"}
                # the yardstick: what an edited hyper-parameter costs through a full refit
                ev, wall = median_ms(lambda i: gp.parameters_changed(), ctx, a.reps, a.warmup)
                row["refit_event_ms"], row["refit_wall_ms"] = ev, wall
                dev = gp._fitted()
                if hasattr(dev, "lml"):
                    desc = k._desc(d)
                    # (theta moves a little every call: nothing can be reused from the last one)
                    ev, wall = median_ms(
                        lambda i: dev.lml(desc[2] * (1 + 1e-3 * (i % 7)), desc[3], noise),
                        ctx, a.reps, a.warmup)
                    row["lml_event_ms"], row["lml_wall_ms"] = ev, wall
                    row["lml_over_refit"] = wall / row["refit_wall_ms"]
                    ev, wall = median_ms(
                        lambda i: dev.set_hyper(desc[2] * (1 + 1e-3 * (i % 7)), desc[3], noise),
                        ctx, a.reps, a.warmup)
                    row["set_hyper_event_ms"], row["set_hyper_wall_ms"] = ev, wall
                    gp2 = gpy.models.GPRegression(X, Y, k.copy(), noise_var=noise)
                    ctx.sync()
                    t0 = time.perf_counter()
                    res = gp2.optimize()
                    ctx.sync()
                    row["optimize_ms"] = (time.perf_counter() - t0) * 1e3
                    row["optimize_evals"] = int(res.funct_eval)
                    row["optimize_f"] = float(res.f_opt)
                if a.sklearn:
                    row["sklearn_cpu_ms"] = sklearn_ms(kind, X, Y, k, noise)
                rows.append(row)
    line = json.dumps({"bench": "hyper", "rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
