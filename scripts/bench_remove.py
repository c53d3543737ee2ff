#!/usr/bin/env python
"""Cost of forgetting one observation: ``remove_data_point`` + the interval update, next to what
the same change cost before -- ``set_XY`` without the row (a refit) + the full sweep.

    python scripts/bench_remove.py [--sizes 64,500,2000] [--reps 7] [--out profiles/remove/SUMMARY.txt]

Three Matern-5/2 GPs on one set of inputs (bench.make_config(3) with n rows) on the 1000 x 1000
grid.  Per n and per row (the middle one, row 0), ``--reps`` times, alternating in one process:

  new     ``opt.remove_data_point(row)`` (``sgp_gp_remove`` per GP) + ``confidence`` (which takes
          ``sgp_grid_rank1_remove``), on a SafeOpt whose resident posterior is current;
  parent  ``gp.set_XY`` of the reduced arrays per GP (``sgp_gp_set_data``: the row is not the last
          one) + ``confidence`` as a full sweep, on a twin.

Both are host-clock milliseconds around work that ends in the read-back of max l0[S], i.e. a
stream synchronise.  Between two timed steps the row goes back in (untimed) and the streak
counter is reset, so that every timed ``confidence`` of the new path is a refresh.  The first
repetition (allocations, code upload) is dropped; median [min .. max] of the rest.  The two
optimisers hold the same data after every step: max |Q_new - Q_parent| is printed as a check.
"""
import argparse, os, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def one_size(n, reps, say):
    import bench
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    cfg = bench.make_config(3)
    rng = np.random.default_rng(40 + n)
    X = rng.uniform(-2.0, 2.0, size=(n, cfg["d"]))
    Y = np.empty((n, cfg["G"]))
    for g in range(cfg["G"]):
        f = bench._bumps(X, 102 + g)
        Y[:, g] = f - f.min() + 0.5
    Y += 0.05 * rng.normal(size=Y.shape)
    cfg["X"], cfg["Y"], cfg["n"] = X, Y, n

    def make():
        gps = bench.build_gps(cfg, gpy)
        opt = safeopt_amd.SafeOpt(gps, cfg["grid"], cfg["fmin"], threshold=cfg["threshold"],
                                  beta=cfg["beta"])
        opt._backend.confidence(cfg["beta"], opt.fmin)
        return opt

    opt, twin = make(), make()
    twin._backend.incremental = False
    for gp in twin.gps:
        gp.incremental = False
    be, tb, beta = opt._backend, twin._backend, cfg["beta"]
    ctx = be.ctx
    for label, pick in (("middle row", lambda t: t // 2), ("row 0", lambda t: 0)):
        new_ms, old_ms, qdiff = [], [], 0.0
        for _ in range(reps + 1):
            row = pick(opt.t)
            x, y = opt.x[row].copy(), opt.y[row].copy()
            be._rank1_streak = 0
            ctx.sync()
            t0 = time.perf_counter()
            opt.remove_data_point(row)
            be.confidence(beta, opt.fmin)
            new_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(dv.removed for dv in be._dev()) and be._rank1_streak == 1
            t0 = time.perf_counter()
            for gp in twin.gps:
                gp.set_XY(np.delete(gp.X, row, axis=0), np.delete(gp.Y, row, axis=0))
            tb.confidence(beta, twin.fmin)
            old_ms.append((time.perf_counter() - t0) * 1e3)
            twin._x, twin._y = np.delete(twin._x, row, axis=0), np.delete(twin._y, row, axis=0)
            qdiff = max(qdiff, float(np.max(np.abs(be.download(_hip.Q) - tb.download(_hip.Q)))))
            for o in (opt, twin):                   # the row goes back in, at the end
                o.add_new_data_point(x[None, :], y[None, :])
                o._backend.confidence(beta, o.fmin)

        def fmt(v):
            v = np.array(v[1:])
            return "%8.3f [%7.3f .. %7.3f]" % (np.median(v), v.min(), v.max())
        say("n = %4d  %-10s  new %s ms   parent %s ms   ratio %5.2f   max|dQ| %.1e"
            % (n, label, fmt(new_ms), fmt(old_ms),
               np.median(old_ms[1:]) / np.median(new_ms[1:]), qdiff))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,500,2000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("remove + interval update, 3 GPs (Matern52, d = 2, one set of inputs), 1e6 rows; "
        "host ms, median [min .. max] of %d" % a.reps)
    for n in [int(s) for s in a.sizes.split(",")]:
        one_size(n, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
