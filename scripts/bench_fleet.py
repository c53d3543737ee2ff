"""Many small SafeOpt problems at once: ``SafeOptFleet.optimize()`` against the Python loop over
``SafeOpt.optimize()`` on the same objects and states.

    python scripts/bench_fleet.py [--sizes 1,16,64,256,1024] [--out FILE] [--loop-only]
                                  [--package-root DIR]

B copies of the benchmark's config 1 (``bench.py: config1`` -- 1-D RBF, the 1000-point grid on
[-10, 10], SafeOpt from x0 = 0 on a sampled function, threshold 0.2), each with its own seed.
Two states are timed: "growing" (3 observations: the first candidate is usually an expander, the
step is the launch alone) and "converged" (20 observations: most members' first candidate is not
certified and they continue alone through the test of every candidate).  Per state and B:
microseconds per member-step, the median of 5 runs after warm-up with the spread (min .. max),
for the fleet and for the loop; in the converged state also how many members took the
continuation.  Last, whole BO iterations of the fleet -- ``fleet.optimize()`` plus B
``add_new_data_point`` -- split into the two parts.

``--loop-only`` times the loop alone (a tree without ``SafeOptFleet``: the parent commit, with
``--package-root`` pointing at it).  One JSON line per measurement on stdout; ``--out`` also
writes the table."""
import argparse
import json
import os
import sys
import time

import numpy as np


def build_members(safeopt_amd, gpy, count):
    """``count`` optimisers at x0 = 0 with their sampled functions (seed = member number)."""
    state = np.random.get_state()
    opts, funs = [], []
    try:
        bounds = [(-10., 10.)]
        grid = safeopt_amd.linearly_spaced_combinations(bounds, 1000)
        for seed in range(count):
            np.random.seed(seed)
            kern = gpy.kern.RBF(1, variance=2.0, lengthscale=1.0)
            fun = safeopt_amd.sample_gp_function(kern, bounds, 0.05 ** 2, 100)
            x0 = np.zeros((1, 1))
            gp = gpy.models.GPRegression(x0, fun(x0), kern, noise_var=0.05 ** 2)
            opt = safeopt_amd.SafeOpt(gp, grid, float(fun(x0, noise=False)[0, 0]) - 1.0,
                                      threshold=0.2)
            opt._backend.incremental = False
            opts.append(opt)
            funs.append(fun)
    finally:
        np.random.set_state(state)
    return opts, funs


def advance(opts, funs, n):
    """Every member up to ``n`` observations by its own SafeOpt run."""
    for opt, fun in zip(opts, funs):
        while opt.gp.X.shape[0] < n:
            x = opt.optimize()
            opt.add_new_data_point(x, fun(x))


def timed(step, ctx, members, runs=5, budget=1500):
    """us per member-step: median, min, max of ``runs`` runs of ``reps`` steps each."""
    reps = max(2, budget // members)
    for _ in range(3):
        step()
    out = []
    for _ in range(runs):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            step()
        ctx.sync()
        out.append((time.perf_counter() - t0) / (reps * members) * 1e6)
    return float(np.median(out)), float(min(out)), float(max(out))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256,1024")
    ap.add_argument("--out")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--package-root",
                    default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args(argv)
    sys.path.insert(0, args.package_root)
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    sizes = [int(s) for s in args.sizes.split(",")]
    opts, funs = build_members(safeopt_amd, gpy, max(sizes))
    ctx = opts[0]._backend.ctx
    np.random.seed(1)          # the measurement noise: the same runs in every process
    lines = []

    def report(**rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for state, n in (("growing", 3), ("converged", 20)):
        advance(opts, funs, n)
        for B in sizes:
            sub = opts[:B]

            def loop():
                for o in sub:
                    o.optimize()
            rec = dict(state=state, n=n, B=B)
            rec["loop_us"] = timed(loop, ctx, B)
            if not args.loop_only:
                fleet = safeopt_amd.SafeOptFleet(sub)
                rec["fleet_us"] = timed(fleet.optimize, ctx, B)
                visits = []
                inner = safeopt_amd.SafeOpt._visit_candidates

                def counting(self, *a, **k):
                    visits.append(1)
                    return inner(self, *a, **k)
                safeopt_amd.SafeOpt._visit_candidates = counting
                try:
                    fleet.optimize()
                finally:
                    safeopt_amd.SafeOpt._visit_candidates = inner
                rec["continued_alone"] = len(visits)
            report(**rec)
    if not args.loop_only:
        # whole BO iterations from the converged state (the states move on: done last; the
        # slices overlap, so the members of a later slice have up to 12 observations more)
        for B in sizes:
            sub, fsub = opts[:B], funs[:B]
            fleet = safeopt_amd.SafeOptFleet(sub)
            fleet.optimize()
            t_opt, t_add = [], []
            for _ in range(3):
                ctx.sync()
                t0 = time.perf_counter()
                X = fleet.optimize()
                t1 = time.perf_counter()
                for o, f, x in zip(sub, fsub, X):
                    o.add_new_data_point(x, f(x))
                ctx.sync()
                t2 = time.perf_counter()
                t_opt.append((t1 - t0) / B * 1e6)
                t_add.append((t2 - t1) / B * 1e6)
            ns = [int(o.gp.X.shape[0]) for o in sub]
            report(state="bo_iteration", B=B, n_after=[min(ns), max(ns)],
                   optimize_us=[float(np.median(t_opt)), min(t_opt), max(t_opt)],
                   add_new_data_point_us=[float(np.median(t_add)), min(t_add), max(t_add)])
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
