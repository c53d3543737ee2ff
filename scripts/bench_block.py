#!/usr/bin/env python
"""From the first added row to current intervals: ``b`` measurements entering the model by three
routes, at config-3 scale (three Matern-5/2 GPs on one set of inputs, n = 500, 1e6 rows).

    python scripts/bench_block.py [--n 500] [--blocks 2,4,8,16] [--reps 9] [--out profiles/block/SUMMARY.txt]

Per block size ``b``, ``--reps`` + 1 times, the three routes alternating in one process, each on
an optimiser of its own that holds the same data and a current resident posterior:

  (a)  ``b`` x ``add_new_data_point``, then ``update_confidence_intervals``: every GP is ``b``
       versions behind, so the interval update is a full sweep (the route of the parent commit);
  (b)  ``b`` x (``add_new_data_point`` + ``update_confidence_intervals``): ``b`` rank-1 refreshes;
  (c)  ``add_new_data_points`` + ``update_confidence_intervals``: one block append per GP and one
       rank-b refresh.

Host-clock milliseconds around work that ends in the read-back of max l0[S] (a stream
synchronise); the context is synchronised in front of every timed window.  Between two timed
windows the ``b`` rows are taken out again (untimed: a refit of the first n rows and a sweep) and
the streak counter is reset, so every timed window starts from the same state and routes (b)
and (c) take their refreshes.  The first repetition (allocations, code upload) is dropped;
median [min .. max] of the rest, and the run-to-run spread (max - min) / median per route.  All
three optimisers hold the same data after every window: max |Q - Q_(a)| is printed as a check.
The whole table is measured twice in the same process (``--passes``) so that the difference
between two passes of the same route can be read next to the difference between routes.
"""
import argparse, os, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def problem(n, bmax):
    import bench
    cfg = bench.make_config(3)
    rng = np.random.default_rng(70 + n)
    X = rng.uniform(-2.0, 2.0, size=(n + bmax, cfg["d"]))
    Y = np.empty((n + bmax, cfg["G"]))
    for g in range(cfg["G"]):
        f = bench._bumps(X, 102 + g)
        Y[:, g] = f - f.min() + 0.5
    Y += 0.05 * rng.normal(size=Y.shape)
    cfg["X"], cfg["Y"], cfg["n"] = X[:n], Y[:n], n
    return cfg, X[n:], Y[n:]


def run(n, blocks, reps, say):
    import bench
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    cfg, Xn, Yn = problem(n, max(blocks))
    X0, Y0 = cfg["X"].copy(), cfg["Y"].copy()

    def make():
        gps = bench.build_gps(cfg, gpy)
        opt = safeopt_amd.SafeOpt(gps, cfg["grid"], cfg["fmin"], threshold=cfg["threshold"],
                                  beta=cfg["beta"])
        opt.update_confidence_intervals()
        return opt

    def reset(opt):
        """Back to the first n rows with a swept posterior (untimed)."""
        for g, gp in enumerate(opt.gps):
            gp.set_XY(X0, Y0[:, [g]])
        opt._x, opt._y = X0.copy(), Y0.copy()
        opt.update_confidence_intervals()
        assert opt._backend._rank1_streak == 0

    def route_a(opt, b):
        for r in range(b):
            opt.add_new_data_point(Xn[r], Yn[r])
        opt.update_confidence_intervals()

    def route_b(opt, b):
        for r in range(b):
            opt.add_new_data_point(Xn[r], Yn[r])
            opt.update_confidence_intervals()

    def route_c(opt, b):
        opt.add_new_data_points(Xn[:b], Yn[:b])
        opt.update_confidence_intervals()

    routes = (("a", route_a, 0), ("b", route_b, None), ("c", route_c, None))
    opts = {name: make() for name, _, _ in routes}
    ctx = opts["a"]._backend.ctx
    rows = {}
    for b in blocks:
        ms = {name: [] for name, _, _ in routes}
        qdiff = 0.0
        for _ in range(reps + 1):
            for name, fn, _ in routes:
                opt = opts[name]
                ctx.sync()
                t0 = time.perf_counter()
                fn(opt, b)
                ms[name].append((time.perf_counter() - t0) * 1e3)
            # (a) swept, (b) and (c) refreshed: b rows on the streak
            assert opts["a"]._backend._rank1_streak == 0
            assert opts["b"]._backend._rank1_streak == b and opts["c"]._backend._rank1_streak == b
            assert all(dv.block == b for dv in opts["c"]._backend._dev())
            Qa = opts["a"]._backend.download(_hip.Q)
            for name in ("b", "c"):
                qdiff = max(qdiff, float(np.max(np.abs(opts[name]._backend.download(_hip.Q) - Qa))))
            for opt in opts.values():
                reset(opt)
        rows[b] = {name: np.array(v[1:]) for name, v in ms.items()}
        line = "b = %2d " % b
        for name, _, _ in routes:
            v = rows[b][name]
            line += "  (%s) %8.3f [%7.3f .. %7.3f] spread %4.1f %%" % (
                name, np.median(v), v.min(), v.max(), 100.0 * (v.max() - v.min()) / np.median(v))
        say(line + "   max|dQ| %.1e" % qdiff)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--blocks", default="2,4,8,16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    blocks = [int(s) for s in a.blocks.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("b measurements -> current intervals, 3 GPs (Matern52, d = 2, one set of inputs), n = %d, "
        "1e6 rows; host ms, median [min .. max] of %d" % (a.n, a.reps))
    say("(a) b x add, one sweep   (b) b x (add + rank-1 refresh)   (c) block append + rank-b refresh")
    passes = []
    for p in range(a.passes):
        say("pass %d" % (p + 1))
        passes.append(run(a.n, blocks, a.reps, say))
    if len(passes) > 1:
        say("pass-to-pass difference of the medians (same route, same code):")
        for b in blocks:
            say("b = %2d " % b + "".join(
                "  (%s) %5.1f %%" % (name, 100.0 * abs(np.median(passes[0][b][name]) -
                                                       np.median(passes[-1][b][name]))
                                     / np.median(passes[0][b][name])) for name in "abc"))
    say("(c) against (b), medians of the last pass: " + "  ".join(
        "b = %d: %.2f x" % (b, np.median(passes[-1][b]["c"]) / np.median(passes[-1][b]["b"]))
        for b in blocks))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
