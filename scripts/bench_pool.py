#!/usr/bin/env python
"""Cost of one more measurement at a row the GP already holds (``pool_repeats``), and of a whole
run with and without pooling.

    python scripts/bench_pool.py [--sizes 64,500,2000] [--reps 9] [--out profiles/pool/SUMMARY.txt]

The driver (no ``--step``) starts every measurement as a child process under its own ``timeout``
and checks every exit status; after a child that aborted, faulted or ran into its limit nothing
more is started, and what could not be run is written down as "not measured".

1. Refresh cost (``--step refresh --n N``; the driver runs it twice per n, in two processes: the
   difference of the two is the run-to-run spread).  Three Matern-5/2 GPs on one set of inputs
   (bench.make_config(3) with n rows) on the 1000 x 1000 grid, ``--reps`` times, alternating in
   one process:

     pool    ``add_new_data_point`` at an input the GPs hold, on a ``pool_repeats`` SafeOpt
             (``pool_data`` = one ``sgp_gp_reweigh`` per GP) + ``confidence`` (which takes
             ``sgp_grid_rank1_reweigh``);
     append  ``add_new_data_point`` at a new input on a twin without pooling (``sgp_gp_append``
             per GP) + ``confidence`` (``sgp_grid_rank1_update``) -- the code of the parent
             commit: its kernels are unchanged (profiles/pool/isa_diff.txt).

   Host-clock milliseconds around work that ends in the read-back of max l0[S], a stream
   synchronise.  Between two timed steps the measurement is taken back (untimed) and the streak
   counter reset, so that every timed ``confidence`` is a refresh.  The first repetition is
   dropped; median [min .. max] of the rest.

2. Run cost (``--step run --rows N --steps K``).  The 1-d problem of tests/test_gpu_pooling.py
   (RBF(2, 1), noise sd 0.1, f = sin(1.5 x) + 0.3 x + 0.8, fmin 0, beta 2) on N grid rows: two
   optimisers, appending and pooling, fed the picks of the appending one; n of each GP and the
   host ms of each ``optimize()``, averaged over windows of the run.
"""
import argparse, os, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

#: exit statuses after which nothing more is started on the device
FATAL = (124, 134, 137, 139, -6, -9, -11)


def refresh(n, reps):
    import bench
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    cfg = bench.make_config(3)
    rng = np.random.default_rng(40 + n)
    X = rng.uniform(-2.0, 2.0, size=(n, cfg["d"]))
    Y = np.empty((n, cfg["G"]))
    for g in range(cfg["G"]):
        f = bench._bumps(X, 102 + g)
        Y[:, g] = f - f.min() + 0.5
    Y += 0.05 * rng.normal(size=Y.shape)
    cfg["X"], cfg["Y"], cfg["n"] = X, Y, n

    def make(pool):
        gps = bench.build_gps(cfg, gpy)
        opt = safeopt_amd.SafeOpt(gps, cfg["grid"], cfg["fmin"], threshold=cfg["threshold"],
                                  beta=cfg["beta"], pool_repeats=pool)
        opt._backend.confidence(cfg["beta"], opt.fmin)
        return opt

    pooled, plain = make(True), make(False)
    bp, ba, beta = pooled._backend, plain._backend, cfg["beta"]
    ctx = bp.ctx
    pool_ms, app_ms = [], []
    for rep in range(reps + 1):
        row = int(rng.integers(n))
        x_old, x_new = X[row], rng.uniform(-2.0, 2.0, size=cfg["d"])
        y = Y[row] + 0.05 * rng.normal(size=cfg["G"])
        bp._rank1_streak = ba._rank1_streak = 0
        ctx.sync()
        t0 = time.perf_counter()
        pooled.add_new_data_point(x_old[None, :], y[None, :])
        bp.confidence(beta, pooled.fmin)
        pool_ms.append((time.perf_counter() - t0) * 1e3)
        assert all(dv.reweighed and dv.n == n for dv in bp._dev()) and bp._rank1_streak == 1
        t0 = time.perf_counter()
        plain.add_new_data_point(x_new[None, :], y[None, :])
        ba.confidence(beta, plain.fmin)
        app_ms.append((time.perf_counter() - t0) * 1e3)
        assert all(dv.appended and dv.n == n + 1 for dv in ba._dev()) and ba._rank1_streak == 1
        for o in (pooled, plain):                   # taken back, untimed
            o.remove_last_data_point()
            o._backend.confidence(beta, o.fmin)

    def fmt(v):
        v = np.array(v[1:])
        return "%8.3f [%7.3f .. %7.3f]" % (np.median(v), v.min(), v.max())
    print("n = %4d  pool %s ms   append %s ms   pool / append %5.2f"
          % (n, fmt(pool_ms), fmt(app_ms), np.median(pool_ms[1:]) / np.median(app_ms[1:])),
          flush=True)


def run(rows, steps):
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    sd = 0.1

    def f(x):
        x = np.atleast_2d(x)
        return np.sin(1.5 * x[:, :1]) + 0.3 * x[:, :1] + 0.8

    rng = np.random.default_rng(0)
    y0 = float(f([[0.0]])[0, 0] + sd * rng.normal())
    grid = np.linspace(-3, 3, rows)[:, None]

    def make(pool):
        gp = gpy.models.GPRegression(np.zeros((1, 1)), np.array([[y0]]), gpy.kern.RBF(1, 2.0, 1.0),
                                     noise_var=sd ** 2)
        return safeopt_amd.SafeOpt(gp, grid, 0.0, beta=2, threshold=0, pool_repeats=pool)

    plain, pooled = make(False), make(True)
    ms = {False: [], True: []}
    ns = {False: [], True: []}
    ctx = plain._backend.ctx
    for _ in range(steps):
        picks = {}
        for pool, opt in ((False, plain), (True, pooled)):
            ctx.sync()
            t0 = time.perf_counter()
            picks[pool] = opt.optimize()
            ms[pool].append((time.perf_counter() - t0) * 1e3)
            ns[pool].append(opt.gp.X.shape[0])
        x = picks[False]
        y = f(x) + sd * rng.normal()
        plain.add_new_data_point(x, y)
        pooled.add_new_data_point(x, y)
    distinct = len(set(map(bytes, np.ascontiguousarray(plain.x))))
    print("%d grid rows, %d steps: the appending GP ends with n = %d, the pooling GP with n = %d "
          "(%d distinct inputs)" % (rows, steps, plain.gp.X.shape[0], pooled.gp.X.shape[0], distinct),
          flush=True)
    w = max(1, steps // 6)
    for s in range(0, steps, w):
        e = min(s + w, steps)
        print("   steps %3d .. %3d   append: n = %3d  %7.3f ms / optimize()   pool: n = %3d  "
              "%7.3f ms / optimize()" % (s, e - 1, ns[False][e - 1], np.median(ms[False][s:e]),
                                         ns[True][e - 1], np.median(ms[True][s:e])), flush=True)


def drive(sizes, reps, out):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    steps = [("refresh n = %d, process %d" % (n, p), ["--step", "refresh", "--n", str(n)], 420)
             for n in sizes for p in (1, 2)]
    steps += [("run, 200 rows, 60 steps", ["--step", "run", "--rows", "200", "--steps", "60"], 180),
              ("run, 1000 rows, 300 steps", ["--step", "run", "--rows", "1000", "--steps", "300"],
               300)]
    say("pool_data + interval update against add_new_data_point + interval update (rank-1 append),"
        " 3 GPs (Matern52, d = 2, one set of inputs), 1e6 rows; host ms, median [min .. max] of %d;"
        " two processes per n" % reps)
    stopped = None
    for label, args, limit in steps:
        if stopped is not None:
            say("%s: not measured (nothing is started after %s)" % (label, stopped))
            continue
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
               "--reps", str(reps)] + args
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            for line in r.stdout.strip().split("\n"):
                say(line)
        else:
            say("%s: not measured (exit status %d)" % (label, r.returncode))
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            if r.returncode in FATAL or "illegal memory access" in r.stderr:
                stopped = "%s (exit status %d)" % (label, r.returncode)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if stopped is None else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,500,2000")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=["refresh", "run"], default=None)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--steps", type=int, default=60)
    a = ap.parse_args()
    if a.step == "refresh":
        refresh(a.n, a.reps)
    elif a.step == "run":
        run(a.rows, a.steps)
    else:
        sys.exit(drive([int(s) for s in a.sizes.split(",")], a.reps, a.out))


if __name__ == "__main__":
    main()
