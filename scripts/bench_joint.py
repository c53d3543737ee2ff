#!/usr/bin/env python
"""Cost of a joint prediction (``full_cov=True``) and of posterior sample paths.

    python scripts/bench_joint.py [--cases 500x4096,2000x8192] [--reps 5] [--out FILE]

Per (n training points, N points), Matern52-ARD at d = 2: milliseconds and algorithmic fp64
TFLOP/s of the four device phases -- whitening V = L^-1 k(X, X*) (n^2 N flop), the SYRK
Sigma = k(X*, X*) - V^T V (N^2 n, the lower triangle counted once), the Cholesky factorisation
(N^3 / 3) and a 16-sample draw mean + C Z (N^2 S) -- from the per-launch hipEvents of
``sgp_profile_*`` (the phases of one C call are told apart by calls that stop earlier: mean
only, mean + covariance, draws of 16 and 32 columns); the whole calls with ``sgp_timer_*`` and
the host clock (uploads and the N x N read-back included); the VALU GEMM of the factorisation
doing the SYRK's product (a second process with SGP_JOINT_SYRK=valu, ``--valu-child``); and the
same computation with NumPy / LAPACK on the host (tests/_joint_numpy.py).  Prints one JSON
line and a table; ``--out`` writes both to a file.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctypes as C
import numpy as np
import safeopt_amd.gpy as gpy
from safeopt_amd import _hip

PEAK_TFLOPS = 78.6
NOISE = 0.05 ** 2


def problem(n, N):
    rng = np.random.default_rng(n + N)
    X = rng.uniform(-3, 3, (n, 2))
    Y = (np.sin(X / [0.9, 1.5]).sum(1) + 0.05 * rng.normal(size=n))[:, None]
    Xs = rng.uniform(-3, 3, (N, 2))
    return X, Y, Xs


def profiled(ctx, fn, reps):
    """Median over reps of (summed kernel-event ms, hipEvent ms of the whole call, host ms)."""
    rows = []
    for i in range(reps + 1):
        ctx.sync()
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        ctx.timer_start()
        fn()
        ev = ctx.timer_stop()
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctx.profile_read()[0]
        ctx.profile_enable(False)
        if i:
            rows.append((ms, ev, wall))
    return tuple(float(np.median([r[k] for r in rows])) for k in range(3))


def device_case(n, N, reps):
    ctx = _hip.Context.default()
    X, Y, Xs = problem(n, N)
    gp = gpy.models.GPRegression(X, Y, gpy.kern.Matern52(2, 1.7, [0.9, 1.5], ARD=True),
                                 noise_var=NOISE)
    dev = gp._fitted()
    mean = np.empty(N)

    def mean_only():
        ctx.check(_hip.lib().sgp_gp_predict_cov(dev.h, _hip.dptr(Xs), N, 2, 1,
                                                _hip.dptr(mean), None))
    Z16 = np.random.default_rng(1).normal(size=(N, 16))
    Z32 = np.random.default_rng(1).normal(size=(N, 32))
    jit = []
    w = profiled(ctx, mean_only, reps)
    c = profiled(ctx, lambda: dev.predict_cov(Xs), reps)
    d16 = profiled(ctx, lambda: jit.append(dev.draw(Xs, Z16)[2]), reps)
    d32 = profiled(ctx, lambda: dev.draw(Xs, Z32), reps)
    return {"n": n, "N": N, "jitter_used": float(jit[-1]),
            "whiten_ms": w[0], "syrk_ms": c[0] - w[0],
            "draw16_ms": d32[0] - d16[0], "chol_ms": d16[0] - c[0] - (d32[0] - d16[0]),
            "predict_cov_event_ms": c[1], "predict_cov_wall_ms": c[2],
            "draw16_event_ms": d16[1], "draw16_wall_ms": d16[2]}


def host_case(n, N):
    from oracle import gp_numpy as gpn
    from _joint_numpy import joint_posterior
    X, Y, Xs = problem(n, N)
    g = gpn.GPRegression(X, Y, gpn.Matern52(2, 1.7, [0.9, 1.5], ARD=True), noise_var=NOISE)
    t0 = time.perf_counter()
    mean, cov = joint_posterior(g, Xs)
    t1 = time.perf_counter()
    L = gpn.jitchol(cov)
    t2 = time.perf_counter()
    out = mean + L.dot(np.random.default_rng(1).normal(size=(N, 16)))
    t3 = time.perf_counter()
    return {"host_cov_ms": (t1 - t0) * 1e3, "host_chol_ms": (t2 - t1) * 1e3,
            "host_draw16_ms": (t3 - t2) * 1e3, "host_threads": os.environ.get("OMP_NUM_THREADS")}


def tflops(flop, ms):
    return flop / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="500x4096,2000x8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--valu-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",")]
    if a.valu_child:        # SGP_JOINT_SYRK=valu is set: only the SYRK phase is of interest
        rows = [device_case(n, N, a.reps) for n, N in cases]
        print(json.dumps([{"n": r["n"], "N": r["N"], "syrk_valu_ms": r["syrk_ms"]} for r in rows]))
        return
    rows = []
    for n, N in cases:
        r = device_case(n, N, a.reps)
        if not a.no_host:
            r.update(host_case(n, N))
        rows.append(r)
    # the VALU yardstick needs the switch read at load time: a fresh child process
    env = dict(os.environ, SGP_JOINT_SYRK="valu")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--valu-child", "--cases",
                            a.cases, "--reps", str(a.reps)], env=env, capture_output=True,
                           text=True, timeout=600)
    if child.returncode == 0:
        for r, v in zip(rows, json.loads(child.stdout.strip().splitlines()[-1])):
            r["syrk_valu_gemm_ms"] = v["syrk_valu_ms"]
    else:
        sys.stderr.write(child.stderr[-2000:])
    lines = []
    for r in rows:
        n, N = r["n"], r["N"]
        fl = {"whiten": 1.0 * n * n * N, "syrk": 1.0 * N * N * n, "chol": N ** 3 / 3.0,
              "draw16": 1.0 * N * N * 16}
        for k, f in fl.items():
            r[k + "_tflops"] = tflops(f, r[k + "_ms"])
        if "syrk_valu_gemm_ms" in r:
            r["syrk_valu_gemm_tflops"] = tflops(fl["syrk"], r["syrk_valu_gemm_ms"])
        lines.append("n = %d, N = %d (Matern52-ARD, d = 2; jitter_used = %g)" % (n, N, r["jitter_used"]))
        for k in ("whiten", "syrk", "chol", "draw16"):
            lines.append("  %-8s %9.3f ms  %7.3f TFLOP/s  (%.1f %% of %.1f)"
                         % (k, r[k + "_ms"], r[k + "_tflops"],
                            100 * r[k + "_tflops"] / PEAK_TFLOPS, PEAK_TFLOPS))
        if "syrk_valu_gemm_ms" in r:
            lines.append("  syrk product on the VALU k_gemm: %9.3f ms  %7.3f TFLOP/s"
                         % (r["syrk_valu_gemm_ms"], r["syrk_valu_gemm_tflops"]))
        lines.append("  predict_cov call: %.1f ms (events) / %.1f ms (host clock);  16-sample draw call:"
                     " %.1f / %.1f ms" % (r["predict_cov_event_ms"], r["predict_cov_wall_ms"],
                                          r["draw16_event_ms"], r["draw16_wall_ms"]))
        if "host_cov_ms" in r:
            lines.append("  NumPy / LAPACK on the host (%s threads): mean + cov %.1f ms, Cholesky %.1f ms,"
                         " draw %.1f ms" % (r["host_threads"], r["host_cov_ms"], r["host_chol_ms"],
                                            r["host_draw16_ms"]))
    line = json.dumps({"bench": "joint", "rows": rows})
    print(line)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
