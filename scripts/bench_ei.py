#!/usr/bin/env python
"""Cost of one log-expected-improvement pass (``sgp_grid_ei``, csrc/ei.hip).

    python scripts/bench_ei.py [--rows 1000000] [--n 500] [--reps 30] [--gpus N]
                               [--out profiles/ei/SUMMARY.txt]

The config-3 shape: a 1000 x 1000 grid, 3 GPs (objective and two constraints) of n = 500
observations, Matern52-ARD at d = 2.  Milliseconds per ``sgp_grid_ei`` call over ``S`` (host clock
around the call, which ends in the read-back of the pick: incumbent reduction, row pass, final
kernel; median, minimum and maximum of ``--reps`` calls after one warm-up) and of the row kernel
alone by the per-launch hipEvents of ``sgp_profile_*``, for ``kind`` in {ei, pi} x ``feasibility`` in
{off, on}.  Beside them, in the same run on the same grid, ``sgp_grid_mes`` with K = 1: the same
pass structure (reduction over ``S``, one thread per row, arg-max epilogue, one read-back) with one
erfcx, one exp and one log per row.  No time is a target: the table records the ratio to that
pass.  ``--gpus N`` starts N ranks, one per GPU, each with its shard of the rows
(``sgp_grid_ei_comm``, ``sgp_grid_mes_comm``); rank 0 reports.  Without ``--out`` nothing is
written; a time that was not measured is written as "not measured".
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

NOISE = 0.05 ** 2
HBM_RATE = 6.3e12                    # bytes per second


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


def spawn(n, argv):
    """``--gpus N``: N ranks, one per GPU, in the torchrun-style environment
    ``dist.init_from_env`` reads (as scripts/bench_mes.py starts them); rank 0 prints."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    nonce = "%d-%x" % (os.getpid(), int(time.time() * 1e6))
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SAFEOPT_RDZV_NONCE=nonce)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv,
                                      env=env, stdout=subprocess.PIPE if r == 0 else
                                      subprocess.DEVNULL, text=True))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out)
    if any(rcs):
        sys.exit("ranks exited with %r" % (rcs,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, dist
    ctx, comm = dist.init_from_env()
    side = int(round(a.rows ** 0.5))
    grid_rows = safeopt_amd.linearly_spaced_combinations([(-5., 5.)] * 2, side)
    N = grid_rows.shape[0]
    rng = np.random.RandomState(0)
    X = rng.uniform(-5, 5, (a.n, 2))
    f0 = 2.0 + np.sin(X / [0.9, 1.5]).sum(1)
    Ys = [f0, 1.0 + np.cos(X / [1.3, 0.8]).sum(1), 1.5 - 0.05 * (X ** 2).sum(1)]
    gps = [gpy.models.GPRegression(X, (y + 0.05 * rng.standard_normal(a.n))[:, None],
                                   gpy.kern.Matern52(2, 1.7, [0.9, 1.5], ARD=True),
                                   noise_var=NOISE) for y in Ys]
    fmin = [0.0, -0.5, -0.5]
    opt = safeopt_amd.SafeOpt(gps, grid_rows, fmin, threshold=0.2, comm=comm)
    opt.update_confidence_intervals()
    opt.compute_safe_set()
    n_safe = int(np.asarray(opt.S).sum())
    be = opt._backend
    multi = comm.world > 1
    in_stream = multi and getattr(comm, "in_stream", False)
    rows, picks = {}, {}
    if not multi or in_stream:
        for kind, code in (("ei", _hip.EI_EI), ("pi", _hip.EI_PI)):
            for feas in (False, True):
                call = lambda: be.ei(code, _hip.MES_S, 'mean', 0.0, fmin if feas else None,
                                     comm=multi)
                key = "%s, feasibility %s" % (kind, "on" if feas else "off")
                picks[key] = call()[1:]
                rows[key] = (host_ms(ctx, call, a.reps), event_ms(ctx, call, a.reps))
        mes = lambda: be.mes([3.0], _hip.MES_S, 'mean', comm=multi)
        mes()
        rows["mes, K = 1"] = (host_ms(ctx, mes, a.reps), event_ms(ctx, mes, a.reps))
    comm.barrier()
    if comm.rank:
        return
    n_local = be.grid.N
    fmt = lambda t: "%8.4f  (%.4f .. %.4f)" % t
    lines = [
        "sgp_grid_ei over S, %d rows (d = 2)%s, 3 GPs of n = %d, Matern52-ARD, |S| = %d; ms, median "
        "(minimum .. maximum) of %d calls after one warm-up"
        % (N, " over %d ranks (%d rows a rank)" % (comm.world, n_local) if multi else "", a.n,
           n_safe, a.reps),
        "  %-24s %-34s %-34s" % ("", "whole call (host clock)", "row kernel alone (hipEvents)")]
    if rows:
        base = rows["mes, K = 1"]
        for key in sorted(rows, key=lambda k: (k.startswith("mes"), k)):
            h, e = rows[key]
            lines.append("  %-24s %-34s %-34s call / MES = %.2f, kernel / MES = %.2f"
                         % (key, fmt(h), fmt(e), h[0] / base[0][0], e[0] / base[1][0]))
    else:
        lines.append("  not measured (the host transport of this communicator runs the pass through "
                     "ei_point only)")
    lines += [
        "one read of the rows at %.1f TB/s: mask only %.4f ms; mean, var of one GP and the mask over "
        "S %.4f ms; of three GPs %.4f ms"
        % (HBM_RATE / 1e12, n_local / HBM_RATE * 1e3, (n_local + 16.0 * n_safe) / HBM_RATE * 1e3,
           (n_local + 48.0 * n_safe) / HBM_RATE * 1e3),
        "counters of k_ei_grid (VALU busy, memory stalls): not measured"]
    line = json.dumps({"bench": "ei", "gpus": comm.world, "rows": N, "n": a.n, "safe": n_safe,
                       "ms": {k: {"call": v[0], "kernel": v[1]} for k, v in rows.items()},
                       "picks": {k: [float(v[0]), int(v[1]), float(v[2])]
                                 for k, v in picks.items()}})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
