#!/usr/bin/env python
"""Cost of one information-theoretic safe exploration pick (``SafeOpt.ise_point``, csrc/ise.hip).

    python scripts/bench_ise.py [--rows 1000000] [--n 500] [--gps 3] [--K 64,256,1024]
                                [--reps 5] [--gpus N] [--out profiles/ise/SUMMARY.txt]

The config-3 shape: a 1000 x 1000 grid, 3 Matern52-ARD GPs at d = 2 with n = 500 observations
each, every fmin finite.  Per K: milliseconds per ``ise_point`` (host clock around the call,
which ends in the read-back of the pick; median, minimum and maximum of ``--reps`` calls after
one warm-up), split into the candidate selection -- on the device (``SafeOpt._ise_select``: keys,
histogram, list, each one pass over the resident variances and S and one round trip, then the
exact ordering of the listed rows on the host) and, for comparison, the host selection it replaces
(one download of the variances and of S, a partition: what a package without the device selection
runs, and the fall-back of this one) --, the device pass (``sgp_grid_ise``: gather, operands, rows,
final kernels, one read-back) on the host clock, and the row kernel alone by the per-launch
hipEvents of ``sgp_profile_*``; the operand stage is the device pass minus the row kernel.  Beside
the row kernel the arithmetic floor ``2 N n_pad K G_active`` flop at the fp64 matrix peak, beside
the selection passes the HBM floor of their reads, and beside the whole call the time of a
converged ``optimize()`` on the same state (no existing kernel takes part in ``ise_point``, and
``ise_point`` changes none of them).  ``--gpus N`` starts N ranks, one per GPU, as
scripts/bench_mes.py does: the grid is row-sharded, the selection agrees over the ranks, every rank
evaluates all candidates against its rows (``sgp_grid_ise_at`` / ``_comm``) and rank 0 reports its
own times.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_MFMA_F64 = 78.6e12              # flop per second
HBM_RATE = 8.0e12                    # bytes per second
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
    ap.add_argument("--gps", type=int, default=3)
    ap.add_argument("--K", default="64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    Ks = [int(k) for k in a.K.split(",")]
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, dist, gp_opt
    from safeopt_amd.gp_opt import ise_candidates
    ctx, comm = dist.init_from_env()
    multi = comm.world > 1
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
                              fmin if a.gps > 1 else 0.0, threshold=0.2, comm=comm)
    opt.optimize()
    step = host_ms(ctx, opt.optimize, a.reps)            # converged: no new data in between
    be = opt._backend
    n_safe = int(np.asarray(opt.S).sum())
    n_pad = (a.n + 15) // 16 * 16
    fm = np.asarray(fmin, dtype=float)
    active = np.isfinite(fm)
    on_device = hasattr(be, "ise_keys")          # (a package from before the device selection)
    in_stream = multi and getattr(comm, "in_stream", False)
    n_local = be.grid.N
    # one selection pass reads var (G_active words a row) and S; the list pass reads them twice
    hbm_ms = (8.0 * a.gps + 1.0) * n_local / HBM_RATE * 1e3
    per_k = {}
    for K in Ks:
        x, alpha = opt.ise_point(candidates=K)
        r = {"ise_point_ms": host_ms(ctx, lambda: opt.ise_point(candidates=K), a.reps)}
        if on_device:
            r["path"] = opt._ise_path
            r["select_device_ms"] = host_ms(ctx, lambda: opt._ise_select(K, fm, active), a.reps)
            _n, lo, hi = opt._ise_safe_count(fm)
            hist = be.ise_hist(fm, lo, hi).astype(np.float64)
            if multi:
                hist = comm.allgather(hist).sum(axis=0)
            thr, listed = gp_opt.ise_threshold(hist, min(K, n_safe), lo, hi)
            _c, gi, _k, _x, lv = be.ise_list(fm, thr, listed + 64)
            r["listed"] = int(listed)
            r["keys_ms"] = host_ms(ctx, lambda: be.ise_keys(fm), a.reps)
            r["hist_ms"] = host_ms(ctx, lambda: be.ise_hist(fm, lo, hi), a.reps)
            r["list_ms"] = host_ms(ctx, lambda: be.ise_list(fm, thr, listed + 64), a.reps)
            r["order_ms"] = host_ms(
                ctx, lambda: gp_opt.ise_order(gi, lv, be.ise_noise(), active, K), a.reps)
        if multi:
            rows, xc, vx = opt._ise_select(K, fm, active)
            call = lambda: be.ise_at(fm, rows, xc, vx, _hip.ISE_UNSAFE, comm=in_stream)
        else:
            var, S, s = be.ise_state()
            rows = ise_candidates(var, S, s, active, K)

            def select():
                v, S_, s_ = be.ise_state()
                return ise_candidates(v, S_, s_, active, K)
            r["select_ms"] = host_ms(ctx, select, a.reps)
            call = lambda: be.ise(fm, rows, _hip.ISE_UNSAFE)
        r["pass_ms"] = host_ms(ctx, call, a.reps)
        r["row_kernel_ms"] = event_ms(ctx, call, a.reps)
        r["operands_ms"] = r["pass_ms"][0] - r["row_kernel_ms"][0]
        r["floor_ms"] = 2.0 * n_local * n_pad * rows.size * a.gps / PEAK_MFMA_F64 * 1e3
        r["candidates"] = int(rows.size)
        r["alpha"], r["x"] = float(alpha), [float(v) for v in x]
        per_k[K] = r
    comm.barrier()
    if comm.rank:
        return
    fmt = lambda t: "%.3f  (%.3f .. %.3f)" % t
    lines = [
        "SafeOpt.ise_point, %d rows (d = 2)%s, %d Matern52-ARD GPs (all active), n = %d, |S| = %d, "
        "about = 'unsafe'; ms, median (minimum .. maximum) of %d calls after one warm-up"
        % (N, " over %d ranks (%d rows a rank, %s merge; rank 0's times)"
           % (comm.world, n_local, "in-stream" if in_stream else "host") if multi else "",
           a.gps, a.n, n_safe, a.reps),
        "converged optimize() on the same state (host clock)     %s" % fmt(step)]
    for K in Ks:
        r = per_k[K]
        lines += [
            "K = %d candidates" % r["candidates"],
            "  ise_point, whole call (host clock)                    %s" % fmt(r["ise_point_ms"])]
        if on_device:
            lines += [
                "    candidate selection on the device (%s)%s %s"
                % (r["path"], " " * max(0, 14 - len(r["path"])), fmt(r["select_device_ms"])),
                "      sgp_grid_ise_keys (count, min, max)               %s" % fmt(r["keys_ms"]),
                "      sgp_grid_ise_hist (4096 bins)                     %s" % fmt(r["hist_ms"]),
                "      sgp_grid_ise_list (%5d rows listed)             %s"
                % (r["listed"], fmt(r["list_ms"])),
                "      exact ordering of the listed rows on the host     %s" % fmt(r["order_ms"]),
                "      HBM floor of one pass over var and S at %.1f TB/s   %.4f ms"
                % (HBM_RATE / 1e12, hbm_ms)]
        if "select_ms" in r:
            lines.append(
                "    candidate selection on the host (download, sort)%s %s"
                % (": not on the call's path" if on_device else "   ", fmt(r["select_ms"])))
        lines += [
            "    device pass (sgp_grid_ise%s)                     %s"
            % ("_comm" if in_stream else "_at  " if multi else "     ", fmt(r["pass_ms"])),
            "      k_ise_rows alone (hipEvents)                      %s" % fmt(r["row_kernel_ms"]),
            "      gather, operand kernels, final kernels, read-back %.3f  (pass - rows, medians)"
            % r["operands_ms"],
            "  arithmetic floor 2 N n_pad K G / %.1f TF                %.3f ms;  k_ise_rows / floor"
            " = %.2f" % (PEAK_MFMA_F64 / 1e12, r["floor_ms"], r["row_kernel_ms"][0] / r["floor_ms"])]
    lines.append("counters of k_ise_rows (MFMA busy, VALU busy, stalls): not measured")
    line = json.dumps({"bench": "ise", "gpus": comm.world, "rows": N, "n": a.n, "gps": a.gps,
                       "safe": n_safe,
                       "optimize_ms": step, "K": {str(k): v for k, v in per_k.items()}})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
