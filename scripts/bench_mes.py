#!/usr/bin/env python
"""Cost of one max-value entropy search pick (``SafeOpt.mes_point``, csrc/mes.hip).

    python scripts/bench_mes.py [--rows 1000000] [--n 500] [--paths 16] [--features 1024]
                                [--reps 30] [--gpus N] [--out profiles/mes/SUMMARY.txt]

The config-3 shape: a 1000 x 1000 grid, n = 500 observations, Matern52-ARD at d = 2, K = 16
maxima.  Milliseconds per ``mes_point`` (host clock around the call, which ends in the read-back
of the pick; median, minimum and maximum of ``--reps`` calls after one warm-up), split into drawing the paths and their
data weights, the path maxima over S (``sgp_grid_paths``) and the MES pass (``sgp_grid_mes``: floor
reduction, row pass, final kernel, one read-back), each on the host clock, and the row kernel
alone by the per-launch hipEvents of ``sgp_profile_*``.  Beside the row kernel two floors that
can be derived: one read of mean, var and the mask byte (17 bytes a row) at the HBM rate
DESIGN.md section 4.3 uses, and K terms a row at the fp64 VALU instructions of the term loop,
counted in the kernel's ISA (every branch of the loop counted once: a wave whose lanes agree on
the sign of gamma and on erfcx's range executes fewer).  ``--gpus N`` starts N ranks, one per
GPU, each with its shard of the rows (``sgp_grid_paths_comm``, ``sgp_grid_mes_comm``); rank 0
reports.  A time that was not measured is written as "not measured".
"""
import argparse, json, os, re, subprocess, sys, tempfile, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_VALU_F64 = 78.6e12 / 2          # fp64 VALU instructions (lanes) per second: FMA = 2 flop
HBM_RATE = 6.3e12                    # bytes per second
ROW_BYTES = 17                       # mean, var, one mask byte
NOISE = 0.05 ** 2


def isa_counts():
    """fp64 VALU instructions of the term loop of k_mes_grid: the basic blocks the listing marks
    as part of the kernel's only loop (the loop over the K maxima).  Raises when the toolchain
    or the kernel is missing."""
    sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
    import isa_stats
    from safeopt_amd import build as B
    src = os.path.join(B.CSRC, "mes.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "mes.s")
        r = subprocess.run([B._hipcc()] + B.BASE + B.EXTRA.get("mes.hip", []) +
                           ["-S", "--cuda-device-only", src, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc -S of mes.hip failed:\n" + r.stderr[-2000:])
        found = [t for name, t in isa_stats.kernels(out) if name.endswith("k_mes_grid")]
    if len(found) != 1:
        raise RuntimeError("k_mes_grid not found in the listing of mes.hip")
    f64 = lambda t: len(re.findall(r"\n\tv_\w+_f64", "\n" + t))
    blocks = re.split(r"\n(?=\.LBB\d+_\d+:|; %bb\.\d+:)", found[0])
    loop = [b for b in blocks if "Loop" in "\n".join(b.split("\n")[:2])]
    if not loop:
        raise RuntimeError("k_mes_grid: no loop block in the listing")
    return {"term_loop_f64_valu": sum(f64(b) for b in loop),
            "term_loop_blocks_f64_valu": [f64(b) for b in loop],
            "term_loop_instructions": sum(len(re.findall(r"\n\t[sv]_\w+", "\n" + b)) for b in loop),
            "kernel_f64_valu": f64(found[0])}


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
    ``dist.init_from_env`` reads (as scripts/bench_paths.py starts them); rank 0 prints."""
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
    ap.add_argument("--paths", type=int, default=16)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    # before any GPU time: raises without toolchain or kernel (rank 0 reports: it alone counts)
    isa = isa_counts() if os.environ.get("RANK", "0") == "0" else None
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, dist
    ctx, comm = dist.init_from_env()
    side = int(round(a.rows ** 0.5))
    grid_rows = safeopt_amd.linearly_spaced_combinations([(-5., 5.)] * 2, side)
    N = grid_rows.shape[0]
    rng = np.random.RandomState(0)
    X = rng.uniform(-5, 5, (a.n, 2))
    Y = (2.0 + np.sin(X / [0.9, 1.5]).sum(1) + 0.05 * rng.standard_normal(a.n))[:, None]
    gp = gpy.models.GPRegression(X, Y, gpy.kern.Matern52(2, 1.7, [0.9, 1.5], ARD=True),
                                 noise_var=NOISE)
    opt = safeopt_amd.SafeOpt(gp, grid_rows, 0.0, threshold=0.2, comm=comm)
    opt.update_confidence_intervals()
    opt.compute_safe_set()
    n_safe = int(np.asarray(opt.S).sum())
    be = opt._backend
    multi = comm.world > 1
    in_stream = multi and getattr(comm, "in_stream", False)
    np.random.seed(0)

    def pick():
        return opt.mes_point(paths=a.paths, features=a.features)
    x, alpha = pick()
    total = host_ms(ctx, pick, a.reps)
    draw = host_ms(ctx, lambda: gp.posterior_paths(size=a.paths, features=a.features), a.reps)
    pp = gp.posterior_paths(size=a.paths, features=a.features)
    rows = {"mes_point_ms": total, "draw_ms": draw}
    if not multi or in_stream:
        _, ystar, _ = be.paths(pp, True, False, comm=multi)
        rows["path_maxima_ms"] = host_ms(ctx, lambda: be.paths(pp, True, False, comm=multi),
                                         a.reps)
        rows["mes_pass_ms"] = host_ms(
            ctx, lambda: be.mes(ystar, _hip.MES_S, 'mean', comm=multi), a.reps)
        rows["row_kernel_ms"] = event_ms(
            ctx, lambda: be.mes(ystar, _hip.MES_S, 'mean', comm=multi), a.reps)
    comm.barrier()
    if comm.rank:
        return
    n_local = be.grid.N
    fmt = lambda k: "%.3f  (%.3f .. %.3f)" % rows[k] if k in rows else "not measured"
    hbm_ms = ROW_BYTES * n_local / HBM_RATE * 1e3
    valu_ms = isa["term_loop_f64_valu"] * float(a.paths) * n_local / PEAK_VALU_F64 * 1e3
    lines = [
        "SafeOpt.mes_point, %d rows (d = 2)%s, n = %d, Matern52-ARD, K = %d paths of %d features, "
        "|S| = %d; ms, median (minimum .. maximum) of %d calls after one warm-up"
        % (N, " over %d ranks (%d rows a rank)" % (comm.world, n_local) if multi else "", a.n,
           a.paths, a.features, n_safe, a.reps),
        "  mes_point, whole call (host clock)                  %s" % fmt("mes_point_ms"),
        "    posterior_paths: draws and data weights           %s" % fmt("draw_ms"),
        "    path maxima over S (sgp_grid_paths%s)         %s"
        % ("_comm" if multi else "     ", fmt("path_maxima_ms")),
        "    MES pass (sgp_grid_mes%s: floor, rows, final)  %s"
        % ("_comm" if multi else "     ", fmt("mes_pass_ms")),
        "      k_mes_grid alone (hipEvents)                    %s" % fmt("row_kernel_ms"),
        "floors of k_mes_grid over %d rows:" % n_local,
        "  HBM: %d bytes a row (mean, var, mask) at %.1f TB/s                      %.4f ms"
        % (ROW_BYTES, HBM_RATE / 1e12, hbm_ms),
        "  fp64 VALU: K = %d terms a row, %d fp64 VALU instructions in the term loop of the ISA "
        "(all branches; %d instructions in all), at %.1f T lane-instructions / s   %.4f ms"
        % (a.paths, isa["term_loop_f64_valu"], isa["term_loop_instructions"],
           PEAK_VALU_F64 / 1e12, valu_ms)]
    if "row_kernel_ms" in rows:
        med = rows["row_kernel_ms"][0]
        lines.append("  k_mes_grid (median) / fp64 VALU floor = %.2f, / HBM floor = %.1f"
                     % (med / valu_ms, med / hbm_ms))
    lines.append("counters of k_mes_grid (VALU busy, stalls): not measured")
    line = json.dumps({"bench": "mes", "gpus": comm.world, "rows": N, "n": a.n, "K": a.paths,
                       "features": a.features, "safe": n_safe, "ms": rows, "isa": isa,
                       "floors_ms": {"hbm": hbm_ms, "valu_f64": valu_ms},
                       "alpha": float(alpha), "x": [float(v) for v in x]})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
