#!/usr/bin/env python
"""Cost of one pick of ``SafeOpt.optimize_batch`` (``sgp_grid_batch_next``, csrc/batch.hip).

    python scripts/bench_batch.py [--configs 2,3] [--picks 8] [--out profiles/batch/SUMMARY.txt]
    python scripts/bench_batch.py --gpus N [--configs 2,3] [--picks 8] [--out FILE]

Per config (bench.make_config: 2 = RBF, G = 1, n = 200; 3 = Matern52, G = 3 on one set of inputs,
n = 500; both on the 1000 x 1000 grid): after one ``optimize()``, ``--picks`` hallucinated picks
on clones of the GPs.  Per pick the milliseconds of ``sgp_grid_batch_next`` between two
hipEvents on the context's stream (the row kernel, the final kernel and the 16-byte read-back)
and the host clock around the append to the clones plus that call.  Next to it, in the same run
and at the same n, ``sgp_grid_rank1_update`` on a twin optimiser whose GPs really receive the
same points: the closed-form refresh of the resident posterior does the same per-row work -- n
covariance evaluations and FMAs per row and group of GPs with one factor -- without the arg-max
and with the stores of mean, Q and S instead of var_h.  That figure is the comparison; the first
pick of each series (allocations, code upload) is dropped, the rest give the median.

``--gpus N`` starts N ranks (one per GPU, torchrun-style environment, as
scripts/swarm_optimize.py does): the grid is sharded over them and a pick is the N-rank one of
``optimize_batch`` -- ``sgp_grid_batch_next_comm`` with an in-stream communicator, else the
shard's ``sgp_grid_batch_next``, one all-gather and ``dist.merge_batch_records``.  Rank 0 prints
the host milliseconds per pick (the call alone, and with the appends to the clones) for that
rank count; the one-rank figures of the same session come from a run without ``--gpus``.
"""
import argparse, json, os, socket, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def one_config(k, picks):
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    from bench import make_config, build_gps
    cfg = make_config(k)

    def make():
        gps = build_gps(cfg, gpy)
        opt = safeopt_amd.SafeOpt(gps if len(gps) > 1 else gps[0], cfg["grid"],
                                  cfg["fmin"] if len(gps) > 1 else cfg["fmin"][0],
                                  threshold=cfg["threshold"], beta=cfg["beta"])
        x0 = opt.optimize()
        return opt, x0

    opt, x0 = make()
    twin, _ = make()
    ctx = opt._backend.ctx
    G, beta = len(opt.gps), cfg["beta"]
    row = int(opt._global_argmax(_hip.ARGMAX_MG_WIDTH)[1])
    assert np.array_equal(opt.inputs[row], x0)
    be, tb = opt._backend, twin._backend
    clones = [dv.clone() for dv in be._dev()]
    rows, pick_ms, pick_host_ms, rank1_ms = [row], [], [], []
    try:
        for b in range(1, picks + 1):
            x = opt.inputs[rows[-1]]
            t0 = time.perf_counter()
            if not all([c.append(x, 0.0) for c in clones]):
                break
            ctx.timer_start()
            _v, i = be.grid.batch_next(clones, b == 1, _hip.ARGMAX_MG_WIDTH, beta, opt.scaling, rows)
            pick_ms.append(ctx.timer_stop())
            pick_host_ms.append((time.perf_counter() - t0) * 1e3)
            # the same point, for real, on the twin: the rank-1 refresh at the same n
            twin.add_new_data_point(x, np.ones((1, G)))
            devs = tb._dev()
            assert all(dv.appended and dv.n == clones[0].n for dv in devs)
            ctx.timer_start()
            tb.grid.rank1_update(devs, [1] * G, beta, twin.fmin, defer=True)
            rank1_ms.append(ctx.timer_stop())
            if i < 0:
                break
            rows.append(int(i))
    finally:
        for c in clones:
            c.destroy()
    med = lambda v: float(np.median(v[1:])) if len(v) > 1 else float("nan")
    return {"config": k, "rows": int(opt.inputs.shape[0]), "G": G, "n": cfg["n"],
            "kind": cfg["kernels"][0][0]["kind"], "picks": len(pick_ms),
            "distinct_rows": len(set(rows)) == len(rows),
            "batch_next_ms": med(pick_ms), "append_plus_batch_next_host_ms": med(pick_host_ms),
            "rank1_update_ms": med(rank1_ms), "batch_next_all_ms": pick_ms,
            "rank1_update_all_ms": rank1_ms}


def spawn(n, argv):
    """One rank per GPU; rank 0's output is this process's."""
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
        raise SystemExit("rank exit codes: %s" % rcs)


def one_config_ranks(k, picks, ctx, comm):
    """The picks of ``optimize_batch`` on the ranks of ``comm``: host clock per pick."""
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    from bench import make_config, build_gps
    cfg = make_config(k)
    gps = build_gps(cfg, gpy)
    opt = safeopt_amd.SafeOpt(gps if len(gps) > 1 else gps[0], cfg["grid"],
                              cfg["fmin"] if len(gps) > 1 else cfg["fmin"][0],
                              threshold=cfg["threshold"], beta=cfg["beta"], comm=comm)
    opt.optimize()
    mode, beta, be = _hip.ARGMAX_MG_WIDTH, cfg["beta"], opt._backend
    rows = [int(opt._global_argmax(mode)[1])]
    clones = [dv.clone() for dv in be._dev()]
    pick_ms, host_ms = [], []
    try:
        for b in range(1, picks + 1):
            x = opt.inputs[rows[-1]]
            ctx.sync()
            comm.barrier()
            t0 = time.perf_counter()
            ok = all([c.append(x, 0.0) for c in clones])
            t1 = time.perf_counter()
            i, stop = be._pick_over_ranks(comm, clones, not ok, b == 1, mode, beta,
                                          opt.scaling, rows)
            t2 = time.perf_counter()
            pick_ms.append((t2 - t1) * 1e3)
            host_ms.append((t2 - t0) * 1e3)
            if stop or i < 0:
                break
            rows.append(int(i))
    finally:
        for c in clones:
            c.destroy()
    med = lambda v: float(np.median(v[1:])) if len(v) > 1 else float("nan")
    return {"config": k, "gpus": comm.world, "rows": int(opt.inputs.shape[0]),
            "rows_per_rank": int(be.grid.N), "G": len(opt.gps), "n": cfg["n"],
            "kind": cfg["kernels"][0][0]["kind"], "picks": len(pick_ms),
            "in_stream": bool(getattr(comm, "in_stream", False)),
            "distinct_rows": len(set(rows)) == len(rows), "pick_host_ms": med(pick_ms),
            "append_plus_pick_host_ms": med(host_ms), "pick_host_all_ms": pick_ms}


def main_ranks(a):
    from safeopt_amd import dist
    ctx, comm = dist.init_from_env()
    res = [one_config_ranks(int(k), a.picks, ctx, comm) for k in a.configs.split(",")]
    comm.barrier()
    if comm.rank != 0:
        return
    lines = ["one pick of SafeOpt.optimize_batch on %d ranks (the grid sharded by row; one record "
             "per rank gathered and merged per pick); host ms, median of the picks behind the first"
             % comm.world,
             "config  kernel     G     n       rows  rows/rank  ranks  picks  pick ms  "
             "append + pick ms"]
    for r in res:
        lines.append("%6d  %-9s %2d %5d %10d %10d %6d %6d %8.3f %17.3f" % (
            r["config"], r["kind"], r["G"], r["n"], r["rows"], r["rows_per_rank"], r["gpus"],
            r["picks"], r["pick_host_ms"], r["append_plus_pick_host_ms"]))
    line = json.dumps({"bench": "batch_nrank", "gpus": comm.world, "configs": res})
    print(line)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--picks", type=int, default=8)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1:
        if "RANK" not in os.environ:
            return spawn(a.gpus, sys.argv[1:])
        return main_ranks(a)
    res = [one_config(int(k), a.picks) for k in a.configs.split(",")]
    lines = ["sgp_grid_batch_next (one pick of SafeOpt.optimize_batch) next to sgp_grid_rank1_update at the "
             "same n in the same run; ms between hipEvents, median of the picks behind the first",
             "config  kernel     G     n       rows  picks  batch_next ms  rank1_update ms   ratio  "
             "append + batch_next, host ms"]
    for r in res:
        lines.append("%6d  %-9s %2d %5d %10d %6d %14.3f %16.3f %7.2f %30.3f" % (
            r["config"], r["kind"], r["G"], r["n"], r["rows"], r["picks"], r["batch_next_ms"],
            r["rank1_update_ms"], r["batch_next_ms"] / r["rank1_update_ms"],
            r["append_plus_batch_next_host_ms"]))
    lines.append("(batch_next: downdate of var_h for every GP, intervals, masked arg-max over M | G with the "
                 "picked rows excluded, final reduction, 16-byte read-back; rank1_update: downdate of mean and "
                 "var, Q, S and the partials of max l0[S], no read-back.  n grows by one per pick in both.)")
    line = json.dumps({"bench": "batch", "configs": res})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
