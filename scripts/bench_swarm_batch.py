#!/usr/bin/env python
"""Cost of a hallucinated swarm run (``sgp_swarm_run_hall``, csrc/swarm_batch.hip) next to the
plain one (``sgp_swarm_run``) in the same run, with the same particles, GPs and iterations.

    python scripts/bench_swarm_batch.py [--iters 20] [--repeats 5] [--out profiles/swarm_batch/SUMMARY.txt]
    python scripts/bench_swarm_batch.py --gpus N [--iters 20] [--picks 4] [--particles 100000] [--out FILE]

Two sizes: config 5's swarm (bench.make_config(5): d = 4, G = 2 GPs of n = 2000 observations,
1e5 particles) and SafeOptSwarm's default on the same data cut to n = 20 (20 particles); per
size b = 1, 8, 63 pending picks on clones of the GPs.  Every figure is the milliseconds of ONE
call (init + ``--iters`` iterations of an expanders swarm, device generator, state up and down
included) between two hipEvents on the context's stream; ``--repeats`` calls behind a dropped
first one (allocations, code upload), the median of the rest.  At 20 particles the plain run
takes the one-workgroup step of a small swarm and a hallucinated run the general launches: the
ratio there compares launch counts, not arithmetic.

Work per particle, GP and fitness call: the real posterior forms n^2 / 2 multiply-adds of the
variance contraction on the matrix pipe and n covariance evaluations; the downdate adds b (n +
b) FMAs and (n + b) ceil(b / 16) covariance evaluations on the fp64 VALU -- about 2 b / n of
the contraction's flops.

``--gpus N`` starts N ranks (one per GPU, torchrun-style environment, as
scripts/swarm_optimize.py does) and measures the product instead: ``SafeOptSwarm(...,
comm=).optimize_batch(size=picks + 1, max_iters=iters)`` at config 5's sizes,
``pso='device-rng'``, the hallucinated swarms split over the ranks by particle
(``sgp_swarm_run_hall_shard``).  Rank 0 prints the host milliseconds per pick for that rank
count -- the two hallucinated swarms of a pick with their start draws, the recheck of the
gathered personal bests and the choice -- with the first pick dropped.  ``--gpus 1`` gives the
one-rank figure of the same measurement; without ``--gpus`` the table above is produced.
"""
import argparse, json, os, socket, subprocess, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def one_size(label, n, P, bs, iters, repeats):
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    from bench import make_config, build_gps
    cfg = make_config(5, side=P)
    cfg["X"], cfg["Y"], cfg["n"] = cfg["X"][:n], cfg["Y"][:n], n
    gps = build_gps(cfg, gpy)
    devs = [g._fitted() for g in gps]
    ctx = devs[0].ctx
    d, G = cfg["d"], cfg["G"]
    start = np.ascontiguousarray(cfg["particles"] * 0.5)
    fmin, scaling = np.array(cfg["fmin"]), np.sqrt([2.0] * G)
    vscale, bounds = np.full(d, 0.1), np.array([(-5., 5.)] * d)
    pend = np.random.default_rng(3).uniform(-2.5, 2.5, size=(max(bs), d))

    def timed(clones):
        ms = []
        for r in range(repeats + 1):
            st = [start.copy(), np.empty((P, d)), np.empty((P, d)), np.empty(P), np.empty(d)]
            tail = (np.broadcast_to(vscale, (d,)), bounds, True, iters, 1.0, -0.6 / max(iters, 1),
                    None)
            ctx.timer_start()
            if clones is None:
                _hip.swarm_run(ctx, devs, "expanders", cfg["beta"], fmin, scaling, 0.0, *st, *tail,
                               seed=7)
            else:
                _hip.swarm_run_hall(ctx, devs, clones, "expanders", cfg["beta"], fmin, scaling,
                                    0.0, *st, *tail, seed=7)
            ms.append(ctx.timer_stop())
        return float(np.median(ms[1:])), ms

    plain_ms, plain_all = timed(None)
    rows = []
    for b in bs:
        clones = [dv.clone() for dv in devs]
        try:
            for x in pend[:b]:
                assert all([c.append(x, 0.0) for c in clones])
            hall_ms, hall_all = timed(clones)
        finally:
            for c in clones:
                c.destroy()
        rows.append({"size": label, "P": P, "n": n, "G": G, "d": d, "b": b, "iters": iters,
                     "plain_ms": plain_ms, "hall_ms": hall_ms, "ratio": hall_ms / plain_ms,
                     "flop_ratio_2b_over_n": 2.0 * b / n, "plain_all_ms": plain_all,
                     "hall_all_ms": hall_all})
    return rows


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


def main_product(a):
    """``optimize_batch`` of the swarm product on the ranks of the launch."""
    import safeopt_amd as sa
    import safeopt_amd.gpy as gpy
    from safeopt_amd import dist, gp_opt
    from bench import make_config, build_gps
    ctx, comm = dist.init_from_env()
    cfg = make_config(5, side=1000)
    picks = []                                   # per pick: the side swarms' host seconds
    side = gp_opt.SafeOptSwarm._side_swarm_pick

    def timed(self, swarm, *args, **kw):
        hall = swarm is not None and getattr(swarm, "_type", None) in ("maximizers", "expanders")
        t0 = time.perf_counter()
        try:
            return side(self, swarm, *args, **kw)
        finally:
            if hall:
                if swarm._type == "maximizers":
                    picks.append(0.0)
                picks[-1] += time.perf_counter() - t0
    gp_opt.SafeOptSwarm._side_swarm_pick = timed
    np.random.seed(11)
    opt = sa.SafeOptSwarm(build_gps(cfg, gpy), cfg["fmin"], bounds=[(-5., 5.)] * 4,
                          threshold=cfg["threshold"], swarm_size=a.particles, pso="device-rng",
                          comm=comm)
    opt.max_iters = a.iters                      # (the real step in front: not what is timed)
    ctx.sync()
    comm.barrier()
    X = opt.optimize_batch(size=a.picks + 1, max_iters=a.iters)
    ms = [p * 1e3 for p in picks]
    res = {"bench": "swarm_batch_nrank", "gpus": comm.world, "particles": a.particles,
           "n": cfg["n"], "G": cfg["G"], "d": cfg["d"], "iters": a.iters, "picks": len(ms),
           "points": int(X.shape[0]),
           "ms_per_pick": float(np.median(ms[1:])) if len(ms) > 1 else float("nan"),
           "ms_all": ms}
    comm.barrier()
    if comm.rank != 0:
        return
    lines = ["one pick of SafeOptSwarm.optimize_batch on %d ranks (two hallucinated swarms of %d "
             "particles, init + %d iterations each, split by particle): host ms, median of the "
             "picks behind the first" % (comm.world, a.particles, a.iters),
             "ranks  particles      n  G  picks  ms per pick",
             "%5d %10d %6d %2d %6d %12.3f" % (comm.world, a.particles, cfg["n"], cfg["G"],
                                              res["picks"], res["ms_per_pick"])]
    line = json.dumps(res)
    print(line)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bs", default="1,8,63")
    ap.add_argument("--gpus", type=int, default=0,
                    help="N >= 1: the product on N ranks, ms per pick (default: the run table)")
    ap.add_argument("--picks", type=int, default=4)
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus >= 1:
        if a.gpus > 1 and "RANK" not in os.environ:
            return spawn(a.gpus, sys.argv[1:])
        return main_product(a)
    bs = [int(b) for b in a.bs.split(",")]
    res = one_size("config5", 2000, 100000, bs, a.iters, a.repeats) + \
        one_size("default", 20, 20, bs, a.iters, a.repeats)
    lines = ["sgp_swarm_run_hall next to sgp_swarm_run in the same run: one call = init + %d iterations of "
             "an expanders swarm, ms between hipEvents, median of %d calls behind a dropped first one"
             % (a.iters, a.repeats),
             "size        P      n  G   b   plain ms    hall ms   ratio   2b/n"]
    for r in res:
        lines.append("%-8s %6d %6d %2d %3d %10.3f %10.3f %7.3f %6.3f" % (
            r["size"], r["P"], r["n"], r["G"], r["b"], r["plain_ms"], r["hall_ms"], r["ratio"],
            r["flop_ratio_2b_over_n"]))
    lines.append("(plain at 20 particles: the one-workgroup step of a small swarm, two launches per "
                 "iteration; a hallucinated run takes the general launches -- move, downdate, posterior, "
                 "shaping, bests, global best -- so its ratio there is launch count, not arithmetic.)")
    line = json.dumps({"bench": "swarm_batch", "rows": res})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
