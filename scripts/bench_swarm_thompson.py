#!/usr/bin/env python
"""Cost of ``SafeOptSwarm.thompson_points`` at config-5 scale (``sgp_swarm_run_path``,
k_swarm_path in csrc/paths.hip).

    python scripts/bench_swarm_thompson.py [--particles 100000] [--size 8] [--features 1024]
                                           [--iters 100] [--reps 3] [--gpus N]
                                           [--out profiles/swarm_thompson/SUMMARY.txt]

Config 5 of bench.py: 4-D RBF, G = 2, n = 2000 observations, a swarm of 1e5 particles,
``pso='device-rng'`` (nothing but the swarm state crosses PCIe).  Milliseconds (host clock,
median of ``--reps`` after one warm-up) per ``thompson_points(size)`` -- ``size`` swarm runs of
``iters`` iterations, the draw of the paths and the picks included -- next to the milliseconds of
ONE maximizers swarm run of the same length (``init_swarm`` + ``run_swarm``), and per iteration
the time of a Thompson swarm over that of a maximizers swarm: what the path term adds.
``--gpus N`` starts N ranks, one per GPU, and splits every swarm over them
(``SafeOptSwarm(..., comm=)``, ``sgp_swarm_run_path_shard``); rank 0 reports.
"""
import argparse, json, os, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def median_ms(fn, reps):
    ms = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def spawn(n, argv):
    """``--gpus N``: N ranks, one per GPU, in the torchrun-style environment
    ``dist.init_from_env`` reads (as scripts/swarm_optimize.py starts them); rank 0 prints."""
    import socket, subprocess
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
    ap.add_argument("--particles", type=int, default=100000)
    ap.add_argument("--size", type=int, default=8)
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import dist
    from bench import make_config, build_gps
    ctx, comm = dist.init_from_env()
    cfg = make_config(5)
    np.random.seed(0)
    opt = safeopt_amd.SafeOptSwarm(build_gps(cfg, gpy), cfg["fmin"],
                                   bounds=[(-cfg["box"], cfg["box"])] * cfg["d"],
                                   threshold=cfg["threshold"], swarm_size=a.particles,
                                   pso='device-rng', comm=comm)
    opt.max_iters = a.iters

    def thompson():
        np.random.seed(1)
        opt.thompson_points(size=a.size, features=a.features)

    def maximizers():
        np.random.seed(1)
        sw = opt.swarms['maximizers']
        sw.init_swarm(opt._initial_particles('maximizers'))
        sw.run_swarm(a.iters)

    t_ms = median_ms(thompson, a.reps)
    m_ms = median_ms(maximizers, a.reps)
    per_t = t_ms / (a.size * (a.iters + 1))
    per_m = m_ms / (a.iters + 1)
    if comm.rank:
        return
    res = {"bench": "swarm_thompson", "gpus": comm.world, "particles": a.particles, "n": cfg["n"], "G": cfg["G"],
           "d": cfg["d"], "size": a.size, "features": a.features, "iters": a.iters,
           "thompson_points_ms": t_ms, "maximizers_run_ms": m_ms,
           "thompson_ms_per_iteration": per_t, "maximizers_ms_per_iteration": per_m}
    lines = ["SafeOptSwarm.thompson_points, %d particles (d = %d), n = %d, G = %d, RBF-ARD, "
             "pso='device-rng', %d rank(s); host clock ms, median of %d"
             % (a.particles, cfg["d"], cfg["n"], cfg["G"], comm.world, a.reps),
             "thompson_points(size=%d, features=%d), %d iterations per swarm: %10.1f ms"
             % (a.size, a.features, a.iters, t_ms),
             "one maximizers swarm run (init + %d iterations):               %10.1f ms"
             % (a.iters, m_ms),
             "per fitness evaluation of the swarm: thompson %.3f ms, maximizers %.3f ms "
             "(ratio %.2f; paths drawn and picks made inside the thompson figure)"
             % (per_t, per_m, per_t / per_m)]
    line = json.dumps(res)
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
