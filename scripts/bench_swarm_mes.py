#!/usr/bin/env python
"""Cost of ``SafeOptSwarm.mes_point`` at config-5 scale (``sgp_swarm_run_mes``, k_swarm_mes in
csrc/mes.hip).

    python scripts/bench_swarm_mes.py [--particles 100000] [--paths 16] [--features 1024]
                                      [--iters 100] [--reps 3] [--gpus N]
                                      [--out profiles/swarm_mes/SUMMARY.txt]

Config 5 of bench.py: 4-D RBF, G = 2, n = 2000 observations, a swarm of 1e5 particles,
``pso='device-rng'`` (nothing but the swarm state crosses PCIe).  Milliseconds on the host
clock, median (min .. max) of ``--reps`` after one warm-up, of

* ``mes_point(paths)``: the ``paths`` Thompson swarms that give the maxima, the floor, the MES
  swarm and its pick;
* ``thompson_points(size=paths)`` alone -- the difference of the two is the MES swarm;
* ONE maximizers swarm run of the same length (``init_swarm`` + ``run_swarm``).

Then the time of k_swarm_mes itself from the library's per-launch hipEvents: the term is the
last timed launch of a ``sgp_swarm_fitness_mes`` call (``sgp_profile_read_last``), next to the
whole timed part of that call (the posterior sweep in front of it).
``--gpus N`` starts N ranks, one per GPU, and splits every swarm over them
(``SafeOptSwarm(..., comm=)``, ``sgp_swarm_run_mes_shard``); rank 0 reports.
"""
import argparse, json, os, sys, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def times_ms(fn, reps):
    """(median, min, max) of ``reps`` calls after one warm-up."""
    ms = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


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
    ap.add_argument("--paths", type=int, default=16)
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
    last = {}

    def mes():
        np.random.seed(1)
        last["mes"] = opt.mes_point(paths=a.paths, features=a.features, return_state=True)

    def thompson():
        np.random.seed(1)
        opt.thompson_points(size=a.paths, features=a.features)

    def maximizers():
        np.random.seed(1)
        sw = opt.swarms['maximizers']
        sw.init_swarm(opt._initial_particles('maximizers'))
        sw.run_swarm(a.iters)

    mes_ms = times_ms(mes, a.reps)
    t_ms = times_ms(thompson, a.reps)
    m_ms = times_ms(maximizers, a.reps)
    # the kernel alone: one fitness call of the whole swarm's size under the profile hooks
    x, alpha, st = last["mes"]
    dctx = opt.gp._fitted().ctx
    rng = np.random.default_rng(2)
    box = cfg["box"]
    particles = rng.uniform(-box, box, size=(a.particles, cfg["d"]))
    kern_ms, call_ms = [], []
    for i in range(a.reps + 1):
        dctx.profile_enable(True)
        opt._compute_mes_fitness((st["ystar"], st["floor"]), particles)
        k = dctx.profile_read_last()
        tot, launches, _ = dctx.profile_read()
        dctx.profile_enable(False)
        if i:
            kern_ms.append(k)
            call_ms.append(tot)
    if comm.rank:
        return
    k_med, c_med = float(np.median(kern_ms)), float(np.median(call_ms))
    res = {"bench": "swarm_mes", "gpus": comm.world, "particles": a.particles, "n": cfg["n"],
           "G": cfg["G"], "d": cfg["d"], "paths": a.paths, "features": a.features,
           "iters": a.iters, "reps": a.reps, "mes_point_ms": list(mes_ms),
           "thompson_points_ms": list(t_ms), "maximizers_run_ms": list(m_ms),
           "mes_swarm_ms": mes_ms[0] - t_ms[0], "k_swarm_mes_ms": k_med,
           "k_swarm_mes_ms_all": kern_ms, "fitness_call_timed_ms": c_med,
           "timed_launches": int(launches), "alpha": alpha}
    lines = ["SafeOptSwarm.mes_point, %d particles (d = %d), n = %d, G = %d, RBF-ARD, "
             "pso='device-rng', %d rank(s); host clock ms, median (min .. max) of %d"
             % (a.particles, cfg["d"], cfg["n"], cfg["G"], comm.world, a.reps),
             "mes_point(paths=%d, features=%d), %d iterations per swarm:  %10.1f (%.1f .. %.1f) ms"
             % ((a.paths, a.features, a.iters) + mes_ms),
             "thompson_points(size=%d) alone:                             %10.1f (%.1f .. %.1f) ms"
             % ((a.paths,) + t_ms),
             "difference = the MES swarm (floor, run, pick):              %10.1f ms"
             % (mes_ms[0] - t_ms[0]),
             "one maximizers swarm run (init + %d iterations):           %10.1f (%.1f .. %.1f) ms"
             % ((a.iters,) + m_ms),
             "k_swarm_mes, %d particles of this rank's call, K = %d (hipEvents, median of %d; "
             "all: %s): %.4f ms" % (a.particles, a.paths, a.reps,
                                    ", ".join("%.4f" % v for v in kern_ms), k_med),
             "the timed launches of that fitness call (%d: posterior sweep + k_swarm_mes): "
             "%.3f ms" % (launches, c_med)]
    line = json.dumps(res)
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
