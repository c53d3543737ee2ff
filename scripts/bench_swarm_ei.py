#!/usr/bin/env python
"""Cost of ``SafeOptSwarm.ei_point`` at config-5 scale (``sgp_swarm_run_ei``, k_swarm_ei in
csrc/ei.hip).

    python scripts/bench_swarm_ei.py [--particles 100000] [--iters 100] [--reps 3] [--gpus N]
                                     [--out profiles/swarm_ei/SUMMARY.txt]

Config 5 of bench.py: 4-D RBF, G = 2, n = 2000 observations, a swarm of 1e5 particles,
``pso='device-rng'`` (nothing but the swarm state crosses PCIe).  Milliseconds, median (min ..
max) of ``--reps`` after one warm-up, of

* one ``sgp_swarm_fitness_ei`` call of the whole swarm's size with ``alpha = post = NULL``, on
  the host clock, with and without the feasibility weights;
* the k_swarm_ei launch of such a call alone, from the library's per-launch hipEvents (the term
  is the last timed launch of the call, ``sgp_profile_read_last``), next to the whole timed part
  of the call (the posterior sweep in front of it) -- with and without weights, and its share;
* for comparison, from the same process, one ``sgp_swarm_fitness_mes`` call at K = 1 and its
  k_swarm_mes launch;
* a whole ``ei_point()`` (the incumbent, one swarm run, the pick) and ONE maximizers swarm run
  of the same length (``init_swarm`` + ``run_swarm``).

``--gpus N`` starts N ranks, one per GPU, and splits every swarm over them
(``SafeOptSwarm(..., comm=)``, ``sgp_swarm_run_ei_shard``); rank 0 reports.
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
    dctx = opt.gp._fitted().ctx
    rng = np.random.default_rng(2)
    box = cfg["box"]
    particles = rng.uniform(-box, box, size=(a.particles, cfg["d"]))
    tau = float(np.max(opt.gp.predict_noiseless(opt.S)[0]))

    def timed(call):
        """(host ms, term ms, timed ms of the call, launches), medians over the repetitions."""
        host, term, tot_ms = [], [], []
        launches = 0
        for i in range(a.reps + 1):
            dctx.profile_enable(True)
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            k = dctx.profile_read_last()
            tot, launches, _ = dctx.profile_read()
            dctx.profile_enable(False)
            if i:
                host.append(dt)
                term.append(k)
                tot_ms.append(tot)
        return (float(np.median(host)), float(np.median(term)), float(np.median(tot_ms)),
                int(launches), term)

    fit = {}
    for name, weigh in (("ei", False), ("ei_weighed", True)):
        fit[name] = timed(lambda: opt._compute_ei_fitness(('ei', tau, 0.0, weigh, False),
                                                          particles))
    fit["mes_K1"] = timed(lambda: opt._compute_mes_fitness((np.array([tau + 1.0]), tau),
                                                           particles))
    last = {}

    def ei_point():
        np.random.seed(1)
        last["ei"] = opt.ei_point(return_state=True)

    def maximizers():
        np.random.seed(1)
        sw = opt.swarms['maximizers']
        sw.init_swarm(opt._initial_particles('maximizers'))
        sw.run_swarm(a.iters)

    e_ms = times_ms(ei_point, a.reps)
    m_ms = times_ms(maximizers, a.reps)
    if comm.rank:
        return
    x, alpha, st = last["ei"]
    res = {"bench": "swarm_ei", "gpus": comm.world, "particles": a.particles, "n": cfg["n"],
           "G": cfg["G"], "d": cfg["d"], "iters": a.iters, "reps": a.reps,
           "ei_point_ms": list(e_ms), "maximizers_run_ms": list(m_ms), "alpha": alpha,
           "tau": st["tau"]}
    lines = ["SafeOptSwarm.ei_point, %d particles (d = %d), n = %d, G = %d, RBF-ARD, "
             "pso='device-rng', %d rank(s); ms, median of %d after one warm-up"
             % (a.particles, cfg["d"], cfg["n"], cfg["G"], comm.world, a.reps)]
    names = {"ei": "sgp_swarm_fitness_ei, no weights, alpha = post = NULL",
             "ei_weighed": "sgp_swarm_fitness_ei, weights of %d GPs" % cfg["G"],
             "mes_K1": "sgp_swarm_fitness_mes, K = 1 (for comparison)"}
    for key in ("ei", "ei_weighed", "mes_K1"):
        host, term, tot, launches, all_terms = fit[key]
        res[key] = {"call_host_ms": host, "term_ms": term, "term_ms_all": all_terms,
                    "timed_ms": tot, "timed_launches": launches,
                    "term_share_of_host_call": term / host, "term_share_of_timed": term / tot}
        lines.append("%-55s host clock %8.3f ms; term launch (hipEvents; all: %s) %.4f ms; "
                     "the %d timed launches (posterior sweep + term) %.3f ms; term = %.3f %% of "
                     "the call, %.3f %% of its timed launches"
                     % (names[key], host, ", ".join("%.4f" % v for v in all_terms), term,
                        launches, tot, 100.0 * term / host, 100.0 * term / tot))
    lines += ["ei_point(), %d iterations (host clock):                  %10.1f (%.1f .. %.1f) ms"
              % ((a.iters,) + e_ms),
              "one maximizers swarm run (init + %d iterations):         %10.1f (%.1f .. %.1f) ms"
              % ((a.iters,) + m_ms)]
    line = json.dumps(res)
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
