#!/usr/bin/env python
"""Cost of ``SafeOptSwarm.ise_point`` at config-5 scale (``sgp_swarm_run_ise``, k_swarm_ise in
csrc/swarm_ise.hip).

    python scripts/bench_swarm_ise.py [--particles 100000] [--T 64,256,1024] [--iters 100]
                                      [--reps 3] [--gpus N]
                                      [--out profiles/swarm_ise/SUMMARY.txt]

Config 5 of bench.py: 4-D RBF, G = 2 (both active), n = 2000 observations, a swarm of 1e5
particles, ``pso='device-rng'`` (nothing but the swarm state crosses PCIe).  Milliseconds on the
host clock, median (min .. max) of ``--reps`` after one warm-up, of

* ``ise_point(targets=T, about='all')`` per T: the targets' posterior, the operands, the swarm
  and its pick (``'all'``: the filter drops nothing, so the swarm really runs against T targets);
* ONE maximizers swarm run of the same length (``init_swarm`` + ``run_swarm``).

Then k_swarm_ise alone from the library's per-launch hipEvents: the term is the last timed
launch of a ``sgp_swarm_fitness_ise`` call (``sgp_profile_read_last``), next to the whole timed
part of that call (the posterior sweep in front of it).  The yardstick is k_ise_rows, the row
kernel of ``sgp_grid_ise``, on the same GPs with the particles as the N = P grid rows and K = T
candidates (``about = all``): per (row, column, GP) the two kernels do the same evaluation, the
same MFMAs and the same term.  One rank only (``--gpus N`` leaves it out and says so).
``--gpus N`` starts N ranks, one per GPU, and splits the swarm over them
(``SafeOptSwarm(..., comm=)``, ``sgp_swarm_run_ise_shard``); rank 0 reports.
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
    ap.add_argument("--T", default="64,256,1024")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    Ts = [int(t) for t in a.T.split(",")]
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, dist
    from bench import make_config, build_gps
    ctx, comm = dist.init_from_env()
    cfg = make_config(5)
    box, d = cfg["box"], cfg["d"]
    np.random.seed(0)
    opt = safeopt_amd.SafeOptSwarm(build_gps(cfg, gpy), cfg["fmin"], bounds=[(-box, box)] * d,
                                   threshold=cfg["threshold"], swarm_size=a.particles,
                                   pso='device-rng', comm=comm)
    opt.max_iters = a.iters
    dctx = opt.gp._fitted().ctx
    rng = np.random.default_rng(2)
    particles = rng.uniform(-box, box, size=(a.particles, d))
    fm = np.asarray(opt.fmin, dtype=float)

    def maximizers():
        np.random.seed(1)
        sw = opt.swarms['maximizers']
        sw.init_swarm(opt._initial_particles('maximizers'))
        sw.run_swarm(a.iters)

    m_ms = times_ms(maximizers, a.reps)
    grid_opt = None
    if comm.world == 1:
        # the yardstick's grid: the particles as rows, the same GPs
        grid_opt = safeopt_amd.SafeOpt(opt.gps, particles, list(fm), threshold=cfg["threshold"])
        grid_opt.update_confidence_intervals()
    per_t = {}
    for T in Ts:
        last = {}

        def ise():
            np.random.seed(1)
            last["r"] = opt.ise_point(targets=T, about='all', return_state=True)

        r = {"ise_point_ms": times_ms(ise, a.reps)}
        x, alpha, st = last["r"]
        targets = (st["targets"], st["zmean"], st["zvar"])
        kern, call = [], []
        for i in range(a.reps + 1):
            dctx.profile_enable(True)
            opt._compute_ise_fitness(targets, particles)
            k = dctx.profile_read_last()
            tot, launches, _ = dctx.profile_read()
            dctx.profile_enable(False)
            if i:
                kern.append(k)
                call.append(tot)
        r.update(k_swarm_ise_ms=float(np.median(kern)), k_swarm_ise_ms_all=kern,
                 fitness_call_timed_ms=float(np.median(call)), timed_launches=int(launches),
                 alpha=alpha, T=int(st["targets"].shape[0]))
        if grid_opt is not None:
            be = grid_opt._backend
            rows = np.arange(T, dtype=np.int64)
            rowk = []
            for i in range(a.reps + 1):
                dctx.sync()
                dctx.profile_enable(True)
                be.ise(fm, rows, _hip.ISE_ALL)
                t = dctx.profile_read()[0]
                dctx.profile_enable(False)
                if i:
                    rowk.append(t)
            r.update(k_ise_rows_ms=float(np.median(rowk)), k_ise_rows_ms_all=rowk,
                     ratio=float(np.median(kern) / np.median(rowk)))
        per_t[T] = r
    if comm.rank:
        return
    lines = ["SafeOptSwarm.ise_point, %d particles (d = %d), n = %d, G = %d (all active), RBF-ARD, "
             "pso='device-rng', %d rank(s); host clock ms, median (min .. max) of %d"
             % (a.particles, d, cfg["n"], cfg["G"], comm.world, a.reps),
             "one maximizers swarm run (init + %d iterations):            %10.1f (%.1f .. %.1f) ms"
             % ((a.iters,) + m_ms)]
    for T in Ts:
        r = per_t[T]
        pairs = float(a.particles) * r["T"] * cfg["G"] / comm.world
        lines += ["T = %d targets (about='all')" % r["T"],
                  "  ise_point, %d iterations:                                  %10.1f (%.1f .. %.1f) ms"
                  % ((a.iters,) + r["ise_point_ms"]),
                  "  k_swarm_ise, this rank's particles (hipEvents, median of %d; all: %s): %.3f ms"
                  " = %.3f ns per (particle, target, GP)"
                  % (a.reps, ", ".join("%.3f" % v for v in r["k_swarm_ise_ms_all"]),
                     r["k_swarm_ise_ms"], r["k_swarm_ise_ms"] * 1e6 / pairs),
                  "  the timed launches of that fitness call (%d: posterior sweep + k_swarm_ise): "
                  "%.3f ms" % (r["timed_launches"], r["fitness_call_timed_ms"])]
        if "k_ise_rows_ms" in r:
            lines += ["  k_ise_rows, N = %d rows, K = %d candidates, same GPs (all: %s): %.3f ms"
                      " = %.3f ns per pair;  k_swarm_ise / k_ise_rows = %.2f (wanted <= 1.5)"
                      % (a.particles, r["T"], ", ".join("%.3f" % v for v in r["k_ise_rows_ms_all"]),
                         r["k_ise_rows_ms"], r["k_ise_rows_ms"] * 1e6 / pairs, r["ratio"])]
        else:
            lines += ["  k_ise_rows: not measured on %d ranks (the yardstick is a one-rank run)"
                      % comm.world]
    res = {"bench": "swarm_ise", "gpus": comm.world, "particles": a.particles, "n": cfg["n"],
           "G": cfg["G"], "d": d, "iters": a.iters, "reps": a.reps,
           "maximizers_run_ms": list(m_ms),
           "per_T": {str(T): {k: (list(v) if isinstance(v, tuple) else v)
                              for k, v in per_t[T].items()} for T in Ts}}
    line = json.dumps(res)
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
