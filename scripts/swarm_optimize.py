#!/usr/bin/env python
"""Milliseconds per ``SafeOptSwarm.optimize()`` at config 5's sizes, split into phases.

d = 4, G = 2 GPs of n = 2000 observations (bench.py's config 5 data), 1e5 particles per
swarm, ``pso='device-rng'``, a fixed seed.  One ``optimize()`` = three swarm runs (greedy,
maximizers, expanders; init + 100 iterations each), two growth steps of the safe set and
the safe-set recheck / point predictions around them.  Reported per step:

  pso_ms     the swarm runs (DeviceSwarmOptimization._device_run)
  grow_ms    the growth of the safe set (SafeOptSwarm._grow_safe_set: sgp_swarm_grow)
  other_ms   the rest: safe-set recheck, point predictions, host work

``--gpus N`` starts N ranks (one per GPU, torchrun-style environment, as bench.py does)
and the swarms are split over them (``SafeOptSwarm(..., comm=)``); rank 0 prints one JSON
line.  Each step starts from the same state (same data, same seed), so steps differ only
in timing.

    python scripts/swarm_optimize.py [--gpus N] [--steps K] [--warmup W] [--particles P]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def spawn(n, argv):
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


def run(args):
    import safeopt_amd as sa
    import safeopt_amd.gpy as gpy
    from safeopt_amd import dist, gp_opt, swarm
    from bench import make_config, build_gps
    ctx, comm = dist.init_from_env()
    cfg = make_config(5, side=1000)
    phase = {"pso": 0.0, "grow": 0.0}

    def timed(name, f):
        def w(*a, **k):
            t0 = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                phase[name] += time.perf_counter() - t0
        return w
    swarm.DeviceSwarmOptimization._device_run = timed(
        "pso", swarm.DeviceSwarmOptimization._device_run)
    gp_opt.SafeOptSwarm._grow_safe_set = timed("grow", gp_opt.SafeOptSwarm._grow_safe_set)

    def step():
        np.random.seed(11)
        opt = sa.SafeOptSwarm(build_gps(cfg, gpy), cfg["fmin"], bounds=[(-5., 5.)] * 4,
                              threshold=cfg["threshold"], swarm_size=args.particles,
                              pso="device-rng", comm=comm)
        for g in opt.gps:
            g._fitted()
        ctx.sync()
        comm.barrier()
        for k in phase:
            phase[k] = 0.0
        t0 = time.perf_counter()
        x = opt.optimize()
        ctx.sync()
        total = time.perf_counter() - t0
        return total, dict(phase), opt.S.shape[0], x
    for _ in range(args.warmup):
        step()
    rows = [step() for _ in range(args.steps)]
    tot = np.array([r[0] for r in rows]) * 1e3
    pso = np.array([r[1]["pso"] for r in rows]) * 1e3
    grow = np.array([r[1]["grow"] for r in rows]) * 1e3
    med = int(np.argsort(tot)[len(tot) // 2])
    out = dict(workload="config5: SafeOptSwarm.optimize(), d=4, G=2, n=2000, pso='device-rng'",
               particles=args.particles, gpus=comm.world, steps=args.steps,
               ms_per_optimize=round(float(tot[med]), 2),
               pso_ms=round(float(pso[med]), 2), grow_ms=round(float(grow[med]), 2),
               other_ms=round(float(tot[med] - pso[med] - grow[med]), 2),
               grow_frac=round(float(grow[med] / tot[med]), 4),
               ms_all=[round(float(t), 2) for t in tot], safe_set_rows=rows[med][2],
               x=[float(v) for v in rows[med][3]])
    if comm.rank == 0:
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--particles", type=int, default=100_000)
    args = ap.parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:
        return spawn(args.gpus, sys.argv[1:])
    run(args)


if __name__ == "__main__":
    main()
