"""``SafeOptSwarm(..., comm=)``: the swarms split over REAL processes by particle.

N operating-system processes, each with its own HIP context on device 0, run their
contiguous blocks of every swarm (``sgp_swarm_run_shard``) and merge the global best after
every iteration through ``safeopt_amd.dist.SocketComm`` registered as the context's
transport (the pattern of tests/test_gpu_nrank.py: RCCL wants one GPU per rank).  Every
rank must arrive, bit for bit, at what one process computes: the returned points, ``S``,
``greedy_point``, ``best_lower_bound`` and every swarm's personal bests -- with every shard
larger than the few-points path (kSmallPoints = 4096) and, at n = 12 observations, a
posterior kernel that the shard's own row count would choose differently.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


def _run(sa, gpy, comm, pso, n, P, seed, sweeps):
    """Two optimize() calls with an observation in between; everything a rank ends with."""
    d, G = 3, 2
    rng = np.random.default_rng(n)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    Ys = [_smooth(X, 40 + g) - _smooth(X, 40 + g).min() + 0.5 for g in range(G)]
    gps = [gpy.models.GPRegression(X, Ys[g], gpy.kern.RBF(d, 1.5, [0.8, 1.0, 1.2], ARD=True),
                                   noise_var=0.05 ** 2) for g in range(G)]
    np.random.seed(seed)
    opt = sa.SafeOptSwarm(gps, [0.0] * G, bounds=[(-3., 3.)] * d, threshold=0.1,
                          swarm_size=P, pso=pso, comm=comm)
    out = {}
    for it in range(2):
        del sweeps[:]
        x = opt.optimize()
        out["x%d" % it] = np.array(x, dtype=float)
        out["sweeps%d" % it] = list(sweeps)
        if it == 0:
            y = np.array([float(_smooth(x[None, :], 40 + g)[0, 0]) + 0.3 for g in range(G)])
            opt.add_new_data_point(x, y)
    out["S"] = opt.S
    out["greedy_point"] = np.array(opt.greedy_point)
    out["best_lower_bound"] = np.array(opt.best_lower_bound)
    for st, sw in opt.swarms.items():
        out[st + "_best_values"] = np.array(sw.best_values)
        out[st + "_best_positions"] = np.array(sw.best_positions)
        out[st + "_global_best"] = np.array(sw.global_best)
    return out


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          SAFEOPT_COMM="socket", SAFEOPT_HIP_DEVICE="0",
                          SAFEOPT_SOCKET_IN_STREAM="1")
        sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import dist, swarm
        ctx, comm = dist.init_from_env()
        assert isinstance(comm, dist.SocketComm) and comm.world == world and comm.in_stream
        # the posterior kernel of every swarm run
        sweeps = []
        orig = swarm.DeviceSwarmOptimization._device_run

        def traced(self, *a, **k):
            orig(self, *a, **k)
            sweeps.append(ctx.last_sweep())
        swarm.DeviceSwarmOptimization._device_run = traced
        report = []
        for pso in ("device", "device-rng"):
            for n, P in ((100, 20_000), (12, 20_000)):
                a = _run(sa, gpy, comm, pso, n, P, 5, sweeps)
                b = _run(sa, gpy, dist.LocalComm(), pso, n, P, 5, sweeps)
                same = sorted(k for k in b if k.startswith("sweeps") or
                              np.array_equal(np.asarray(a[k]), np.asarray(b[k])))
                report.append(("%s n=%d P=%d" % (pso, n, P), sorted(b) == same,
                               {k: np.asarray(v) for k, v in a.items()},
                               a["sweeps0"] + a["sweeps1"] == b["sweeps0"] + b["sweeps1"]))
        try:
            sa.SafeOptSwarm(gpy.models.GPRegression(np.zeros((1, 2)), np.ones((1, 1)),
                                                     noise_var=0.01), [0.], bounds=[(-1., 1.)] * 2,
                            pso="host", comm=comm)
            host_err = False
        except ValueError:
            host_err = True
        comm.barrier()
        comm.close()
        q.put((rank, report, host_err, None))
    except Exception:
        import traceback
        q.put((rank, [], False, traceback.format_exc()))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_swarm_bit_identical(hip_device, world):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=1150) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for rank, report, host_err, err in results:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        assert host_err, "pso='host' with %d ranks did not raise ValueError" % world
        for what, ok, _out, same_kernel in report:
            print("rank %d  %-40s %s, kernels %s" % (rank, what, "ok" if ok else "MISMATCH",
                                                      "same" if same_kernel else "DIFFER"))
            assert ok and same_kernel, (rank, what)
    # every rank holds the same bits
    r0 = results[0][1]
    for rank, report, _, _ in results[1:]:
        assert [w for w, *_ in report] == [w for w, *_ in r0]
        for (what, _, out, _), (_, _, out0, _) in zip(report, r0):
            for k in out0:
                assert np.array_equal(out[k], out0[k]), (rank, what, k)
