"""``SafeOptSwarm.optimize_batch`` on N ranks: the hallucinated swarms split over REAL
processes by particle (needs an MI355X).

World 2 and 4: N operating-system processes, each with its own HIP context on device 0, run
their contiguous blocks of every swarm -- the hallucinated ones through
``sgp_swarm_run_hall_shard`` -- and merge the global best after every iteration through
``safeopt_amd.dist.SocketComm`` registered as the context's transport (the pattern of
tests/test_gpu_swarm_nrank.py, whose problem this is: d = 3, two GPs, RBF ARD).  Every rank
must arrive, bit for bit, at what ``LocalComm()`` computes IN THE SAME PROCESS from the same
seed: ``X``, ``sd_h``, the state of NumPy's generator afterwards, ``S``, ``greedy_point``,
``best_lower_bound``, and the posterior kernel of every swarm run.

Sizes ``(n, swarm_size)``: (100, 20000) and (12, 20000), the ground of the N-rank swarm test,
and (100, 5000): at world 4 a block of 1250 particles lies under the few-points path
(kSmallPoints = 4096) while the swarm does not -- the kernel choice must follow the swarm.
``pso`` in {'device', 'device-rng'}; ``optimize_batch(size=3, max_iters=4,
return_state=True)``.  The clones are gone afterwards: every handle ``DeviceGP.clone`` handed
out is released.  ``sgp_swarm_run_hall_shard`` with ``P < P_total`` on a context without a
communicator is an error, not a fault.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((100, 20_000), (12, 20_000), (100, 5_000))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


def _gps(gpy, n):
    d, G = 3, 2
    rng = np.random.default_rng(n)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    Ys = [_smooth(X, 40 + g) - _smooth(X, 40 + g).min() + 0.5 for g in range(G)]
    return [gpy.models.GPRegression(X, Ys[g], gpy.kern.RBF(d, 1.5, [0.8, 1.0, 1.2], ARD=True),
                                    noise_var=0.05 ** 2) for g in range(G)]


def _same_state(a, b):
    return bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:])


def _run(sa, gpy, comm, pso, n, P, sweeps, clones):
    np.random.seed(5)
    opt = sa.SafeOptSwarm(_gps(gpy, n), [0.0, 0.0], bounds=[(-3., 3.)] * 3, threshold=0.1,
                          swarm_size=P, pso=pso, comm=comm)
    del sweeps[:], clones[:]
    X, sd_h = opt.optimize_batch(size=3, max_iters=4, return_state=True)
    assert len(clones) == 2 and all(c.h is None for c in clones), "a clone is still alive"
    return {"X": X, "sd_h": sd_h, "state": np.random.get_state(), "S": np.array(opt.S),
            "greedy_point": np.array(opt.greedy_point),
            "best_lower_bound": np.array(opt.best_lower_bound), "sweeps": list(sweeps)}


def _worker(rank, world, port, q):
    try:
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                          MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          SAFEOPT_COMM="socket", SAFEOPT_HIP_DEVICE="0",
                          SAFEOPT_SOCKET_IN_STREAM="1")
        sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import _hip, dist, swarm
        ctx, comm = dist.init_from_env()
        assert isinstance(comm, dist.SocketComm) and comm.world == world and comm.in_stream
        # the posterior kernel of every swarm run, and every clone handed out
        sweeps, clones = [], []
        run0, clone0 = swarm.DeviceSwarmOptimization._device_run, _hip.DeviceGP.clone

        def traced(self, *a, **k):
            run0(self, *a, **k)
            sweeps.append((self._type, self._clones is not None, ctx.last_sweep()))

        def cloned(self):
            c = clone0(self)
            clones.append(c)
            return c
        swarm.DeviceSwarmOptimization._device_run = traced
        _hip.DeviceGP.clone = cloned
        report, out = [], {}
        for pso in ("device", "device-rng"):
            for n, P in SIZES:
                what = "%s n=%d P=%d" % (pso, n, P)
                a = _run(sa, gpy, comm, pso, n, P, sweeps, clones)
                b = _run(sa, gpy, dist.LocalComm(), pso, n, P, sweeps, clones)
                bad = sorted(k for k in b if k not in ("state", "sweeps")
                             and not np.array_equal(a[k], b[k]))
                if not _same_state(a["state"], b["state"]):
                    bad.append("state")
                if a["sweeps"] != b["sweeps"] or not any(h for _t, h, _k in a["sweeps"]):
                    bad.append("sweeps %r / %r" % (a["sweeps"], b["sweeps"]))
                if a["X"].shape[0] < 2 or a["sd_h"].shape != (a["X"].shape[0], 2):
                    bad.append("shape %r" % (a["X"].shape,))
                report.append((what, True if not bad else bad))
                out[what] = {k: v for k, v in a.items() if k not in ("state", "sweeps")}
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_hallucinated_swarms_bit_identical(hip_device, world):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=540) for _ in procs), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=30)
        hung = [p.pid for p in procs if p.is_alive()]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert not hung, "ranks still running after their report: %r" % (hung,)
    for rank, report, _out, err in results:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        assert len(report) == 2 * len(SIZES)
        for what, ok in report:
            print("rank %d  %-32s %s" % (rank, what, "ok" if ok is True else "MISMATCH %r" % (ok,)))
        assert all(ok is True for _what, ok in report), (rank, report)
    # every rank holds the same bits
    out0 = results[0][2]
    for rank, _report, out, _err in results[1:]:
        assert sorted(out) == sorted(out0)
        for what in out0:
            for k in out0[what]:
                assert np.array_equal(out[what][k], out0[what][k]), (rank, what, k)


def test_a_block_without_a_communicator_is_an_error(hip_device):
    """``sgp_swarm_run_hall_shard`` with ``P < P_total`` on a context without a communicator
    returns an error; ``p0 = 0, P = P_total`` is ``sgp_swarm_run_hall``, bit for bit."""
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    assert "sgp_swarm_run_hall_shard" in _hip.PROTOTYPES
    assert hasattr(_hip.lib(), "sgp_swarm_run_hall_shard")
    # a context of its own: the default one may carry a communicator by now
    ctx = _hip.Context(0)
    devs = []
    for g in _gps(gpy, 12):
        dv = _hip.DeviceGP(ctx, g.kern._desc(3), 0.05 ** 2)
        dv.set_data(np.asarray(g.X), np.asarray(g.Y)[:, 0])
        devs.append(dv)
    d, P = 3, 40
    clones = [dv.clone() for dv in devs]
    try:
        assert all(c.append(np.array([0.1, -0.2, 0.3]), 0.0) for c in clones)
        rng = np.random.default_rng(1)
        fit = (2.0, np.array([0.0, 0.0]), np.array([1.0, 1.0]), 0.0)

        def state(rows):
            return [rng0[:rows].copy(), np.empty((rows, d)), np.empty((rows, d)),
                    np.empty(rows), np.empty(d)]
        rng0 = rng.uniform(-0.5, 0.5, size=(P, d))
        st = state(10)
        with pytest.raises(_hip.HipError, match="communicator"):
            _hip.swarm_run_hall(ctx, devs, clones, "maximizers", *fit, *st, np.full(d, 0.1),
                                None, True, 2, 1.0, -0.4, None, seed=7, shard=(0, P))
        # an empty block of a sharded swarm is refused too, and a block outside the swarm
        with pytest.raises(_hip.HipError, match="bad block"):
            _hip.swarm_run_hall(ctx, devs, clones, "maximizers", *fit, *st, np.full(d, 0.1),
                                None, True, 2, 1.0, -0.4, None, seed=7, shard=(35, P))
        whole, same = state(P), state(P)
        _hip.swarm_run_hall(ctx, devs, clones, "maximizers", *fit, *whole, np.full(d, 0.1),
                            None, True, 2, 1.0, -0.4, None, seed=7)
        _hip.swarm_run_hall(ctx, devs, clones, "maximizers", *fit, *same, np.full(d, 0.1),
                            None, True, 2, 1.0, -0.4, None, seed=7, shard=(0, P))
        for a, b in zip(whole, same):
            assert np.array_equal(a, b)
        assert np.isfinite(whole[3]).all()
    finally:
        for c in clones:
            c.destroy()
