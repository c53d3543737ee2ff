"""``SafeOptSwarm.mes_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4: N operating-system processes, a fresh spawned child per rank, each with its own
HIP context on device 0 and its TRUE block of the particles, connected by
``safeopt_amd.dist.SocketComm`` in stream (the pattern of tests/test_gpu_thompson_nrank.py: RCCL
wants one GPU per rank).  Every rank must arrive, bit for bit, at what a ``LocalComm`` optimiser
on the whole swarm computes IN THE SAME PROCESS from the same seed, and at what rank 0 holds.

d = 3, two GPs, ``paths=3``, ``features=64``, ``max_iters=5``; per ``pso`` in {'device',
'device-rng'} the combinations (n, swarm_size) cover n in {12, 100} (the VALU and the
resident-factor posterior kernel) and swarm_size in {203, 20} (203: not divisible by 4; 20:
five particles a rank in world 4): ``x``, ``alpha``, the maxima, the floor, the Thompson picks,
the gathered personal bests and the global best of the 'mes' swarm (``sgp_swarm_run_mes_shard``),
and the state of NumPy's generator.  A rank that is handed another ``ystar`` makes EVERY rank
raise ``ValueError`` (one ``allreduce_max`` of a digest), none is left in a collective.

At most 4 worker processes plus the parent hold the GPU at once.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = {"device": [(12, 203), (100, 20)], "device-rng": [(100, 203), (12, 20)]}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


def _init(rank, world, port):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SAFEOPT_COMM="socket", SAFEOPT_HIP_DEVICE="0",
                      SAFEOPT_SOCKET_IN_STREAM="1")
    sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
    from safeopt_amd import dist
    ctx, comm = dist.init_from_env()
    assert isinstance(comm, dist.SocketComm) and comm.world == world and comm.in_stream
    return ctx, comm


def _same_state(a, b):
    return bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:])


def _optimiser(sa, gpy, comm, pso, n, P):
    d, G = 3, 2
    rng = np.random.default_rng(n)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    Ys = [_smooth(X, 40 + g) - _smooth(X, 40 + g).min() + 0.5 for g in range(G)]
    gps = [gpy.models.GPRegression(X, Ys[g], gpy.kern.RBF(d, 1.5, [0.8, 1.0, 1.2], ARD=True),
                                   noise_var=0.05 ** 2) for g in range(G)]
    np.random.seed(5)
    return sa.SafeOptSwarm(gps, [0.0] * G, bounds=[(-3., 3.)] * d, threshold=0.1,
                           swarm_size=P, pso=pso, comm=comm)


def _mes_run(sa, gpy, comm, pso, n, P, runs):
    opt = _optimiser(sa, gpy, comm, pso, n, P)
    del runs[:]
    x, alpha, st = opt.mes_point(paths=3, features=64, max_iters=5, return_state=True)
    out = {"x": x, "alpha": np.array([alpha]), "ystar": st["ystar"],
           "floor": np.array([st["floor"]]), "thompson_x": st["thompson_x"],
           "state": np.random.get_state()}
    assert len(runs) == 1                                   # one 'mes' swarm
    bp, bv, gb = runs[0]
    assert bp.shape == (P, 3) and bv.shape == (P,)          # gathered: the whole swarm
    out["best_positions"], out["best_values"], out["global_best"] = bp, bv, gb
    return out


def _mes_worker(rank, world, port, q):
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import dist, swarm
        runs = []
        orig = swarm.DeviceSwarmOptimization.run_swarm

        def traced(self, *a, **k):
            orig(self, *a, **k)
            if self._type == 'mes':
                runs.append((np.array(self.best_positions), np.array(self.best_values),
                             np.array(self.global_best)))
        swarm.DeviceSwarmOptimization.run_swarm = traced
        report, out = [], {}
        for pso in ("device", "device-rng"):
            for n, P in COMBOS[pso]:
                what = "%s n=%d P=%d" % (pso, n, P)
                a = _mes_run(sa, gpy, comm, pso, n, P, runs)
                b = _mes_run(sa, gpy, dist.LocalComm(), pso, n, P, runs)
                bad = sorted(k for k in b if k != "state" and not np.array_equal(a[k], b[k]))
                if not _same_state(a["state"], b["state"]):
                    bad.append("state")
                report.append((what, not bad if not bad else bad))
                out[what] = {k: v for k, v in a.items() if k != "state"}
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _mismatch_worker(rank, world, port, q):
    """The last rank holds another ``ystar``, then another floor: ``ValueError`` on every rank,
    and the ranks are still in step afterwards (a matching call goes through)."""
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        opt = _optimiser(sa, gpy, comm, "device", 12, 20)
        report = []
        odd = rank == world - 1
        for what, ystar, floor in (("another ystar", [0.5, 1.25 if odd else 1.0], 0.25),
                                   ("another floor", [0.5, 1.0], 0.5 if odd else 0.25)):
            np.random.seed(3)
            try:
                opt.mes_point(ystar=ystar, floor=floor, max_iters=2)
                report.append((what, "no error"))
            except ValueError as e:
                report.append((what, True if "different maxima or floors" in str(e) else str(e)))
        np.random.seed(3)
        x, alpha = opt.mes_point(ystar=[0.5, 1.0], floor=0.25, max_iters=2)
        report.append(("in step afterwards", bool(np.all(np.isfinite(x)) and alpha >= 0.0)))
        comm.barrier()
        comm.close()
        q.put((rank, report, {"after": (x, np.array([alpha]))}, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


# ---- the parent --------------------------------------------------------------------------------

def _launch(target, world):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = sorted((q.get(timeout=240) for _ in procs), key=lambda r: r[0])
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
        assert report
        for what, ok in report:
            print("rank %d  %-40s %s" % (rank, what, "ok" if ok is True else "MISMATCH %r" % (ok,)))
        assert all(ok is True for _what, ok in report), (rank, report)
    return results


def _ranks_agree(results):
    out0 = results[0][2]
    for rank, _report, out, _err in results[1:]:
        assert sorted(out) == sorted(out0)
        for what in out0:
            a, b = out[what], out0[what]
            if isinstance(b, dict):
                a, b = [a[k] for k in sorted(b)], [b[k] for k in sorted(b)]
            for u, w in zip(a, b):
                assert np.array_equal(u, w), (rank, what)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_mes_point_bit_identical(hip_device, world):
    _ranks_agree(_launch(_mes_worker, world))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_another_ystar_on_one_rank_raises_on_every_rank(hip_device, world):
    _ranks_agree(_launch(_mismatch_worker, world))


def test_library_has_the_three_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_swarm_fitness_mes", "sgp_swarm_run_mes", "sgp_swarm_run_mes_shard"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
