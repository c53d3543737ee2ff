"""``SafeOptSwarm.ise_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4: N operating-system processes, a fresh spawned child per rank, each with its own
HIP context on device 0 and its TRUE block of the particles, connected by
``safeopt_amd.dist.SocketComm`` in stream (the pattern of tests/test_gpu_swarm_mes_nrank.py).
Every rank must arrive, bit for bit, at what a ``LocalComm`` optimiser on the whole swarm
computes IN THE SAME PROCESS from the same seed, and at what rank 0 holds.

d = 3, two GPs, ``targets=70`` (more than one block of 64 columns), ``about='all'``,
``max_iters=4``; (n, swarm_size) = (12, 203) with ``pso='device'`` and (100, 20) with
``'device-rng'``: ``x``, ``alpha``, the targets and their posterior, the attained target, the
gathered personal bests and the global best of the 'ise' swarm (``sgp_swarm_run_ise_shard``),
and the state of NumPy's generator.  A rank that is handed other targets makes EVERY rank
raise ``ValueError`` (one ``allreduce_max`` of a digest), none is left in a collective.

At most 4 worker processes plus the parent hold the GPU at once; every worker ends itself
after ``WORKER_SECONDS`` (``signal.alarm``), whatever state it is in.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = {"device": [(12, 203)], "device-rng": [(100, 20)]}
WORKER_SECONDS = 150


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
    import signal
    signal.alarm(WORKER_SECONDS)                # the process's own time limit
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


def _ise_run(sa, gpy, comm, pso, n, P, runs):
    opt = _optimiser(sa, gpy, comm, pso, n, P)
    del runs[:]
    x, alpha, st = opt.ise_point(targets=70, about='all', max_iters=4, return_state=True)
    out = {"x": x, "alpha": np.array([alpha]), "targets": st["targets"],
           "target": st["target"], "zmean": st["zmean"], "zvar": st["zvar"],
           "state": np.random.get_state()}
    assert st["targets"].shape == (70, 3)
    assert len(runs) == 1                                   # one 'ise' swarm
    bp, bv, gb = runs[0]
    assert bp.shape == (P, 3) and bv.shape == (P,)          # gathered: the whole swarm
    out["best_positions"], out["best_values"], out["global_best"] = bp, bv, gb
    return out


def _ise_worker(rank, world, port, q):
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import dist, swarm
        runs = []
        orig = swarm.DeviceSwarmOptimization.run_swarm

        def traced(self, *a, **k):
            orig(self, *a, **k)
            if self._type == 'ise':
                runs.append((np.array(self.best_positions), np.array(self.best_values),
                             np.array(self.global_best)))
        swarm.DeviceSwarmOptimization.run_swarm = traced
        report, out = [], {}
        for pso in ("device", "device-rng"):
            for n, P in COMBOS[pso]:
                what = "%s n=%d P=%d" % (pso, n, P)
                a = _ise_run(sa, gpy, comm, pso, n, P, runs)
                b = _ise_run(sa, gpy, dist.LocalComm(), pso, n, P, runs)
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
    """The last rank holds another target row: ``ValueError`` on every rank, and the ranks are
    still in step afterwards (a matching call goes through)."""
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        opt = _optimiser(sa, gpy, comm, "device", 12, 20)
        report = []
        odd = rank == world - 1
        rows = np.random.default_rng(9).uniform(-3.0, 3.0, size=(5, 3))
        other = rows.copy()
        other[4, 1] += 0.25
        np.random.seed(3)
        try:
            opt.ise_point(targets=other if odd else rows, about='all', max_iters=2)
            report.append(("other targets", "no error"))
        except ValueError as e:
            report.append(("other targets", True if "different targets" in str(e) else str(e)))
        np.random.seed(3)
        x, alpha = opt.ise_point(targets=rows, about='all', max_iters=2)
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
        results = sorted((q.get(timeout=WORKER_SECONDS + 10) for _ in procs),
                         key=lambda r: r[0])
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
def test_sharded_ise_point_bit_identical(hip_device, world):
    _ranks_agree(_launch(_ise_worker, world))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_other_targets_on_one_rank_raise_on_every_rank(hip_device, world):
    _ranks_agree(_launch(_mismatch_worker, world))


def test_library_has_the_three_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_swarm_fitness_ise", "sgp_swarm_run_ise", "sgp_swarm_run_ise_shard"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
