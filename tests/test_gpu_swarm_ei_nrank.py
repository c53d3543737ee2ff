"""``SafeOptSwarm.ei_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4: N operating-system processes, a fresh spawned child per rank, each with its own
HIP context on device 0 and its TRUE block of the particles, connected by
``safeopt_amd.dist.SocketComm`` in stream (the pattern, the problem and the ``COMBOS`` of
tests/test_gpu_swarm_mes_nrank.py).  Every rank must arrive, bit for bit, at what a ``LocalComm``
optimiser on the whole swarm computes IN THE SAME PROCESS from the same seed, and at what rank 0
holds: ``x``, ``alpha``, the incumbent, the safety flag of the pick, the gathered personal bests
and the global best of the 'ei' swarm (``sgp_swarm_run_ei_shard``), and the state of NumPy's
generator -- in safe mode (``within='safe'``, log-EI) and in free mode (``within='bounds'``,
log-PI with the feasibility weights), ``max_iters=5``.  A rank that is handed another incumbent
makes EVERY rank raise ``ValueError`` (one ``allreduce_max`` of a digest), none is left in a
collective.

At most 4 worker processes plus the parent hold the GPU at once.  A child that ends without a
report ends the test at once; every child is waited for under a limit of its own.
"""
import queue as queue_mod
import time

import numpy as np
import pytest

from test_gpu_swarm_mes_nrank import (COMBOS, _free_port, _init, _optimiser, _ranks_agree,
                                      _same_state)

pytestmark = pytest.mark.gpu

MODES = [("safe", dict(kind='ei', within='safe')),
         ("free", dict(kind='pi', within='bounds', feasibility=True, xi=0.125))]
CHILD_LIMIT = 240.0        # seconds a child may take to report


def _ei_run(sa, gpy, comm, pso, n, P, runs, kw):
    opt = _optimiser(sa, gpy, comm, pso, n, P)
    del runs[:]
    x, alpha, st = opt.ei_point(max_iters=5, return_state=True, **kw)
    out = {"x": x, "alpha": np.array([alpha]), "tau": np.array([st["tau"]]),
           "safe": np.array([st["safe"]]), "state": np.random.get_state()}
    assert len(runs) == 1                                   # one 'ei' swarm
    bp, bv, gb = runs[0]
    assert bp.shape == (P, 3) and bv.shape == (P,)          # gathered: the whole swarm
    out["best_positions"], out["best_values"], out["global_best"] = bp, bv, gb
    return out


def _ei_worker(rank, world, port, q):
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import dist, swarm
        runs = []
        orig = swarm.DeviceSwarmOptimization.run_swarm

        def traced(self, *a, **k):
            orig(self, *a, **k)
            if self._type == 'ei':
                runs.append((np.array(self.best_positions), np.array(self.best_values),
                             np.array(self.global_best)))
        swarm.DeviceSwarmOptimization.run_swarm = traced
        report, out = [], {}
        for pso in ("device", "device-rng"):
            for n, P in COMBOS[pso]:
                for mode, kw in MODES:
                    what = "%s n=%d P=%d %s" % (pso, n, P, mode)
                    a = _ei_run(sa, gpy, comm, pso, n, P, runs, kw)
                    b = _ei_run(sa, gpy, dist.LocalComm(), pso, n, P, runs, kw)
                    bad = sorted(k for k in b if k != "state" and not np.array_equal(a[k], b[k]))
                    if not _same_state(a["state"], b["state"]):
                        bad.append("state")
                    if not np.all(np.isfinite(a["best_values"])):
                        bad.append("a personal best is not finite")
                    report.append((what, not bad if not bad else bad))
                    out[what] = {k: v for k, v in a.items() if k != "state"}
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _mismatch_worker(rank, world, port, q):
    """The last rank holds another ``tau``, then another ``xi``: ``ValueError`` on every rank,
    and the ranks are still in step afterwards (a matching call goes through)."""
    try:
        ctx, comm = _init(rank, world, port)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        opt = _optimiser(sa, gpy, comm, "device", 12, 20)
        report = []
        odd = rank == world - 1
        for what, tau, xi in (("another tau", 1.25 if odd else 1.0, 0.0),
                              ("another xi", 1.0, 0.5 if odd else 0.25)):
            np.random.seed(3)
            try:
                opt.ei_point(incumbent=tau, xi=xi, max_iters=2)
                report.append((what, "no error"))
            except ValueError as e:
                report.append((what, True if "different incumbents" in str(e) else str(e)))
        np.random.seed(3)
        x, alpha = opt.ei_point(incumbent=1.0, xi=0.25, max_iters=2)
        report.append(("in step afterwards", bool(np.all(np.isfinite(x)) and np.isfinite(alpha))))
        comm.barrier()
        comm.close()
        q.put((rank, report, {"after": (x, np.array([alpha]))}, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


# ---- the parent --------------------------------------------------------------------------------

def _launch(target, world):
    """One fresh process per rank.  Every child has ``CHILD_LIMIT`` seconds to report; a child
    that ends without a report (a crash) ends the test at once, the others are killed."""
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=target, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results, failed = [], None
    deadline = time.monotonic() + CHILD_LIMIT
    try:
        while len(results) < world and failed is None:
            try:
                results.append(q.get(timeout=0.25))
                continue
            except queue_mod.Empty:
                pass
            reported = set(r[0] for r in results)
            dead = [(r, p.exitcode) for r, p in enumerate(procs)
                    if r not in reported and p.exitcode is not None]
            if dead and q.empty():
                failed = "ranks ended without a report (rank, exit code): %r" % (dead,)
            elif time.monotonic() > deadline:
                failed = "ranks %r did not report within %.0f s" % (
                    sorted(set(range(world)) - reported), CHILD_LIMIT)
        if failed is None:
            for p in procs:
                p.join(timeout=30)
            hung = [p.pid for p in procs if p.is_alive()]
            if hung:
                failed = "ranks still running after their report: %r" % (hung,)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert failed is None, failed
    results.sort(key=lambda r: r[0])
    for rank, report, _out, err in results:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
        assert report
        for what, ok in report:
            print("rank %d  %-40s %s" % (rank, what, "ok" if ok is True else "MISMATCH %r" % (ok,)))
        assert all(ok is True for _what, ok in report), (rank, report)
    return results


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_ei_point_bit_identical(hip_device, world):
    _ranks_agree(_launch(_ei_worker, world))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_another_tau_on_one_rank_raises_on_every_rank(hip_device, world):
    _ranks_agree(_launch(_mismatch_worker, world))


def test_library_has_the_three_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_swarm_fitness_ei", "sgp_swarm_run_ei", "sgp_swarm_run_ei_shard"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
