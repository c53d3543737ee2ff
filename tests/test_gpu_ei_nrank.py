"""``SafeOpt.ei_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4 (the machinery of tests/test_gpu_mes_nrank.py): N operating-system processes, each
with its own HIP context on device 0 and its TRUE shard of the 70 x 70 grid of
tests/_mes_problems.py (2450 or 1225 rows: no multiple of the 256 rows of a workgroup),
connected by ``safeopt_amd.dist.SocketComm``.  Every rank must arrive, bit for bit, at what a
``LocalComm`` optimiser on the whole grid computes IN THE SAME PROCESS, and at what rank 0
holds: ``x``, its alpha, the gathered ``(N,)`` alpha array and the incumbent.  With
``SAFEOPT_SOCKET_IN_STREAM=1`` incumbent and records are merged on the device behind the
in-stream collectives (``sgp_grid_ei_comm``: all-reduce, all-gather, k_ei_merge); with ``=0`` on
the host (``allreduce_max``, ``allgather``, ``dist.merge_mes_records``): the same bits.

The same worker then edits ``S`` -- rank 0 without a safe row; the safe set in the last shard
only -- and asks again, against the one-rank optimiser with the same edit; with ``kind='pi'`` and
an incumbent far below every mean, ln Phi is exactly 0 on every row: a tie across all shards,
which the lowest safe row wins wherever it lies.  An empty ``S`` raises ``RuntimeError`` on every
rank.  ``DeviceGrid.ei(comm=True)`` is driven directly for the in-stream communicator: the
incumbent over the safe rows of all shards, an empty mask.  Every worker reports through a queue
the parent reads under a time limit; ranks still alive after it are killed.  At most 4 worker
processes plus the parent hold the GPU at once.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [dict(), dict(kind='pi', xi=0.05), dict(incumbent='data'), dict(incumbent=1.9),
         dict(within='MG'), dict(within='all', feasibility=True), dict(feasibility=True)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _init(rank, world, port, in_stream):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SAFEOPT_COMM="socket", SAFEOPT_HIP_DEVICE="0",
                      SAFEOPT_SOCKET_IN_STREAM="1" if in_stream else "0")
    sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
    from safeopt_amd import dist
    ctx, comm = dist.init_from_env()
    assert isinstance(comm, dist.SocketComm) and comm.world == world
    assert comm.in_stream == bool(in_stream)
    return ctx, comm


def _opt(comm):
    import safeopt_amd as sa
    import safeopt_amd.gpy as gpy
    import _mes_problems as P
    from _golden import make_kernel
    z, meta = P.problem("plane")
    gp = gpy.models.GPRegression(z["it0_X0"], z["it0_Y0"],
                                 make_kernel(gpy.kern, meta["kernels"][0]), noise_var=P.NOISE)
    opt = sa.SafeOpt(gp, z["parameter_set"], P.FMIN, beta=P.BETA, threshold=0.1, comm=comm)
    opt.optimize()
    return opt


def _both(opt, one, kw):
    res = []
    for o in (opt, one):
        x, a, values, tau = o.ei_point(return_values=True, **kw)
        res.append((x, np.float64(a), values, np.float64(tau)))
    return res


def _picks_worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        from safeopt_amd import _hip, dist
        opt, one = _opt(comm), _opt(dist.LocalComm())
        N = opt.inputs.shape[0]
        lo, hi = opt._shard
        assert (lo, hi) == dist.shard_range(N, rank, world) and hi - lo < N
        S = np.array(one.S)
        report, out = [("same S", bool(np.array_equal(np.array(opt.S), S) and 0 < S.sum() < N))], {}
        for kw in CASES:
            what = repr(sorted(kw.items()))
            a, b = _both(opt, one, kw)
            ok = a[2].shape == (N,) and all(np.array_equal(u, w) for u, w in zip(a, b))
            x2, a2 = opt.ei_point(**kw)
            ok = ok and np.array_equal(x2, a[0]) and a2 == a[1]
            report.append((what, bool(ok)))
            out[what] = a
        if in_stream:
            want = one._backend.grid.ei(rows=_hip.MES_S, tau='mean')
            got = opt._backend.grid.ei(rows=_hip.MES_S, tau='mean', comm=True)
            report.append(("value, row, tau of sgp_grid_ei_comm", got[1:] == want[1:]))
        # ---- edited safe sets, against the one-rank optimiser with the same edit
        lo1 = dist.shard_range(N, 1, world)[0]
        lo_last = dist.shard_range(N, world - 1, world)[0]
        cases = [("rank 0 without a safe row", list(range(lo1 + 5, lo1 + 200)) +
                  list(range(lo_last + 20, N))),
                 ("safe set in the last shard", list(range(lo_last + 3, lo_last + 150)) + [N - 1])]
        for what, rows in cases:
            full = np.zeros(N, dtype=bool)
            full[rows] = True
            opt.S[:] = full
            one.S[:] = full
            a, b = _both(opt, one, dict())
            row = int(np.flatnonzero(full)[np.argmax(a[2][full])])
            ok = (all(np.array_equal(u, w) for u, w in zip(a, b))
                  and np.array_equal(a[0], opt.inputs[row]) and a[1] == a[2][row])
            report.append((what, bool(ok)))
            out[what] = a
            # every row ties at ln Phi = 0: the lowest safe row, in whichever shard it lies
            tie = dict(kind='pi', incumbent=-1e6)
            a, b = _both(opt, one, tie)
            ok = (all(np.array_equal(u, w) for u, w in zip(a, b)) and np.all(a[2] == 0.0)
                  and a[1] == 0.0 and np.array_equal(a[0], opt.inputs[rows[0]]))
            report.append((what + ", a tie across the shards", bool(ok)))
        # ---- nothing is safe: behind the collective, on every rank
        opt.S[:] = False
        for kw in (dict(), dict(incumbent=1.0)):
            try:
                opt.ei_point(**kw)
                report.append(("RuntimeError on every rank %r" % (kw,), False))
            except RuntimeError as e:
                report.append(("RuntimeError on every rank %r" % (kw,), "no safe points" in str(e)))
        if in_stream:
            al, v, i, tu = opt._backend.grid.ei(rows=_hip.MES_S, tau='mean', alpha=True, comm=True)
            report.append(("empty mask over the ranks",
                           bool((v, i, tu) == (-np.inf, -1, -np.inf) and np.all(al == -np.inf))))
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _launch(target, world, in_stream):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=target, args=(r, world, port, in_stream, q))
             for r in range(world)]
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
            print("rank %d  %-60s %s" % (rank, what, "ok" if ok is True else "MISMATCH %r" % (ok,)))
        assert all(ok is True for _what, ok in report), (rank, report)
    return results


def _ranks_agree(results):
    out0 = results[0][2]
    for rank, _report, out, _err in results[1:]:
        assert sorted(out) == sorted(out0)
        for what in out0:
            for u, w in zip(out[what], out0[what]):
                assert np.array_equal(u, w), (rank, what)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("in_stream", [True, False], ids=["device-merge", "host-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_ei_point_bit_identical(hip_device, world, in_stream):
    _ranks_agree(_launch(_picks_worker, world, in_stream))


def test_library_has_the_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_ei_eval", "sgp_grid_ei", "sgp_grid_ei_comm"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
