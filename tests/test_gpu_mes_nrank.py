"""``SafeOpt.mes_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4 (the pattern of tests/test_gpu_thompson_nrank.py): N operating-system processes,
each with its own HIP context on device 0 and its TRUE shard of the 70 x 70 grid of
tests/_mes_problems.py (2450 or 1225 rows: no multiple of the 256 rows of a workgroup),
connected by ``safeopt_amd.dist.SocketComm``.  Every rank must arrive, bit for bit, at what a
``LocalComm`` optimiser on the whole grid computes IN THE SAME PROCESS from the same seed, and at
what rank 0 holds: ``x``, its alpha, the gathered ``(N,)`` alpha array, ``ystar`` and the floor.
With ``SAFEOPT_SOCKET_IN_STREAM=1`` floor and records are merged on the device behind the
in-stream collectives (``sgp_grid_mes_comm``: all-reduce, all-gather, k_mes_merge); with ``=0``
on the host (``allreduce_max``, ``allgather``, ``dist.merge_mes_records``): the same bits.

Through ``DeviceGrid.mes(comm=True)`` directly, with maxima so high that every alpha is exactly 0
(all rows tie) and chosen safe masks: a shard without a safe row takes part without winning, the
lowest safe row wins wherever it lies, the floor is the largest mean over the safe rows of all
shards, an empty mask gives -inf / -1 -- and ``mes_point`` then raises ``RuntimeError`` on every
rank.  That entry point needs the communicator in the context; for both kinds the same cases run
through ``mes_point`` with an edited ``S`` against the one-rank optimiser with the same edit.
Every worker reports through a queue the parent reads under a time limit; ranks still alive
after it are killed, and nothing is started after a failure.  At most 4 worker processes plus
the parent hold the GPU at once.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5


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


def _picks_worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import _mes_problems as P
        from safeopt_amd import _hip, dist
        opt, one = _opt(comm), _opt(dist.LocalComm())
        N = opt.inputs.shape[0]
        lo, hi = opt._shard
        assert (lo, hi) == dist.shard_range(N, rank, world) and hi - lo < N
        S = np.array(one.S)
        report, out = [("same S", bool(np.array_equal(np.array(opt.S), S) and 0 < S.sum() < N))], {}
        for within in ("safe", "MG", "all"):
            for floor in ("mean", None, 1.9):
                what = "%s floor=%r" % (within, floor)
                res = []
                for o in (opt, one):
                    np.random.seed(SEED)
                    x, a, values, ystar = o.mes_point(paths=P.PATHS, features=P.FEATURES,
                                                      within=within, floor=floor,
                                                      return_values=True)
                    res.append((x, np.float64(a), values, ystar, np.random.get_state()[1]))
                a, b = res
                ok = a[2].shape == (N,) and all(np.array_equal(u, w) for u, w in zip(a, b))
                np.random.seed(SEED)
                x2, a2 = opt.mes_point(paths=P.PATHS, features=P.FEATURES, within=within,
                                       floor=floor)
                ok = ok and np.array_equal(x2, a[0]) and a2 == a[1]
                report.append((what, bool(ok)))
                out[what] = a[:4]
        # the floor: the largest mean over the safe rows of all shards, as one rank has it
        ystar = out["safe floor='mean'"][3]
        want = one._backend.grid.mes(ystar, rows=_hip.MES_S, floor='mean')
        if in_stream:
            got = opt._backend.grid.mes(ystar, rows=_hip.MES_S, floor='mean', comm=True)
            report.append(("value, row, floor of sgp_grid_mes_comm", got[1:] == want[1:]))
        else:
            mine = opt._backend.grid.mes(ystar[:1], rows=_hip.MES_S, floor='mean')[3]
            report.append(("floor over the ranks",
                           float(comm.allreduce_max(np.array([mine]))[0]) == want[3]))
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _direct_worker(rank, world, port, in_stream, q):
    """``DeviceGrid.mes(comm=True)`` with alpha identically 0, under chosen safe masks."""
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        from safeopt_amd import _hip, dist
        opt = _opt(comm)
        N = opt.inputs.shape[0]
        be = opt._backend
        lo, hi = opt._shard
        lo1 = dist.shard_range(N, 1, world)[0]
        lo_last = dist.shard_range(N, world - 1, world)[0]
        mean = dist.gather_shard_columns(comm, be.download(_hip.MEAN), N)[0]

        def run(rows, which=_hip.MES_S, floor='mean'):
            full = np.zeros(N, dtype=bool)
            full[list(rows)] = True
            be.upload_mask(_hip.S, full[lo:hi])
            return be.grid.mes([1e6], rows=which, floor=floor, alpha=True, comm=True)
        report = []
        # rank 0 has no safe row; the lowest safe row lies in rank 1's shard
        first = lo1 + 5
        rows = [first, first + 70, lo_last + 20, N - 1]
        al, v, i, fl = run(rows)
        report.append(("lowest safe row in rank 1's shard, rank 0 without one",
                       bool((v, i) == (0.0, first) and fl == mean[rows].max()
                            and al.shape == (hi - lo,) and np.all(al == 0.0))))
        rows = [lo_last + 3, N - 1]
        _, v, i, fl = run(rows)
        report.append(("safe set in the last shard",
                       bool((v, i) == (0.0, lo_last + 3) and fl == mean[rows].max())))
        _, v, i, fl = run([first], which=_hip.MES_ALL)
        report.append(("all rows tie", bool((v, i) == (0.0, 0) and fl == mean.max())))
        _, v, i, fl = run([first], floor=None)
        report.append(("no floor", bool((v, i, fl) == (0.0, first, -np.inf))))
        _, v, i, fl = run([])
        report.append(("empty mask", bool((v, i, fl) == (-np.inf, -1, -np.inf))))
        opt.S[:] = False
        np.random.seed(SEED)                 # (SPMD: the ranks draw the same paths)
        try:
            opt.mes_point(paths=3, features=16)
            report.append(("RuntimeError on every rank", False))
        except RuntimeError as e:
            report.append(("RuntimeError on every rank", "no safe points" in str(e)))
        comm.barrier()
        comm.close()
        q.put((rank, report, {}, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _edited_worker(rank, world, port, in_stream, q):
    """``mes_point`` under edited safe sets, against the one-rank optimiser with the same edit:
    the cases of ``_direct_worker`` for a communicator whose merges run on the host."""
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import _mes_problems as P
        from safeopt_amd import dist
        opt, one = _opt(comm), _opt(dist.LocalComm())
        N = opt.inputs.shape[0]
        lo1 = dist.shard_range(N, 1, world)[0]
        lo_last = dist.shard_range(N, world - 1, world)[0]
        cases = [("rank 0 without a safe row", list(range(lo1 + 5, lo1 + 200)) +
                  list(range(lo_last + 20, N))),
                 ("safe set in the last shard", list(range(lo_last + 3, lo_last + 150)) + [N - 1])]
        report, out = [], {}
        for what, rows in cases:
            full = np.zeros(N, dtype=bool)
            full[rows] = True
            res = []
            for o in (opt, one):
                o.S[:] = full
                np.random.seed(SEED)
                x, a, values, ystar = o.mes_point(paths=P.PATHS, features=P.FEATURES,
                                                  return_values=True)
                res.append((x, np.float64(a), values, ystar))
            a, b = res
            row = int(np.argmax(np.where(full, a[2], -np.inf)))
            ok = (all(np.array_equal(u, w) for u, w in zip(a, b)) and full[row]
                  and np.array_equal(a[0], opt.inputs[row]) and a[1] == a[2][row])
            report.append((what, bool(ok)))
            out[what] = a
        opt.S[:] = False
        np.random.seed(SEED)
        try:
            opt.mes_point(paths=3, features=16)
            report.append(("RuntimeError on every rank", False))
        except RuntimeError as e:
            report.append(("RuntimeError on every rank", "no safe points" in str(e)))
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
            print("rank %d  %-55s %s" % (rank, what, "ok" if ok is True else "MISMATCH %r" % (ok,)))
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
def test_mes_point_bit_identical(hip_device, world, in_stream):
    _ranks_agree(_launch(_picks_worker, world, in_stream))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_grid_mes_comm_ties_and_empty_shards(hip_device, world):
    _launch(_direct_worker, world, True)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("in_stream", [True, False], ids=["device-merge", "host-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_mes_point_with_empty_shards(hip_device, world, in_stream):
    _ranks_agree(_launch(_edited_worker, world, in_stream))


def test_library_has_the_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_mes_eval", "sgp_grid_mes", "sgp_grid_mes_comm"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
