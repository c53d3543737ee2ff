"""``SafeOpt.ise_point`` / ``info_point`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4 (the pattern of tests/test_gpu_mes_nrank.py): N operating-system processes, each
with its own HIP context on device 0 and its TRUE shard of the 70 x 70 grid of
tests/_mes_problems.py (2450 or 1225 rows: no multiple of a workgroup), connected by
``safeopt_amd.dist.SocketComm``.  Every rank must arrive, bit for bit, at what a ``LocalComm``
optimiser on the whole grid computes IN THE SAME PROCESS, and at what rank 0 holds: ``x``, its
alpha, the candidate ``rows``, their ``values`` and ``targets`` -- a pair depends on the candidate
and the row alone.  With ``SAFEOPT_SOCKET_IN_STREAM=1`` the ranks' alpha | target blocks are merged
on the device behind one in-stream all-gather (``sgp_grid_ise_comm``: k_ise_merge, k_ise_pick);
with ``=0`` on the host (``allgather``, ``dist.merge_ise_records``): the same bits.

Under edited safe sets: rank 0 without a safe row, ``S`` in the last shard only, every unsafe row
in ONE shard (the other ranks have no target and must not win), explicit rows that span all
shards or lie in the last one; ``S`` all true or all false and a candidate outside ``S`` raise the
same error on every rank.  Every worker reports through a queue the parent reads under a time
limit; ranks still alive after it are killed, and nothing is started after a failure.  At most 4
worker processes plus the parent hold the GPU at once.
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


def _point(o, **kw):
    """``ise_point``'s result as arrays, or the error it raises as ``(type name, message)``."""
    try:
        x, a, rows, values, targets = o.ise_point(return_values=True, **kw)
        return ("ok", x, np.float64(a), rows, values, targets)
    except (RuntimeError, ValueError) as e:
        return (type(e).__name__, str(e))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, w) for u, w in zip(a, b))


def _worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import _mes_problems as P
        from safeopt_amd import _hip, dist
        opt, one = _opt(comm), _opt(dist.LocalComm())
        N = opt.inputs.shape[0]
        lo, hi = opt._shard
        assert (lo, hi) == dist.shard_range(N, rank, world) and hi - lo < N
        lo1 = dist.shard_range(N, 1, world)[0]
        lo_last = dist.shard_range(N, world - 1, world)[0]
        S0 = np.array(one.S)
        report = [("same S", bool(np.array_equal(np.array(opt.S), S0) and 0 < S0.sum() < N))]
        out = {}

        def both(what, want_ok=True, **kw):
            a, b = _point(opt, **kw), _point(one, **kw)
            ok = _same(a, b) and (a[0] == "ok") == want_ok
            if ok and a[0] == "ok":
                x2, a2 = opt.ise_point(**kw)
                ok = np.array_equal(x2, a[1]) and a2 == a[2]
            report.append((what, bool(ok)))
            out[what] = a
            return a

        def edit(mask):
            for o in (opt, one):
                o.S[:] = mask

        # ---- the natural safe set: candidates by count
        a = both("K = 40, unsafe", candidates=40, about='unsafe')
        report.append(("selected on the device", opt._ise_path == one._ise_path == 'device'))
        report.append(("targets are unsafe rows", bool(not np.any(S0[a[5]]))))
        both("K = 7, all", candidates=7, about='all')
        # ---- info_point: the two N-rank picks
        res = []
        for o in (opt, one):
            np.random.seed(SEED)
            x, al, which = o.info_point(paths=P.PATHS, features=P.FEATURES, candidates=40)
            res.append((x, np.float64(al), np.array([which == 'ise'])))
        report.append(("info_point", _same(*res)))
        out["info_point"] = res[0]
        # ---- sgp_grid_ise_comm against the host merge of the ranks' sgp_grid_ise_at
        if in_stream:
            be = opt._backend
            rows = a[3]
            fmin = np.asarray(opt.fmin, dtype=float).reshape(-1)
            xc, vx = opt._ise_rows_by_value(rows, fmin)
            ok = True
            for code in (_hip.ISE_UNSAFE, _hip.ISE_ALL):
                al, tg, _v, _i = be.grid.ise_at(be._dev(), fmin, rows, xc, vx, about=code)
                rec = comm.allgather(np.stack([al, tg.astype(np.float64)]))
                wal, wtg = dist.merge_ise_records(rec[:, 0], rec[:, 1].astype(np.int64))
                got = be.grid.ise_at(be._dev(), fmin, rows, xc, vx, about=code, comm=True)
                ok = (ok and np.array_equal(got[0], wal) and np.array_equal(got[1], wtg)
                      and got[2:] == dist.pick_ise(wal, wtg, rows))
            report.append(("sgp_grid_ise_comm is the host merge of sgp_grid_ise_at", bool(ok)))
        # ---- explicit rows, under a safe set with rows in every shard
        stripes = S0 | (np.arange(N) % 7 == 0)
        edit(stripes)
        ids = np.flatnonzero(stripes)
        span = ids[::max(1, ids.size // 23)][:24]
        assert span.min() < lo1 and span.max() >= lo_last
        both("explicit rows spanning all shards", candidates=span)
        both("explicit rows in the last shard", candidates=ids[ids >= lo_last][-9:][::-1].copy())
        outside = np.array([ids[0], int(np.flatnonzero(~stripes)[0]), ids[-1]])
        e = both("a candidate outside S", want_ok=False, candidates=outside)
        report.append(("... is a ValueError", e[0] == "ValueError" and "outside the safe set" in e[1]))
        # ---- edited safe sets
        mask = np.zeros(N, dtype=bool)
        mask[lo1 + 5:lo1 + 200] = True
        mask[lo_last + 20:N - 40] = True
        edit(mask)
        a = both("rank 0 without a safe row", candidates=40)
        report.append(("... rows from the other shards", bool(a[0] == "ok" and a[3].min() >= lo1)))
        mask = np.zeros(N, dtype=bool)
        mask[lo_last + 3:lo_last + 150] = True
        edit(mask)
        a = both("safe set in the last shard", candidates=12)
        report.append(("... rows from the last shard", bool(a[0] == "ok" and a[3].min() >= lo_last)))
        mask = np.ones(N, dtype=bool)
        mask[lo1 + 40:lo1 + 90] = False
        edit(mask)
        a = both("every unsafe row in rank 1's shard", candidates=40)
        report.append(("... every target there",
                       bool(a[0] == "ok" and np.all((a[5] >= lo1 + 40) & (a[5] < lo1 + 90)))))
        edit(np.ones(N, dtype=bool))
        e = both("S all true", want_ok=False, candidates=40)
        report.append(("... no row qualifies", e[0] == "RuntimeError" and "no row qualifies" in e[1]))
        a = both("S all true, about all", candidates=40, about='all')
        edit(np.zeros(N, dtype=bool))
        e = both("S all false", want_ok=False, candidates=40)
        report.append(("... no safe points", e[0] == "RuntimeError" and "no safe points" in e[1]))
        e = both("S all false, explicit rows", want_ok=False, candidates=np.array([3, N - 1]))
        report.append(("... no safe points either", e[0] == "RuntimeError"))
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
            assert len(out[what]) == len(out0[what]), (rank, what)
            for u, w in zip(out[what], out0[what]):
                assert np.array_equal(u, w), (rank, what)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("in_stream", [True, False], ids=["device-merge", "host-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_ise_point_bit_identical(hip_device, world, in_stream):
    _ranks_agree(_launch(_worker, world, in_stream))


def test_library_has_the_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_grid_ise_keys", "sgp_grid_ise_hist", "sgp_grid_ise_list",
                 "sgp_grid_ise_at", "sgp_grid_ise_comm"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
