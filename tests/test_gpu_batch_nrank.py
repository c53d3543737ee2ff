"""``SafeOpt.optimize_batch`` on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4: N operating-system processes, each with its own HIP context on device 0 and its
TRUE shard of the grid, connected by ``safeopt_amd.dist.SocketComm`` (the pattern of
tests/test_gpu_swarm_nrank.py: RCCL wants one GPU per rank).  Every rank runs the N-rank
product, then the same problem with ``LocalComm()`` IN THE SAME PROCESS, and must arrive at
its bits: ``X``, ``rows``, ``var_h``; the parent checks that all ranks hold the same bits.
With ``SAFEOPT_SOCKET_IN_STREAM=1`` a pick is ``sgp_grid_batch_next_comm`` (the records
gathered at the point where RCCL's all-gather is enqueued, ``k_batch_merge`` on the device);
with ``=0`` the shard's ``sgp_grid_batch_next``, one ``allgather`` and
``dist.merge_batch_records``.

The problems are those of tests/test_gpu_batch.py (``case`` / ``build``, the communicator
handed through by a wrapper): 37 x 41 = 1517 rows -- shards of 759 / 758 and 380 / 379 / 379 /
379 rows, every one ending in a partial 64-row workgroup.

* A-RBF, A-Matern52: n = 12, size 6; the picks land on more than one shard.
* E-RBF: ``ucb=True``; shape and bits of ``var_h (G, N)``, ``rows.dtype == int64``.
* C: three GPs of which two share a factor, a context column, an extra observation,
  Matern-5/2 and RBF, n = 100 / 99, size 5.
* the sets run out: |M u G| = 3 rows, all in ONE shard, size 8: exactly three rows on every
  rank; the shards without an eligible row never win and nobody is left waiting.
* ties across ranks: the 23 x 11 grid stacked on itself (506 rows); at world 2 the shard
  boundary is the duplicate boundary, rows r and r + 253 carry equal values and every pick
  takes the lower of the two in the merge.

Afterwards, on every rank: ``Q / S / M / G`` and the next ``add_new_data_point`` +
``optimize()`` equal those of a twin that only called ``optimize()``.

At most 4 worker processes plus the parent hold the GPU at once.
"""
import functools
import os
import socket
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA = 2.0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _init(rank, world, port, in_stream):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      SAFEOPT_COMM="socket", SAFEOPT_HIP_DEVICE="0",
                      SAFEOPT_SOCKET_IN_STREAM=in_stream)
    sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
    from safeopt_amd import dist
    ctx, comm = dist.init_from_env()
    assert isinstance(comm, dist.SocketComm) and comm.world == world
    assert comm.in_stream == (in_stream == "1")
    return ctx, comm


def _build(tb, mods, c, comm):
    """``test_gpu_batch.build`` with the communicator handed to ``SafeOpt``."""
    sa = types.SimpleNamespace(SafeOpt=functools.partial(mods[0].SafeOpt, comm=comm))
    return tb.build((sa,) + tuple(mods[1:]), c)


def _shards_of(rows, N, world):
    from safeopt_amd import dist
    edges = [dist.shard_range(N, r, world)[0] for r in range(world)] + [N]
    return sorted(set(int(np.searchsorted(edges, r, side="right")) - 1 for r in rows))


def _same_afterwards(opt, twin, x0, context, ucb):
    """``Q / S / M / G`` and the step after the next measurement against the twin."""
    ok = all(np.array_equal(np.array(getattr(opt, k)), np.array(getattr(twin, k)))
             for k in "QSMG")
    y = np.array([[1.3 + 0.1 * i for i in range(len(opt.gps))]])
    for o in (opt, twin):
        o.add_new_data_point(x0, y, context=context)
    xa = opt.optimize(context=context, ucb=ucb)
    xb = twin.optimize(context=context, ucb=ucb)
    return bool(ok and np.array_equal(xa, xb) and all(
        np.array_equal(np.array(getattr(opt, k)), np.array(getattr(twin, k))) for k in "QSMG"))


def _named_case(tb, mods, comm, name, report, out, world):
    from safeopt_amd import dist
    c = tb.case(name)
    N, G = c['grid'].shape[0], len(c['gps'])
    kw = dict(size=c['size'], context=c['context'], ucb=c['ucb'], return_state=True)
    opt = _build(tb, mods, c, comm)
    assert opt._shard == dist.shard_range(N, comm.rank, world) and (opt._shard[1] - opt._shard[0]) % 64
    X, rows, var_h = opt.optimize_batch(**kw)
    one = _build(tb, mods, c, dist.LocalComm())
    X1, rows1, var1 = one.optimize_batch(**kw)
    report.append((name + " X", np.array_equal(X, X1) and X.shape == (c['size'], 2)))
    report.append((name + " rows", np.array_equal(rows, rows1) and rows.dtype == np.int64
                   and len(set(rows.tolist())) == c['size']))
    report.append((name + " var_h", var_h.shape == (G, N) and var_h.dtype == np.float64
                   and np.array_equal(var_h, var1)))
    if name.startswith('A'):
        report.append((name + " picks on more than one shard",
                       len(_shards_of(rows, N, world)) > 1))
    # without the state: the points alone
    report.append((name + " X alone", np.array_equal(
        _build(tb, mods, c, comm).optimize_batch(size=c['size'], context=c['context'],
                                                 ucb=c['ucb']), X1)))
    twin = _build(tb, mods, c, comm)
    x_twin = twin.optimize(context=c['context'], ucb=c['ucb'])
    report.append((name + " row 0 is optimize()", np.array_equal(X[0], x_twin)))
    report.append((name + " afterwards", _same_afterwards(opt, twin, X[0], c['context'],
                                                           c['ucb'])))
    out[name] = (X, rows, var_h)


def _sets_run_out(tb, mods, comm, report, out, world):
    """|M u G| = 3, the three rows in one shard of the world-4 split (the split of world 2
    joins pairs of them), size 8."""
    from safeopt_amd import _hip, dist
    c = tb.case('A-RBF')
    res = []
    for cm in (comm, dist.LocalComm()):
        opt = _build(tb, mods, c, cm)
        opt.optimize()
        N = opt.inputs.shape[0]
        mg = np.flatnonzero(np.array(opt.M) | np.array(opt.G))
        # (the shard of the world-4 split with the most rows of M | G: the same on every rank)
        per = [mg[(mg >= lo) & (mg < hi)] for lo, hi in
               (dist.shard_range(N, r, 4) for r in range(4))]
        inside = max(per, key=len)
        assert inside.size >= 3, [p.size for p in per]
        keep = inside[[0, inside.size // 2, inside.size - 1]]
        m = np.zeros(N, dtype=bool)
        m[keep[:2]] = True
        g = np.zeros_like(m)
        g[keep[2]] = True
        opt.M[:] = m
        opt.G[:] = g
        x0 = opt.get_new_query_point()                 # (uploads the masks)
        row0 = int(np.flatnonzero((opt.inputs == x0).all(1))[0])
        assert row0 in keep
        rows, downdates, var_h = opt._backend.batch(
            opt.inputs, row0, 8, _hip.ARGMAX_MG_WIDTH, BETA, opt.scaling, want_var=True,
            **({'comm': cm} if cm.world > 1 else {}))
        res.append((rows, downdates, var_h, keep))
    (rows, downdates, var_h, keep), (rows1, downdates1, var1, _k) = res
    report.append(("sets run out: three rows", sorted(rows.tolist()) == sorted(keep.tolist())
                   and len(_shards_of(keep, 1517, world)) == 1))
    report.append(("sets run out: the one-rank bits", np.array_equal(rows, rows1)
                   and downdates == downdates1 == 3 and np.array_equal(var_h, var1)))
    out["sets run out"] = (rows, var_h)


def _ties(mods, comm, report, out, world):
    """The grid stacked on itself: rows r and r + 253 are the same point."""
    sa, gpy = mods[0], mods[1]
    from safeopt_amd import dist
    g = sa.linearly_spaced_combinations([(-2.0, 2.0)] * 2, [23, 11])
    assert g.shape[0] == 253
    rng = np.random.default_rng(11)
    Xo = rng.uniform(-1.5, 1.5, size=(12, 2))
    Y = (1.0 + np.exp(-(Xo ** 2).sum(1) / 2) + 0.05 * rng.normal(size=12))[:, None]
    res = []
    for cm in (comm, dist.LocalComm()):
        gp = gpy.models.GPRegression(Xo, Y, gpy.kern.RBF(2, 1.7, [0.8, 1.6], ARD=True),
                                     noise_var=0.05 ** 2)
        opt = sa.SafeOpt(gp, np.vstack([g, g]), 0.0, threshold=0.2, beta=BETA, comm=cm)
        res.append(opt.optimize_batch(size=6, return_state=True))
    (X, rows, var_h), (X1, rows1, var1) = res
    report.append(("ties: the one-rank bits", np.array_equal(X, X1) and np.array_equal(rows, rows1)
                   and np.array_equal(var_h, var1) and len(rows) == 6))
    # duplicates carry equal values (a row's value does not depend on its position in the
    # launch: the one-rank run itself stays below 253), so every pick is "the lowest global
    # row among equal values" -- inside the shard at world 2's rank 0, in the merge otherwise
    report.append(("ties: the lower of two equal rows",
                   bool(np.all(rows1 < 253) and np.all(rows < 253))))
    report.append(("ties: duplicates have equal variances",
                   np.array_equal(var_h[:, :253], var_h[:, 253:])))
    out["ties"] = (X, rows, var_h)


def _worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from oracle import gp_numpy as gpn, safeopt_numpy as son
        import test_gpu_batch as tb
        mods = (sa, gpy, gpn, son)
        report, out = [], {}
        for name in ('A-RBF', 'A-Matern52', 'E-RBF', 'C'):
            _named_case(tb, mods, comm, name, report, out, world)
        _sets_run_out(tb, mods, comm, report, out, world)
        _ties(mods, comm, report, out, world)
        comm.barrier()
        comm.close()
        q.put((rank, [(w, bool(ok)) for w, ok in report], out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _launch(world, in_stream):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    port = _free_port()
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, world, port, in_stream, q))
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
            print("rank %d  %-50s %s" % (rank, what, "ok" if ok else "MISMATCH"))
        assert all(ok for _what, ok in report), (rank, report)
    return results


@pytest.mark.timeout(300)
@pytest.mark.parametrize("in_stream", ["1", "0"], ids=["device-merge", "host-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_grid_batch_bit_identical(hip_device, world, in_stream):
    results = _launch(world, in_stream)
    out0 = results[0][2]
    for rank, _report, out, _err in results[1:]:
        assert sorted(out) == sorted(out0)
        for what in out0:
            for u, w in zip(out[what], out0[what]):
                assert np.array_equal(u, w), (rank, what)


def test_library_has_the_entry_point(hip_device):
    from safeopt_amd import _hip
    assert "sgp_grid_batch_next_comm" in _hip.PROTOTYPES
    assert hasattr(_hip.lib(), "sgp_grid_batch_next_comm")
