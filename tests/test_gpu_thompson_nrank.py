"""Thompson picks on N ranks: REAL processes on device 0 (needs an MI355X).

World 2 and 4: N operating-system processes, each with its own HIP context on device 0 and
its TRUE shard of the grid / block of the particles, connected by
``safeopt_amd.dist.SocketComm`` (the pattern of tests/test_gpu_swarm_nrank.py: RCCL wants one
GPU per rank).  Every rank must arrive, bit for bit, at what a ``LocalComm`` optimiser on the
whole grid / swarm computes IN THE SAME PROCESS from the same seed, and at what rank 0 holds.

Grid (``SafeOpt.thompson_points`` -> ``sgp_grid_paths_comm``, k_paths_merge): 37 x 41 = 1517
rows -- in world 4 shards of 379 / 380 rows, no multiple of the 64 rows of a k_paths tile and a
ragged last workgroup -- and, in world 4, 5 x 3 = 15 rows (shards of 3 or 4 rows: less than
one workgroup); RBF and Matern-5/2, 12 observations, ``size=5``, ``features=64``,
``within='safe'`` and ``'all'``.  With ``SAFEOPT_SOCKET_IN_STREAM=1`` the merge runs on the
device behind the in-stream all-gather; with ``=0`` the records are merged on the host
(``dist.merge_path_records``): the same bits.  (The host merge needs the variable at 0: left
unset, ``SocketComm`` registers itself as the context's transport and runs in stream.)
Through ``_hip.grid_paths_comm`` directly, with W = 0 and V = 0 (every path identically 0: all
rows tie): the lowest safe row wins wherever it lies, a mask confined to the last shard gives
a row of that shard, an empty mask -inf / -1 -- and ``thompson_points`` then raises
``RuntimeError`` on every rank.

Swarm (``SafeOptSwarm.thompson_points`` -> ``sgp_swarm_run_path_shard``): d = 3, two GPs,
n in {12, 100}, swarm_size in {203, 20} (203: not divisible by 4; 20: five particles a rank in
world 4), ``max_iters=5``, ``size=3``, ``features=64``, pso in {'device', 'device-rng'}: ``x``,
``values``, every swarm's gathered personal bests and global best, and the state of NumPy's
generator.

At most 4 worker processes plus the parent hold the GPU at once.
"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, FEATURES = 5, 64


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _smooth(x, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-3, 3, size=(10, x.shape[1]))
    w = rng.normal(size=10)
    r2 = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    return (np.exp(-0.25 * r2) * w).sum(1)[:, None]


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


def _same_state(a, b):
    return bool(a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:])


# ---- grid --------------------------------------------------------------------------------------

def _grid_opt(sa, gpy, comm, kind, shape):
    d = 2
    rng = np.random.default_rng(7)
    X = rng.uniform(-1.5, 1.5, size=(12, d))
    Y = _smooth(X, 41)
    Y = Y - Y.min() + 0.5
    kern = getattr(gpy.kern, kind)(d, 1.5, [0.7, 0.9], ARD=True)
    gp = gpy.models.GPRegression(X, Y, kern, noise_var=0.05 ** 2)
    grid = sa.linearly_spaced_combinations([[-2., 2.]] * d, list(shape))
    opt = sa.SafeOpt(gp, grid, 0.0, threshold=0.1, comm=comm)
    opt.update_confidence_intervals()
    opt.compute_safe_set()               # S: 788 / 543 of 1517 rows, 4 / 3 of 15 (RBF / Matern)
    return opt


def _grid_worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import _hip, dist
        report, out = [], {}
        shapes = [(37, 41)] + ([(5, 3)] if world == 4 else [])
        for shape in shapes:
            for kind in ("RBF", "Matern52"):
                opt = _grid_opt(sa, gpy, comm, kind, shape)
                one = _grid_opt(sa, gpy, dist.LocalComm(), kind, shape)
                N = shape[0] * shape[1]
                lo, hi = opt._shard
                assert (lo, hi) == dist.shard_range(N, rank, world) and hi - lo < N
                S = np.array(one.S)
                same_S = np.array_equal(np.array(opt.S), S)
                for within in ("safe", "all"):
                    what = "%dx%d %s %s" % (shape + (kind, within))
                    res = []
                    for o in (opt, one):
                        np.random.seed(9)
                        x, v, vals = o.thompson_points(size=SIZE, features=FEATURES,
                                                       within=within, return_values=True)
                        res.append((x, v, vals, np.random.get_state()))
                    a, b = res
                    ok = (same_S and 0 < S.sum() < N and a[2].shape == (N, SIZE)
                          and all(np.array_equal(u, w) for u, w in zip(a[:3], b[:3]))
                          and _same_state(a[3], b[3]))
                    # without return_values: the same picks
                    np.random.seed(9)
                    x2, v2 = opt.thompson_points(size=SIZE, features=FEATURES, within=within)
                    ok = ok and np.array_equal(x2, a[0]) and np.array_equal(v2, a[1])
                    report.append((what, bool(ok)))
                    out[what] = a[:3]
        comm.barrier()
        comm.close()
        q.put((rank, report, out, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


def _direct_worker(rank, world, port, in_stream, q):
    """``_hip.grid_paths_comm`` with paths that are identically 0, under chosen safe masks."""
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import _hip, dist
        opt = _grid_opt(sa, gpy, comm, "RBF", (37, 41))
        N = 37 * 41
        be = opt._backend
        dev = opt.gp._fitted()
        rng = np.random.default_rng(3)
        m, S = FEATURES, SIZE
        Om, ph = rng.normal(size=(m, 2)), rng.uniform(0, 2 * np.pi, m)
        W0, V0 = np.zeros((m, S)), np.zeros((dev.n, S))
        lo, hi = opt._shard
        lo1 = dist.shard_range(N, 1, world)[0]
        lo_last = dist.shard_range(N, world - 1, world)[0]

        def run(rows, mask=True, values=False):
            full = np.zeros(N, dtype=bool)
            full[list(rows)] = True
            be.upload_mask(_hip.S, full[lo:hi])
            return _hip.grid_paths_comm(be.grid, dev, Om, ph, W0, V0, mask=mask, values=values)
        report = []
        # the lowest safe row lies in rank 1's shard; later ranks hold safe rows too
        first = lo1 + 5
        # (world 2: rank 1 is the last rank too -- every other row lies behind `first`)
        vals, bv, bi = run([first, first + 70, lo_last + 20, N - 1], values=True)
        report.append(("lowest safe row in rank 1's shard",
                       bool(np.all(bi == first) and np.all(bv == 0.0)
                            and vals.shape == (hi - lo, S) and np.all(vals == 0.0))))
        # the safe set confined to the last rank's shard
        _, bv, bi = run([lo_last + 3, N - 1])
        report.append(("safe set in the last shard", bool(np.all(bi == lo_last + 3)
                                                          and np.all(bv == 0.0))))
        # every row: row 0 wins the tie of all rows of all ranks
        _, bv, bi = run([first], mask=False)
        report.append(("all rows tie", bool(np.all(bi == 0) and np.all(bv == 0.0))))
        # nothing is safe
        _, bv, bi = run([])
        report.append(("empty mask", bool(np.all(bi == -1) and np.all(bv == -np.inf))))
        opt.S[:] = False
        np.random.seed(9)                    # (SPMD: the ranks draw the same paths)
        try:
            opt.thompson_points(size=3, features=16)
            report.append(("RuntimeError on every rank", False))
        except RuntimeError as e:
            report.append(("RuntimeError on every rank", "no safe points" in str(e)))
        comm.barrier()
        comm.close()
        q.put((rank, report, {}, None))
    except Exception:
        import traceback
        q.put((rank, [], {}, traceback.format_exc()))


# ---- swarm -------------------------------------------------------------------------------------

def _swarm_run(sa, gpy, comm, pso, n, P, runs):
    d, G = 3, 2
    rng = np.random.default_rng(n)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    Ys = [_smooth(X, 40 + g) - _smooth(X, 40 + g).min() + 0.5 for g in range(G)]
    gps = [gpy.models.GPRegression(X, Ys[g], gpy.kern.RBF(d, 1.5, [0.8, 1.0, 1.2], ARD=True),
                                   noise_var=0.05 ** 2) for g in range(G)]
    np.random.seed(5)
    opt = sa.SafeOptSwarm(gps, [0.0] * G, bounds=[(-3., 3.)] * d, threshold=0.1,
                          swarm_size=P, pso=pso, comm=comm)
    del runs[:]
    x, values = opt.thompson_points(size=3, features=64, max_iters=5)
    out = {"x": x, "values": values, "state": np.random.get_state()}
    assert len(runs) == 3                                   # one swarm per path
    for s, (bp, bv, gb) in enumerate(runs):
        assert bp.shape == (P, d) and bv.shape == (P,)      # gathered: the whole swarm
        out["best_positions%d" % s], out["best_values%d" % s] = bp, bv
        out["global_best%d" % s] = gb
    return out


def _swarm_worker(rank, world, port, in_stream, q):
    try:
        ctx, comm = _init(rank, world, port, in_stream)
        import safeopt_amd as sa
        import safeopt_amd.gpy as gpy
        from safeopt_amd import dist, swarm
        runs = []
        orig = swarm.DeviceSwarmOptimization.run_swarm

        def traced(self, *a, **k):
            orig(self, *a, **k)
            if self._type == 'thompson':
                runs.append((np.array(self.best_positions), np.array(self.best_values),
                             np.array(self.global_best)))
        swarm.DeviceSwarmOptimization.run_swarm = traced
        report, out = [], {}
        for pso in ("device", "device-rng"):
            for n in (12, 100):
                for P in (203, 20):
                    what = "%s n=%d P=%d" % (pso, n, P)
                    a = _swarm_run(sa, gpy, comm, pso, n, P, runs)
                    b = _swarm_run(sa, gpy, dist.LocalComm(), pso, n, P, runs)
                    bad = sorted(k for k in b if k != "state"
                                 and not np.array_equal(a[k], b[k]))
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


# ---- the parent --------------------------------------------------------------------------------

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
@pytest.mark.parametrize("in_stream", [True, False], ids=["device-merge", "host-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_grid_picks_bit_identical(hip_device, world, in_stream):
    _ranks_agree(_launch(_grid_worker, world, in_stream))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_grid_paths_comm_ties_and_empty_shards(hip_device, world):
    _launch(_direct_worker, world, True)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_thompson_swarm_bit_identical(hip_device, world):
    _ranks_agree(_launch(_swarm_worker, world, True))


def test_library_has_the_two_entry_points(hip_device):
    from safeopt_amd import _hip
    for name in ("sgp_grid_paths_comm", "sgp_swarm_run_path_shard"):
        assert name in _hip.PROTOTYPES and hasattr(_hip.lib(), name)
