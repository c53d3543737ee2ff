"""Host side of the N-rank Thompson picks (no GPU).

1. ``dist.merge_argmax`` / ``dist.merge_path_records`` on hand-made path records: the largest
   value, the lowest global row among equals, a shard without a row never wins.
2. ``SafeOpt.thompson_points`` in world 2 over real gloo (the pattern of
   tests/test_dist_gloo.py), with a NumPy backend that evaluates the paths through
   tests/_paths_numpy.py: ``x``, ``values``, the gathered ``(N, size)`` array and the state of
   NumPy's generator equal the unsharded run bit for bit; paths that differ between the ranks
   raise ``ValueError`` and an all-unsafe ``S`` raises ``RuntimeError`` -- on BOTH ranks, and
   neither rank is left waiting (the workers are joined with a timeout).

Bit for bit on the CPU: ``_paths_numpy.paths_eval`` goes through BLAS, whose blocking may
depend on the number of rows; the backend below therefore evaluates ONE row per call -- the
same shapes, hence the same bits, for a row of a shard and the same row of the whole grid.
"""
import os
import sys

import numpy as np
import pytest

from test_dist_gloo import TorchComm, _free_port, _needs_torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZE, FEATURES = 5, 32
NOISE = 0.05 ** 2


# ---- 1. the merge ------------------------------------------------------------------------------

def test_merge_argmax_on_path_records():
    from safeopt_amd.dist import merge_argmax
    # a tie across ranks: the lowest global row
    assert merge_argmax([1.5, 1.5, 0.2], [40, 7, 90]) == (1.5, 7)
    assert merge_argmax([1.5, 1.5], [7, 40]) == (1.5, 7)
    # the largest value wins whatever its row
    assert merge_argmax([0.5, 2.0], [3, 50]) == (2.0, 50)
    # a rank without a qualifying row never wins, not even against -inf with a row
    assert merge_argmax([-np.inf, -3.0], [-1, 12]) == (-3.0, 12)
    assert merge_argmax([-np.inf, -np.inf], [-1, 12]) == (-np.inf, 12)
    # ... whatever value it carries
    assert merge_argmax([9.0, -3.0], [-1, 12]) == (-3.0, 12)
    # all ranks empty
    assert merge_argmax([-np.inf, -np.inf, -np.inf], [-1, -1, -1]) == (-np.inf, -1)


def test_merge_path_records():
    from safeopt_amd.dist import merge_path_records
    inf = np.inf
    #            tie      rank 1 empty   all empty   rank 0 empty   plain
    vals = np.array([[1.5, 0.25, -inf, -inf, -1.0],
                     [1.5, -inf, -inf, -2.0, 3.0],
                     [0.1, 0.25, -inf, -2.0, 2.0]])
    rows = np.array([[11, 3, -1, -1, 0],
                     [25, -1, -1, 29, 20],
                     [44, 41, -1, 40, 47]])
    bv, bi = merge_path_records(vals, rows)
    assert bi.dtype == np.int64
    np.testing.assert_array_equal(bv, [1.5, 0.25, -inf, -2.0, 3.0])
    np.testing.assert_array_equal(bi, [11, 3, -1, 29, 20])
    # the order of the ranks does not matter
    bv2, bi2 = merge_path_records(vals[::-1], rows[::-1])
    np.testing.assert_array_equal(bv2, bv)
    np.testing.assert_array_equal(bi2, bi)


# ---- 2. world 2 over gloo ----------------------------------------------------------------------

def _problem():
    rng = np.random.RandomState(11)
    X = rng.uniform(-1.5, 1.5, (6, 2))
    Y = (1.0 + 0.5 * np.cos(X).prod(1))[:, None]
    from safeopt_amd import linearly_spaced_combinations
    grid = linearly_spaced_combinations([[-2., 2.], [-2., 2.]], [9, 7])      # 63 rows: 32 | 31
    return X, Y, grid


def _make_backend_and_gp():
    """A NumPy grid backend with ``paths`` and an oracle GP with ``posterior_paths``."""
    import _paths_numpy as pn
    from oracle import gp_numpy as gpn
    from _oracle_backend import OracleGridBackend
    from safeopt_amd import paths as P

    ls, var = np.array([0.8, 1.1]), 1.5
    kern = ([pn.RBF], [var], [list(1.0 / ls)])

    class PathsGP(gpn.GPRegression):
        def posterior_paths(self, size=16, features=1024):
            X, y = self.X.copy(), self.Y[:, 0].copy()
            Om, b, W, E = P.draw_path_inputs((kern[0], kern[2]), self.noise_var, X.shape[0],
                                             X.shape[1], size, features)
            V = pn.path_weights(kern, self.noise_var, X, y, Om, b, W, E)

            def evaluate(Z):          # one row per call: see the module docstring
                return np.vstack([pn.paths_eval(kern, X, Om, b, W, V, Z[i:i + 1])
                                  for i in range(Z.shape[0])] or [np.empty((0, size))])
            return P.PosteriorPaths(Om, b, W, V, evaluate, lambda: X.shape[0])

    class PathsBackend(OracleGridBackend):
        def paths(self, pp, mask, values):
            f = pp.paths(self.x)[:, 0, :]
            rows = np.flatnonzero(self.S) if mask else np.arange(self.x.shape[0])
            S = f.shape[1]
            bv, bi = np.full(S, -np.inf), np.full(S, -1, dtype=np.int64)
            if rows.size:
                j = rows[np.argmax(f[rows], axis=0)]              # first among equals
                bv, bi = f[j, np.arange(S)], j + self.lo
            return (f if values else None), bv, bi

    def make_gp(X, Y):
        return PathsGP(X, Y, gpn.RBF(2, var, ls, ARD=True), noise_var=NOISE)
    return PathsBackend, make_gp


def _pick(opt, seed):
    np.random.seed(seed)
    x, v, vals = opt.thompson_points(size=SIZE, features=FEATURES, return_values=True)
    state = np.random.get_state()
    return x, v, vals, state


def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
        import torch.distributed as td
        td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                              rank=rank, world_size=world)
        import safeopt_amd
        import safeopt_amd.gp_opt as go
        from safeopt_amd.dist import LocalComm
        backend, make_gp = _make_backend_and_gp()
        go._BACKEND_FACTORY = backend
        comm = TorchComm()
        X, Y, grid = _problem()
        out = {}

        def make(c):
            opt = safeopt_amd.SafeOpt(make_gp(X, Y), grid, 0.9, threshold=0.1, comm=c)
            opt.optimize()
            return opt
        opt, one = make(comm), make(LocalComm())
        lo, hi = opt._shard
        assert hi - lo < grid.shape[0]                           # really sharded
        S = np.array(one.S)
        out["safe_rows"] = int(S.sum())
        assert 0 < S.sum() < S.size                              # 'safe' differs from 'all'

        # ---- the picks, against the unsharded run in this process
        a, b = _pick(opt, 3), _pick(one, 3)
        out["picks"] = [np.array_equal(u, w) for u, w in zip(a[:3], b[:3])]
        out["rng"] = bool(a[3][0] == b[3][0] and np.array_equal(a[3][1], b[3][1])
                          and a[3][2:] == b[3][2:])
        out["x"], out["values"], out["all"] = a[:3]
        out["shape"] = a[2].shape == (grid.shape[0], SIZE)
        np.random.seed(3)
        xa, va = opt.thompson_points(size=SIZE, features=FEATURES, within='all')
        np.random.seed(3)
        xb, vb = one.thompson_points(size=SIZE, features=FEATURES, within='all')
        out["all_rows"] = bool(np.array_equal(xa, xb) and np.array_equal(va, vb))
        out["all_differs"] = not np.array_equal(xa, a[0])

        # ---- paths that differ between the ranks
        np.random.seed(100 + rank)
        try:
            opt.thompson_points(size=SIZE, features=FEATURES)
            out["differ"] = "no error"
        except ValueError as e:
            out["differ"] = "ValueError" if "different sample paths" in str(e) else str(e)
        comm.barrier()                                           # both ranks came out

        # ---- nothing is safe
        opt.S[:] = False
        np.random.seed(3)
        try:
            opt.thompson_points(size=SIZE, features=FEATURES)
            out["unsafe"] = "no error"
        except RuntimeError as e:
            out["unsafe"] = "RuntimeError" if "no safe points" in str(e) else str(e)
        comm.barrier()
        td.destroy_process_group()
        q.put((rank, out, None))
    except Exception:
        import traceback
        q.put((rank, {}, traceback.format_exc()))


@pytest.fixture(scope="module")
def two_ranks():
    _needs_torch()
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _free_port()
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
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
    for rank, _out, err in results:
        assert err is None, "rank %d failed:\n%s" % (rank, err)
    return [out for _rank, out, _err in results]


@pytest.mark.timeout(300)
def test_two_ranks_pick_what_one_rank_picks(two_ranks):
    for rank, out in enumerate(two_ranks):
        assert out["picks"] == [True, True, True], (rank, out["picks"])    # x, values, (N, size)
        assert out["shape"] and out["all_rows"], rank
        assert out["rng"], "rank %d: NumPy's generator is not where one rank leaves it" % rank
        assert out["all_differs"]          # (the safe mask matters in this problem)
    a, b = two_ranks
    for k in ("x", "values", "all"):
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.timeout(300)
def test_paths_that_differ_raise_on_both_ranks(two_ranks):
    assert [out["differ"] for out in two_ranks] == ["ValueError", "ValueError"]


@pytest.mark.timeout(300)
def test_all_unsafe_raises_on_both_ranks(two_ranks):
    assert [out["unsafe"] for out in two_ranks] == ["RuntimeError", "RuntimeError"]
