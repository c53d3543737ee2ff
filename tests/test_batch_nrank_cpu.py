"""``optimize_batch`` on N ranks without a GPU: the host form of the record merge
(``dist.merge_batch_records``), the gate of both classes, the loop of the device backend on
stand-ins for the device objects -- two ranks as two threads behind a barrier -- and the
assembly of ``var_h`` from uneven shards."""
import logging
import threading
import types

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import safeopt_amd
from _oracle_backend import OracleGridBackend
from oracle import gp_numpy as gpn
from safeopt_amd import _hip, dist, gp_opt


# ---- the merge rule ------------------------------------------------------------------------
def test_merge_takes_the_largest_value():
    recs = [[1.0, 7, 0], [3.0, 900, 0], [2.0, 2, 0]]
    assert dist.merge_batch_records(recs) == (3.0, 900, False)


def test_merge_takes_the_lowest_row_among_equal_values():
    recs = [[2.5, 400, 0], [2.5, 31, 0], [2.5, 77, 0], [1.0, 3, 0]]
    assert dist.merge_batch_records(recs) == (2.5, 31, False)
    # ... in whatever order the ranks hold them
    assert dist.merge_batch_records(recs[::-1]) == (2.5, 31, False)


def test_merge_never_lets_a_shard_without_a_row_win():
    # (-inf, -1) is what an empty shard sends; a row of -1 loses whatever value comes with it
    recs = [[-np.inf, -1, 0], [-4.0, 12, 0], [99.0, -1, 0]]
    assert dist.merge_batch_records(recs) == (-4.0, 12, False)
    # a row with the value -inf still beats no row
    assert dist.merge_batch_records([[-np.inf, -1, 0], [-np.inf, 5, 0]]) == (-np.inf, 5, False)


def test_merge_of_empty_shards_is_empty():
    v, i, stop = dist.merge_batch_records([[-np.inf, -1, 0]] * 4)
    assert v == -np.inf and i == -1 and stop is False
    assert isinstance(i, int)


def test_merge_stops_all_ranks_when_one_stops():
    recs = [[1.0, 7, 0], [-np.inf, -1, 1], [2.0, 9, 0]]
    assert dist.merge_batch_records(recs) == (2.0, 9, True)
    assert dist.merge_batch_records(np.array(recs)[[1]]) == (-np.inf, -1, True)
    # what comm.allgather hands over: (world, 3) float64
    assert dist.merge_batch_records(np.array(recs, dtype=np.float64))[2] is True


# ---- the gate ------------------------------------------------------------------------------
class _NoCollectives(object):
    rank, world = 0, 2

    def allreduce_max(self, a):
        raise AssertionError("a collective ran")

    allgather = barrier = allreduce_max


class _BatchBackend(OracleGridBackend):
    reached = []

    def batch(self, inputs, row0, size, mode, beta, scaling, want_var=False, comm=None):
        type(self).reached.append(comm)
        return np.array([row0], dtype=np.int64), 0, None


def _grid_opt(comm):
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, size=(5, 1))
    Y = 1.5 + 0.3 * np.sin(2 * X) + 0.01 * rng.normal(size=(5, 1))
    gp = gpn.GPRegression(X, Y, gpn.RBF(1, variance=1.0, lengthscale=0.7), noise_var=1e-4)
    grid = safeopt_amd.linearly_spaced_combinations([(-3.0, 3.0)], 61)
    return safeopt_amd.SafeOpt(gp, grid, 0.0, threshold=0.05, comm=comm)


def test_grid_two_ranks_without_a_context_raise_before_anything_runs():
    _BatchBackend.reached = []
    gp_opt._BACKEND_FACTORY = _BatchBackend
    opt = _grid_opt(_NoCollectives())
    with pytest.raises(NotImplementedError, match="one rank"):
        opt.optimize_batch(size=4)
    assert _BatchBackend.reached == []


def test_grid_two_ranks_with_a_context_reach_the_backend():
    _BatchBackend.reached = []
    gp_opt._BACKEND_FACTORY = _BatchBackend

    class WithCtx(_NoCollectives):
        ctx = object()
    comm = WithCtx()
    opt = _grid_opt(comm)
    ran = []
    opt.optimize = lambda context=None, ucb=False: ran.append(1) or opt.inputs[7]
    opt._argmax_cache = (1.0, 7)
    X = opt.optimize_batch(size=4)
    assert ran == [1] and _BatchBackend.reached == [comm]
    assert_array_equal(X, opt.inputs[[7]])
    # one rank: the backend is called as before, without the keyword
    _BatchBackend.reached = []
    one = _grid_opt(None)
    one.optimize = lambda context=None, ucb=False: one.inputs[7]
    one._argmax_cache = (1.0, 7)
    one.optimize_batch(size=4)
    assert _BatchBackend.reached == [None]


class _SwarmStub(object):
    """What SafeOptSwarm.optimize_batch touches before it runs anything."""

    def __init__(self, comm):
        self._comm = comm
        self.calls = 0

    def optimize(self, ucb=False):
        self.calls += 1
        raise RuntimeError("reached optimize()")


def test_swarm_two_ranks_without_a_context_raise_before_anything_is_drawn():
    stub = _SwarmStub(types.SimpleNamespace(world=2, rank=0))
    state = np.random.get_state()[1].copy()
    with pytest.raises(NotImplementedError, match="one rank"):
        gp_opt.SafeOptSwarm.optimize_batch(stub, size=4)
    assert stub.calls == 0
    assert_array_equal(np.random.get_state()[1], state)
    stub = _SwarmStub(types.SimpleNamespace(world=2, rank=0, ctx=None))
    with pytest.raises(NotImplementedError, match="one rank"):
        gp_opt.SafeOptSwarm.optimize_batch(stub, size=4)
    assert stub.calls == 0


def test_swarm_two_ranks_with_a_context_pass_the_gate():
    stub = _SwarmStub(types.SimpleNamespace(world=2, rank=0, ctx=object()))
    with pytest.raises(RuntimeError, match="reached optimize"):
        gp_opt.SafeOptSwarm.optimize_batch(stub, size=4)
    assert stub.calls == 1


def test_hallucinated_swarm_objects_take_a_communicator():
    from safeopt_amd.swarm import DeviceSwarmOptimization

    class World2(object):
        rank, world = 1, 2

        def allgather(self, a):
            raise AssertionError("a collective ran")
    sw = DeviceSwarmOptimization(7, np.array([0.1, 0.1]), None, 'expanders', seed=3,
                                 comm=World2())
    sw.set_clones([object(), object()])
    assert sw._rows == (4, 7) and len(sw._clones) == 2
    for name in ("sgp_swarm_run_hall_shard", "sgp_grid_batch_next_comm"):
        assert name in _hip.PROTOTYPES
    assert (_hip.PROTOTYPES["sgp_swarm_run_hall_shard"][1]
            == _hip.PROTOTYPES["sgp_swarm_run_hall"][1] + [_hip.C.c_int64] * 2)


# ---- the loop of the device backend on two ranks --------------------------------------------
class _ThreadComm(object):
    """Two ranks in two threads: an all-gather through a barrier."""

    def __init__(self, rank, world, shared, in_stream=False):
        self.rank, self.world, self._s, self.in_stream = rank, world, shared, in_stream
        self.gathers = 0

    def allgather(self, a):
        s = self._s
        self.gathers += 1
        s['slots'][self.rank] = np.array(a, copy=True)
        s['barrier'].wait(timeout=20)
        out = np.stack(s['slots'])
        s['barrier'].wait(timeout=20)
        return out


class _Clone(object):
    def __init__(self, book, fail_at):
        self.appends, self.fail_at, self.book = 0, fail_at, book
        book.append(self)
        self.alive = True

    def append(self, x, y):
        self.appends += 1
        return self.appends != self.fail_at

    def destroy(self):
        self.alive = False


class _Dev(object):
    def __init__(self, book, fail_at=0):
        self.book, self.fail_at = book, fail_at

    def clone(self):
        return _Clone(self.book, self.fail_at)


class _ShardGrid(object):
    """A shard whose pick number k is ``table[k]`` = (value, global row)."""

    def __init__(self, table, comm=None, boom_at=0):
        self.table, self.calls, self.comm, self.boom_at = table, [], comm, boom_at
        self.stops = []

    def batch_next(self, clones, first, mode, beta, scaling, picked):
        self.calls.append((bool(first), list(picked)))
        if len(self.calls) == self.boom_at:
            raise RuntimeError("device error")
        return self.table[len(self.calls) - 1]

    def batch_next_comm(self, clones, first, mode, beta, scaling, picked, stop=False):
        # the library's in-stream form: its own all-gather and merge
        self.stops.append(bool(stop))
        v, i = (-np.inf, -1) if stop else self.batch_next(clones, first, mode, beta, scaling,
                                                          picked)
        return dist.merge_batch_records(
            self.comm.allgather(np.array([v, float(i), float(stop)])))

    def download(self, what):
        lo, hi = dist.shard_range(41, self.comm.rank, 2)               # 21 and 20 rows
        return np.full((2, hi - lo), 1.0 if what == _hip.VAR_H else 0.0)


def _backend(devs, grid):
    be = object.__new__(gp_opt._HipGridBackend)
    be._dev = lambda: devs
    be.posterior_is_current = lambda: True
    be.grid = grid
    return be


def _two_ranks(tables, fail_at, size, in_stream, boom_at=(0, 0), want_var=False):
    shared = dict(slots=[None, None], barrier=threading.Barrier(2))
    out, books = [None, None], [[], []]
    comms = [_ThreadComm(r, 2, shared, in_stream) for r in range(2)]
    grids = [_ShardGrid(tables[r], comms[r], boom_at[r]) for r in range(2)]

    def rank(r):
        be = _backend([_Dev(books[r]), _Dev(books[r], fail_at[r])], grids[r])
        try:
            out[r] = be.batch(np.arange(41.0)[:, None], 3, size, 0, 2.0, [1.0, 1.0],
                              want_var=want_var, comm=comms[r])
        except Exception as e:                       # noqa: BLE001 (handed to the test)
            out[r] = e
            shared['barrier'].abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in threads), "a rank is left waiting in a collective"
    return out, books, grids, comms


@pytest.mark.parametrize("in_stream", [False, True], ids=["host-merge", "library-merge"])
def test_picks_alternate_between_the_shards(in_stream):
    tables = [[(5.0, 10), (1.0, 11), (-np.inf, -1), (-np.inf, -1)],
              [(4.0, 30), (3.0, 30), (3.0, 30), (-np.inf, -1)]]
    out, books, grids, comms = _two_ranks(tables, (0, 0), 8, in_stream, want_var=True)
    assert not any(isinstance(o, Exception) for o in out), out
    # picks: 10 (5 > 4), 30 (3 > 1), the table's (3, 30) against a shard without a row, none
    assert out[0][0].tolist() == out[1][0].tolist() == [3, 10, 30, 30]
    assert out[0][1] == out[1][1] == 4
    for r in range(2):
        assert grids[r].calls == [(True, [3]), (False, [3, 10]), (False, [3, 10, 30]),
                                  (False, [3, 10, 30, 30])]
        assert all(not c.alive for c in books[r]) and len(books[r]) == 2
        # ONE collective per pick, then the gathers of var_h: one per GP
        assert comms[r].gathers == 4 + 2
        assert out[r][2].shape == (2, 41) and np.all(out[r][2] == 1.0)
        assert out[r][0].dtype == np.int64


@pytest.mark.parametrize("in_stream", [False, True], ids=["host-merge", "library-merge"])
def test_a_rank_whose_append_fails_still_makes_its_collective_call(in_stream, caplog):
    tables = [[(5.0, 10), (1.0, 11), (1.0, 12)], [(4.0, 30), (3.0, 31), (3.0, 32)]]
    # rank 1's second GP fails at its third append: pick 3 never comes
    with caplog.at_level(logging.INFO, logger='safeopt_amd.gp_opt'):
        out, books, grids, comms = _two_ranks(tables, (0, 3), 6, in_stream)
    assert not isinstance(out[0], Exception) and not isinstance(out[1], Exception), out
    assert out[0][0].tolist() == out[1][0].tolist() == [3, 10, 31]        # k = 3 < size
    # both ranks made three collective calls; the rank that stopped ran no third row kernel
    assert comms[0].gathers == comms[1].gathers == 3
    assert len(grids[0].calls) == 3 and len(grids[1].calls) == 2
    if in_stream:
        assert grids[0].stops == [False] * 3 and grids[1].stops == [False, False, True]
    # downdates: what the rank's own var_h accounts for
    assert out[0][1] == 3 and out[1][1] == 2
    assert all(not c.alive for r in range(2) for c in books[r])
    recs = [r for r in caplog.records if 'non-positive pivot' in r.getMessage()]
    assert len(recs) == 1 and recs[0].levelno == logging.INFO             # once, on rank 1


def test_the_clones_are_released_when_a_call_raises_after_a_collective():
    tables = [[(5.0, 10), (1.0, 11), (1.0, 12)], [(4.0, 30), (3.0, 31), (3.0, 32)]]
    out, books, grids, comms = _two_ranks(tables, (0, 0), 6, False, boom_at=(2, 2))
    assert all(isinstance(o, RuntimeError) for o in out)
    assert comms[0].gathers == 1                      # (the first pick's collective ran)
    assert all(not c.alive for r in range(2) for c in books[r])


def test_one_rank_loop_is_unchanged_by_the_keyword():
    book = []
    grid = _ShardGrid([(1.0, 10), (1.0, 11), (1.0, 12)])
    be = _backend([_Dev(book)], grid)
    rows, downdates, _ = be.batch(np.arange(40.0)[:, None], 3, 4, 0, 2.0, [1.0],
                                  comm=dist.LocalComm())
    assert rows.tolist() == [3, 10, 11, 12] and downdates == 3 and grid.stops == []


# ---- var_h over uneven shards ----------------------------------------------------------------
class _ReplayComm(object):
    """Rank ``rank`` of ``world``: all-gathers return what every rank would send."""

    def __init__(self, rank, parts):
        self.rank, self.world, self._parts, self.sent = rank, len(parts), parts, []

    def allgather(self, a):
        g = len(self.sent)
        self.sent.append(np.array(a))
        pad = a.shape[0]
        blocks = []
        for p in self._parts:
            b = np.zeros(pad)
            b[:p.shape[1]] = p[g]
            blocks.append(b)
        return np.stack(blocks)


@pytest.mark.parametrize("N, world", [(10, 4), (7, 2), (5, 5), (9, 4)])
def test_var_h_is_assembled_in_global_row_order(N, world):
    G = 3
    full = np.arange(G * N, dtype=float).reshape(G, N) + 0.5
    parts = [full[:, slice(*dist.shard_range(N, r, world))] for r in range(world)]
    assert len({p.shape[1] for p in parts}) == (1 if N % world == 0 else 2)
    for r in range(world):
        comm = _ReplayComm(r, parts)
        got = dist.gather_shard_columns(comm, parts[r], N)
        assert got.shape == (G, N)
        assert_array_equal(got, full)
        assert len(comm.sent) == G                   # one all-gather per GP
        # a short shard is padded to the longest one
        assert all(s.shape == (-(-N // world),) for s in comm.sent)
