"""The candidate selection of ``SafeOpt.ise_point`` where the variances are, and ``ise_point`` on N
ranks, without a GPU: the threshold and superset rule in NumPy against ``gp_opt.ise_candidates``
(device keys = NumPy keys perturbed by up to the bound ``ISE_KEY_EPS``, 1 / 2 / 4 shards), the
host form of the merge (``dist.merge_ise_records``), and N fake ranks -- threads behind a barrier,
the pattern of tests/test_batch_nrank_cpu.py -- over a NumPy backend that implements keys / hist /
list / ise_at: every rank must return what one rank returns, on the device path and on both
fall-backs to the host selection."""
import threading

import numpy as np
import pytest
from numpy.testing import assert_array_equal

import safeopt_amd
from _oracle_backend import OracleGridBackend
from oracle import gp_numpy as gpn
from safeopt_amd import dist, gp_opt
from safeopt_amd.gp_opt import (ISE_BINS, ISE_KEY_EPS, ise_candidates, ise_list_cap, ise_order,
                                ise_threshold)

INF = np.inf


# ---- 1. threshold and superset, pure NumPy ----------------------------------------------------
def _np_keys(var, s, active):
    key = np.zeros(var.shape[1])
    for g in np.flatnonzero(active):
        key = key + 0.5 * np.log1p(var[g] / s[g])
    return key


def _bins(key, lo, hi):
    """The bin ``k_ise_hist`` counts a key in (the rule of ``k_pass_hist``)."""
    return np.clip(((key - lo) * (ISE_BINS / (hi - lo))).astype(np.int64), 0, ISE_BINS - 1)


def _device_select(dev_key, S, var, s, active, K, shards):
    """``SafeOpt._ise_select`` over ``shards`` row blocks, on arrays: ``(listed rows, picked
    rows)`` or ``None`` for a fall-back."""
    ids = np.flatnonzero(S)
    n, lo, hi = ids.size, dev_key[ids].min(), dev_key[ids].max()
    eps = ISE_KEY_EPS * max(1.0, hi)
    if not hi - lo >= ISE_BINS * 2.0 * eps:
        return None
    N = S.size
    hist = np.zeros(ISE_BINS)
    for r in range(shards):
        a, b = dist.shard_range(N, r, shards)
        mine = ids[(ids >= a) & (ids < b)]
        hist += np.bincount(_bins(dev_key[mine], lo, hi), minlength=ISE_BINS)
    assert hist.sum() == n
    thr, listed = ise_threshold(hist, min(K, n), lo, hi)
    if listed > ise_list_cap(K):
        return None
    rows = ids[dev_key[ids] >= thr]                      # (ascending: the ranks' lists in order)
    at = ise_order(rows, var[:, rows].T, s, active, K)
    return rows, rows[at]


@pytest.mark.parametrize("shards", [1, 2, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_listed_set_holds_the_host_selection(seed, shards):
    rng = np.random.default_rng(seed)
    N, G = 3000, 3
    var = 10.0 ** rng.uniform(-6, 1, size=(G, N))
    if seed == 2:
        var = np.round(var, 3) + 1e-6                    # exact ties among the keys
    S = rng.random(N) < 0.4
    s = np.array([1e-4, 2.5e-3, 1e-2]) + 1e-8
    active = np.array([True, seed != 1, True])
    key = _np_keys(var, s, active)
    # the "device" keys: off by up to the bound, in the unit the bound is stated in
    dev = key + ISE_KEY_EPS * max(1.0, key[S].max()) * rng.uniform(-1.0, 1.0, N)
    nS = int(S.sum())
    for K in (1, 7, 64, nS, nS + 5):
        want = ise_candidates(var, S, s, active, K)
        got = _device_select(dev, S, var, s, active, K, shards)
        if got is None:                                  # (a mass of ties above the cap)
            assert seed == 2
            continue
        listed, picked = got
        assert np.all(np.isin(want, listed))
        assert_array_equal(picked, want)
        assert listed.size <= ise_list_cap(K) + 64
    assert _device_select(dev, S, var, s, active, 64, shards) is not None


def test_threshold_is_the_lower_edge_of_the_bin_below():
    hist = np.zeros(ISE_BINS)
    hist[[4095, 4000, 3999, 10]] = [3, 2, 5, 7]
    lo, hi = 1.0, 3.0
    edge = lambda b: lo + (hi - lo) * (float(b) / ISE_BINS)                  # noqa: E731
    assert ise_threshold(hist, 1, lo, hi) == (edge(4094), 3)
    assert ise_threshold(hist, 3, lo, hi) == (edge(4094), 3)
    assert ise_threshold(hist, 4, lo, hi) == (edge(3999), 10)    # b = 4000: bin 3999 comes along
    assert ise_threshold(hist, 6, lo, hi) == (edge(3998), 10)
    assert ise_threshold(hist, 11, lo, hi) == (edge(9), 17)
    assert ise_threshold(hist, 17, lo, hi) == (edge(9), 17)
    low = np.zeros(ISE_BINS)
    low[[1, 0]] = [2, 9]
    assert ise_threshold(low, 2, lo, hi) == (-INF, 11)           # b = 1: everything
    assert ise_threshold(low, 11, lo, hi) == (-INF, 11)


def test_the_bound_is_one_named_constant():
    assert ISE_KEY_EPS == 2.0 ** -46 and ISE_BINS == 4096
    assert ise_list_cap(64) == 4 * 64 + 4096


# ---- 2. the merge -----------------------------------------------------------------------------
def test_merge_ise_records():
    al = np.array([[0.5, 0.2, -INF, 0.7, -INF],
                   [0.5, 0.9, -INF, 9.0, -INF],
                   [0.1, 0.9, 0.3, 0.7, -INF]])
    tg = np.array([[40, 3, -1, 8, -1],
                   [7, 800, -1, -1, -1],
                   [90, 500, 12, 2, -1]])
    a, t = dist.merge_ise_records(al, tg)
    # ties take the lowest target; a rank without a target never wins (9.0 / -1); none: -inf / -1
    assert_array_equal(a, [0.5, 0.9, 0.3, 0.7, -INF])
    assert_array_equal(t, [7, 500, 12, 2, -1])
    assert t.dtype == np.int64
    a2, t2 = dist.merge_ise_records(al[::-1], tg[::-1])         # whatever the rank order
    assert_array_equal(a2, a)
    assert_array_equal(t2, t)
    empty = dist.merge_ise_records(np.full((4, 3), -INF), np.full((4, 3), -1))
    assert np.all(empty[0] == -INF) and np.all(empty[1] == -1)
    # the pick: the largest alpha, the lowest ROW among equals, no target never
    assert dist.pick_ise(a, t, np.array([9, 5, 4, 6, 1])) == (0.9, 5)
    assert dist.pick_ise([0.7, 0.7, 0.9], [3, 3, -1], np.array([9, 8, 1])) == (0.7, 8)
    assert dist.pick_ise([0.7, 0.9], [-1, -1], np.array([9, 8])) == (-INF, -1)


# ---- 3. N fake ranks --------------------------------------------------------------------------
class _ThreadComm(object):
    """``world`` ranks in as many threads: collectives through a barrier."""

    def __init__(self, rank, world, shared, in_stream):
        self.rank, self.world, self._s, self.in_stream = rank, world, shared, in_stream

    def allgather(self, a):
        s = self._s
        s['slots'][self.rank] = np.array(a, copy=True)
        s['barrier'].wait(timeout=20)
        out = np.stack(s['slots'])
        s['barrier'].wait(timeout=20)
        return out

    def allreduce_max(self, a):
        return self.allgather(np.asarray(a, dtype=np.float64)).max(axis=0)


def _unit(rows):
    """A fixed number in [-1, 1] per global row: the device's rounding, the same on any shard."""
    return ((rows * 2654435761) % 1000003) / 500001.5 - 1.0


class _SelBackend(OracleGridBackend):
    """A shard of ``problem``: ``var`` and ``S`` as functions of the rows, device keys off by up
    to the bound, and pairs that depend on the candidate and the row alone."""
    problem = None

    def __init__(self, gps, inputs_shard, global_offset):
        OracleGridBackend.__init__(self, gps, inputs_shard, global_offset)
        p = type(self).problem
        self.rows = self.lo + np.arange(self.x.shape[0])
        self.v = p['var'](self.x, self.rows)                                   # (G, n)
        self.S = p['S'](self.x, self.rows)
        self.comm, self.log = None, []

    def ise_noise(self):
        return np.asarray(type(self).problem['noise']) + 1e-8

    def _dev_keys(self, fmin):
        key = _np_keys(self.v, self.ise_noise(), np.isfinite(fmin))
        return key + ISE_KEY_EPS * np.maximum(1.0, key) * _unit(self.rows)

    def ise_keys(self, fmin):
        self.log.append('keys')
        k = self._dev_keys(fmin)[self.S]
        return (int(k.size), k.min(), k.max()) if k.size else (0, INF, -INF)

    def ise_hist(self, fmin, lo, hi):
        self.log.append('hist')
        return np.bincount(_bins(self._dev_keys(fmin)[self.S], lo, hi),
                           minlength=ISE_BINS).astype(np.uint32)

    def ise_list(self, fmin, thr, cap):
        self.log.append('list')
        k = self._dev_keys(fmin)
        at = np.flatnonzero(self.S & (k >= thr))
        m = at[:cap]
        return at.size, self.rows[m], k[m], self.x[m].copy(), self.v[:, m].T.copy()

    def ise_state(self):
        self.log.append('state')
        return self.v.copy(), self.S.copy(), self.ise_noise()

    def ise_safe(self, gidx):
        return self.S[np.asarray(gidx) - self.lo]

    def gather_rows(self, gidx):
        at = np.asarray(gidx, dtype=np.int64) - self.lo
        return self.x[at].copy(), None, self.v[:, at].T.copy(), None

    def ise_at(self, fmin, cand, xc, vx, about, comm=False):
        self.log.append('at')
        cand = np.asarray(cand, dtype=np.int64)
        pr = np.zeros((cand.size, self.x.shape[0]))
        near = np.exp(-((xc[:, None, :] - self.x[None, :, :]) ** 2).sum(-1))
        for g in np.flatnonzero(np.isfinite(fmin)):
            pr = pr + near * np.sqrt(vx[g][:, None] * self.v[g][None, :])
        pr = np.round(pr, 3)                                      # ties between rows and shards
        z = ~self.S if about == 0 else np.ones(self.S.size, dtype=bool)
        if z.any():
            al = np.where(z, pr, -INF).max(axis=1)
            tg = np.array([self.lo + np.flatnonzero(z & (pr[j] == al[j]))[0]
                           for j in range(cand.size)], dtype=np.int64)
        else:
            al, tg = np.full(cand.size, -INF), np.full(cand.size, -1, dtype=np.int64)
        if comm:                                                  # the library's in-stream form
            rec = self.comm.allgather(np.stack([al, tg.astype(np.float64)]))
            al, tg = dist.merge_ise_records(rec[:, 0], rec[:, 1].astype(np.int64))
        return (al, tg) + dist.pick_ise(al, tg, cand)

    def ise(self, fmin, cand, about, pairs=False):
        at = np.asarray(cand, dtype=np.int64) - self.lo
        return self.ise_at(fmin, cand, self.x[at], self.v[:, at], about) + (None,)


N_ROWS = 1200


def _problem(kind):
    def var(x, rows):
        base = 0.02 + (x[:, 0] + 2.0) ** 2 * (1.5 + np.sin(3.0 * x[:, 0]))
        if kind == 'flat':
            base = np.full(rows.size, 0.25)                      # one key: a degenerate range
        if kind == 'mass':
            base = np.where(rows % 11 == 0, np.minimum(base, 0.25), 0.25)   # equal keys on top
        return np.stack([base, 0.5 * base + 0.01])

    def S(x, rows):
        if kind == 'last':
            return rows >= N_ROWS - 90                           # the last shard only
        if kind == 'none':
            return np.zeros(rows.size, dtype=bool)
        if kind == 'every':
            return np.ones(rows.size, dtype=bool)
        if kind == 'mass':
            return x[:, 0] > -1.8                                # more safe rows than the cap
        return (rows % 3 != 1) & (np.abs(x[:, 0]) < 1.5)
    return dict(var=var, S=S, noise=(1e-4, 4e-4), N=6000 if kind == 'mass' else N_ROWS)


def _opt(comm):
    x = np.linspace(-1.0, 1.0, 5)[:, None]
    gps = [gpn.GPRegression(x, np.cos(x) + 1.0, gpn.RBF(1, 1.0, 0.5), noise_var=1e-4 * (g + 1))
           for g in range(2)]
    opt = safeopt_amd.SafeOpt(gps, np.linspace(-2.0, 2.0, _SelBackend.problem['N'])[:, None],
                              [0.0, 0.5], comm=comm)
    opt._backend.comm = comm
    return opt


def _call(opt, kw):
    try:
        out = opt.ise_point(return_values=True, **kw)
        return ('ok',) + tuple(np.asarray(a) for a in out), opt._ise_path
    except (RuntimeError, ValueError) as e:
        return (type(e).__name__, str(e)), opt._ise_path


def _ranks(world, in_stream, calls):
    shared = dict(slots=[None] * world, barrier=threading.Barrier(world))
    out = [None] * world

    def rank(r):
        try:
            opt = _opt(_ThreadComm(r, world, shared, in_stream))
            out[r] = [_call(opt, kw) for kw in calls] + [list(opt._backend.log)]
        except Exception as e:                       # noqa: BLE001 (handed to the test)
            out[r] = e
            shared['barrier'].abort()
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a rank is left waiting in a collective"
    for o in out:
        if isinstance(o, Exception):
            raise o
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, w) for u, w in zip(a, b))


@pytest.fixture
def backend():
    gp_opt._BACKEND_FACTORY = _SelBackend          # (tests/conftest.py resets the hook)
    yield _SelBackend
    _SelBackend.problem = None


SAFE = [r for r in range(N_ROWS) if r % 3 != 1 and abs(-2.0 + 4.0 * r / (N_ROWS - 1)) < 1.5]
CALLS = [dict(candidates=40), dict(candidates=7, about='all'), dict(candidates=4096),
         dict(candidates=np.array(SAFE[::97])), dict(candidates=np.array(SAFE[-5:])),
         dict(candidates=np.array([SAFE[0], 1, SAFE[9]]))]


@pytest.mark.parametrize("in_stream", [False, True], ids=["host-merge", "library-merge"])
@pytest.mark.parametrize("world", [2, 4])
def test_every_rank_returns_the_one_rank_result(backend, world, in_stream):
    backend.problem = _problem('plain')
    one = _opt(None)
    want = [_call(one, kw) for kw in CALLS[:3]]
    assert [w[1] for w in want] == ['device'] * 3 and 'state' not in one._backend.log
    want += [_call(one, kw) for kw in CALLS[3:]]
    assert want[0][0][0] == 'ok' and want[5][0][0] == 'ValueError'
    # (the device selection is the host's: rows of the first call against ise_candidates)
    var, S, s = one._backend.ise_state()
    assert_array_equal(want[0][0][3], ise_candidates(var, S, s, np.array([True, True]), 40))
    for r, got in enumerate(_ranks(world, in_stream, CALLS)):
        for kw, g, w in zip(CALLS, got, want):
            assert _same(g[0], w[0]), (r, kw)
        assert [g[1] for g in got[:3]] == ['device'] * 3
        assert 'state' not in got[-1]


@pytest.mark.parametrize("kind, path", [('flat', 'host: degenerate key range'),
                                        ('mass', 'host: list above the cap')])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_fallbacks_are_taken_and_agree(backend, kind, path, world):
    backend.problem = _problem(kind)
    calls = [dict(candidates=30), dict(candidates=30, about='all')]
    one = _opt(None)
    var, S, s = one._backend.ise_state()
    host = ise_candidates(var, S, s, np.array([True, True]), 30)
    assert kind != 'mass' or S.sum() > ise_list_cap(30)
    ranks = [[_call(one, kw) for kw in calls]] if world == 1 else _ranks(world, False, calls)
    first = [_call(_opt(None), kw) for kw in calls]
    for got in ranks:
        for g, w in zip(got, first):
            assert g[1] == path
            assert g[0][0] == 'ok' and _same(g[0], w[0])
            assert_array_equal(g[0][3], host)


@pytest.mark.parametrize("world", [2, 4])
def test_empty_shards_and_errors_on_every_rank(backend, world):
    calls = [dict(candidates=12), dict(candidates=12, about='all')]
    backend.problem = _problem('last')                # S in the last shard only
    want = [_call(_opt(None), kw) for kw in calls]
    assert want[0][0][0] == 'ok' and np.all(want[0][0][3] >= N_ROWS - 90)
    for in_stream in (False, True):
        for got in _ranks(world, in_stream, calls):
            assert all(_same(g[0], w[0]) for g, w in zip(got, want))
    backend.problem = _problem('none')
    for got in _ranks(world, False, calls[:1]):
        assert got[0][0][0] == 'RuntimeError' and 'no safe points' in got[0][0][1]
    backend.problem = _problem('every')
    for got in _ranks(world, False, calls[:1]):
        assert got[0][0][0] == 'RuntimeError' and 'no row qualifies' in got[0][0][1]


def test_a_communicator_without_collectives_is_refused_first(backend):
    backend.problem = _problem('plain')

    class Two(object):
        rank, world = 0, 2
    opt = _opt(Two())
    for call in (opt.ise_point, opt.info_point):
        with pytest.raises(NotImplementedError, match="one rank"):
            call()
    assert opt._backend.log == []
