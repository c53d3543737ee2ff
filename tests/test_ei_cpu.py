"""Log expected improvement without a GPU: the yardstick (tests/_ei_ref.py: the float64
restatement of csrc/ei_term.h against the definitions in 50-digit mpmath), the under-flow case
the logarithm exists for, the declarations, and the host logic of ``SafeOpt.ei_point`` through a
NumPy stand-in (tests/_ei_backend.py) on one rank and on two ranks over gloo."""
import os
import re
import sys

import numpy as np
import pytest
from numpy.testing import assert_array_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import _ei_ref as ref                                                      # noqa: E402
from test_dist_gloo import TorchComm, _free_port, _needs_torch             # noqa: E402


# ---- 1. the restatement against mpmath ---------------------------------------------------------

def test_restatement_is_finite_monotone_and_measured():
    """The yardstick of tests/test_gpu_ei.py: measured and printed, not bounded here."""
    z, _eh, _en, uh, un = ref.reference()
    assert z.size == 3201 + 2000 + 400 + 100 + 4
    h, n = ref.log_h(z), ref.log_ndtr(z)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(n))
    print("restatement over %d points: max error in units of EPS (1 + z^2 / 2): log_h %.3f at "
          "z = %r, log_ndtr %.3f at z = %r"
          % (z.size, uh.max(), z[np.argmax(uh)], un.max(), z[np.argmax(un)]))
    assert np.isfinite(uh.max()) and np.isfinite(un.max())
    order = np.argsort(z, kind="stable")
    assert np.all(np.diff(h[order]) >= 0.0)
    assert np.all(np.diff(h[order])[np.diff(z[order]) > 0.0] > 0.0)
    assert np.all(np.diff(n[order]) >= 0.0) and np.all(n <= 0.0)
    # h(z) -> z:  ln h(z) - ln z -> 0
    big = z[z >= 10.0]
    gap = np.abs(ref.log_h(big) - np.log(big))
    assert gap[np.argmax(big)] == 0.0 and np.all(gap <= 4 * ref.EPS * np.maximum(1.0, np.log(big)))
    assert ref.log_h(np.inf) == np.inf and ref.log_ndtr(np.inf) == 0.0


def test_branches_meet_at_the_branch_points():
    """Each form evaluated on both sides of its branch point: the neighbouring doubles differ
    by no more than the unit allows."""
    for zb in (ref.Z_DIRECT, ref.Z_ASYMPT):
        lo, hi = np.nextafter(zb, -np.inf), zb
        a, b = ref.log_h(lo), ref.log_h(hi)
        assert b >= a and b - a <= 8 * ref.EPS * (1.0 + 0.5 * zb * zb) + 2 * abs(zb) * (hi - lo)


def test_the_logarithm_orders_rows_whose_ei_underflows():
    """A converged run in small: sigma = 1e-3, the incumbent 1000 sigma and more above every
    row.  EI is exactly 0 on all of them -- its arg-max would be 'the lowest row among equals'
    by accident -- and alpha is finite, strictly decreasing, largest on row 0."""
    mean = -np.linspace(0.0, 1.0, 64)
    var = np.full(64, 1e-6)
    for kind in (ref.EI, ref.PI):
        a = ref.alpha(mean, var, 1.0, kind=kind)
        assert np.all(np.isfinite(a))
        assert np.all(np.exp(a) == 0.0)
        assert int(np.argmax(a)) == 0 and np.all(np.diff(a) < 0.0)
    # the naive form on the same rows: all zeros
    from scipy.special import ndtr
    z = (mean - 1.0) / 1e-3
    naive = 1e-3 * (np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) + z * ndtr(z))
    assert np.all(naive == 0.0)


def test_converged_problem_has_one_pick_and_no_ei():
    """The case tests/test_gpu_ei.py builds as a real optimiser (tests/_ei_problems.py), on the
    oracle's posterior: EI is 0 on every safe row, and the two largest alpha over S differ by
    far more than the tolerance of a term at those rows -- the device's arg-max is decided."""
    import _ei_problems as EP
    mean, var, S = EP.host_state()
    assert S.sum() > 500 and np.sqrt(var).max() < 5e-3
    tau = mean[S].max()
    a = ref.alpha(mean, var, tau, EP.XI)
    assert np.all(np.isfinite(a)) and np.exp(a[S]).max() == 0.0
    z = (mean - tau - EP.XI) / np.sqrt(var)
    tol = 4.0 * ref.reference()[3].max() * ref.EPS * (1.0 + 0.5 * z * z)
    gap = EP.top_two_gap(a, S)
    print("converged problem: |S| = %d, alpha in [%.4g, %.4g], top-two gap %.4g, tolerance %.3g"
          % (S.sum(), a[S].min(), a[S].max(), gap, tol.max()))
    assert gap > 1e6 * tol.max()


def test_alpha_is_ln_ei_where_ei_is_representable():
    rng = np.random.default_rng(5)
    mean, var = rng.normal(size=500), np.exp(rng.uniform(np.log(1e-4), np.log(4.0), 500))
    from scipy.special import ndtr
    s = np.sqrt(var)
    z = (mean - 0.3 - 0.01) / s
    keep = z > -6.0
    ei = s * (np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) + z * ndtr(z))
    a = ref.alpha(mean, var, 0.3, xi=0.01)
    assert keep.sum() > 300 and np.max(np.abs(a[keep] - np.log(ei[keep]))) < 1e-9
    # the weights: one finite fmin adds ln Phi of that GP, -inf adds nothing
    m2, v2 = np.vstack([mean, mean[::-1]]), np.vstack([var, var[::-1]])
    assert_array_equal(ref.alpha(m2, v2, 0.3, fmin=[-np.inf, -np.inf]), ref.alpha(mean, var, 0.3))
    w = ref.alpha(m2, v2, 0.3, fmin=[-np.inf, 0.1])
    assert_array_equal(w, ref.alpha(mean, var, 0.3) + ref.log_ndtr((m2[1] - 0.1) / np.sqrt(v2[1])))


# ---- 2. the declarations -----------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "safeopt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("sgp_ei_eval", "sgp_grid_ei", "sgp_grid_ei_comm"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    for name, val in (("SGP_EI_EI", 0), ("SGP_EI_PI", 1), ("SGP_EI_TAU_MEAN", 1),
                      ("SGP_EI_TAU_VALUE", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), code), name
    from safeopt_amd import _hip
    assert (_hip.EI_EI, _hip.EI_PI, _hip.EI_TAU_MEAN, _hip.EI_TAU_VALUE) == (0, 1, 1, 2)
    for name in ("sgp_ei_eval", "sgp_grid_ei", "sgp_grid_ei_comm"):
        assert name in _hip.PROTOTYPES
    assert callable(_hip.Context.ei_eval) and callable(_hip.DeviceGrid.ei)


def test_ei_source_is_built_without_contraction():
    from safeopt_amd import build
    assert "ei.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA["ei.hip"]
    assert any(h.endswith("ei_term.h") for h in build.HEADERS)
    src = open(os.path.join(build.CSRC, "ei_term.h")).read()
    for name, val in (("SGP_EI_Z_DIRECT", ref.Z_DIRECT), ("SGP_EI_Z_ASYMPT", ref.Z_ASYMPT)):
        m = re.search(r"#define\s+%s\s+\((-[0-9.e]+)\)" % name, src)
        assert m and float(m.group(1)) == val, name


# ---- 3. the host logic of ei_point -------------------------------------------------------------

def _problem():
    """Data on the left of the grid only: the safe set ends before the middle, so the second
    of two shards (31 | 30 rows) has no safe row."""
    x = np.linspace(-1.7, -0.7, 5)[:, None]
    y = [np.cos(x + 1.2) + 1.0 + 0.1 * g for g in range(2)]
    return x, y, np.linspace(-2.0, 2.0, 61)[:, None]


def _opt(comm=None, fmin=(0.0, 0.5)):
    import safeopt_amd
    from oracle import gp_numpy as gpn
    from _ei_backend import use_ei_backend
    use_ei_backend()
    x, y, grid = _problem()
    gps = [gpn.GPRegression(x, y[g], gpn.RBF(1, 1.0, 0.5 + 0.1 * g), noise_var=1e-4 * (g + 1))
           for g in range(2)]
    kw = {} if comm is None else dict(comm=comm)
    opt = safeopt_amd.SafeOpt(gps, grid, list(fmin), **kw)
    opt.optimize()
    return opt


CASES = [dict(), dict(kind='pi'), dict(incumbent='data'), dict(incumbent=1.25, xi=0.05),
         dict(within='MG'), dict(within='all'), dict(within='all', feasibility=True),
         dict(feasibility=True, kind='pi')]


def _want(opt, kw):
    """The pick from the stand-in's own posterior (one rank)."""
    be = opt._backend
    be._posterior()
    N = be.x.shape[0]
    within = kw.get('within', 'safe')
    inc = kw.get('incumbent', 'mean')
    over = np.ones(N, dtype=bool) if within == 'all' else be.S
    tau = be.mean[over, 0].max() if inc == 'mean' else opt.y[:, 0].max() if inc == 'data' else inc
    al = ref.alpha(be.mean.T, be.var.T, tau, kw.get('xi', 0.0),
                   ref.PI if kw.get('kind') == 'pi' else ref.EI,
                   np.asarray(opt.fmin, dtype=float) if kw.get('feasibility') else None)
    mask = {'safe': be.S, 'MG': be.M | be.G, 'all': np.ones(N, dtype=bool)}[within]
    j = int(np.flatnonzero(mask)[np.argmax(al[mask])])
    return j, al, tau


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items())
                         or "default")
def test_ei_point_picks_masks_and_strips(kw):
    opt = _opt()
    S = opt._backend.S
    assert 3 < S.sum() < S.size and not S[31:].any() and (opt._backend.M | opt._backend.G).any()
    j, al, tau = _want(opt, kw)
    x, a, values, tau_used = opt.ei_point(return_values=True, **kw)
    assert_array_equal(values, al)
    assert tau_used == tau and a == al[j] and x.shape == (1,)
    assert_array_equal(x, opt.inputs[j])
    if kw.get('within', 'safe') != 'all':
        assert S[j]
    x2, a2 = opt.ei_point(**kw)
    assert_array_equal(x2, x)
    assert a2 == a


def test_the_unconstrained_pick_differs_from_the_safe_one():
    opt = _opt()
    assert not np.array_equal(opt.ei_point()[0], opt.ei_point(within='all')[0])


@pytest.mark.parametrize("kw", [dict(within='unsafe'), dict(kind='ucb'), dict(xi=-1.0),
                                dict(xi=np.nan), dict(incumbent='best'),
                                dict(incumbent=np.inf), dict(incumbent=np.nan)])
def test_ei_point_refuses_bad_arguments(kw):
    opt = _opt()
    with pytest.raises(ValueError):
        opt.ei_point(**kw)
    assert opt._backend.calls == []


def test_ei_point_errors_and_state():
    opt = _opt()
    be = opt._backend
    before = [a.copy() for a in (be.Q, be.S, be.M, be.G, opt.x, opt.y)]
    rs = np.random.get_state()
    opt.ei_point()
    opt.ei_point(within='MG', feasibility=True, return_values=True)
    for u, w in zip(before, (be.Q, be.S, be.M, be.G, opt.x, opt.y)):
        assert_array_equal(u, w)
    now = np.random.get_state()
    assert rs[0] == now[0] and np.array_equal(rs[1], now[1]) and rs[2:] == now[2:]
    opt.S[:] = False
    with pytest.raises(RuntimeError, match="no safe points"):
        opt.ei_point()
    # every row: there is an incumbent and a pick whatever S holds
    assert np.isfinite(opt.ei_point(within='all')[1])


def test_backend_without_ei_is_refused():
    import safeopt_amd
    from oracle import gp_numpy as gpn
    from _oracle_backend import OracleGridBackend, use_oracle_backend
    assert not hasattr(OracleGridBackend, 'ei')
    use_oracle_backend()
    x = np.linspace(-1.0, 1.0, 5)[:, None]
    gp = gpn.GPRegression(x, np.cos(x) + 1.0, gpn.RBF(1, 1.0, 0.5), noise_var=1e-4)
    opt = safeopt_amd.SafeOpt(gp, np.linspace(-2.0, 2.0, 50)[:, None], 0.0)
    with pytest.raises(NotImplementedError):
        opt.ei_point()


def test_communicator_without_the_collectives_is_refused():
    opt = _opt()

    class Two(object):
        rank, world = 0, 2
    opt._comm = Two()
    with pytest.raises(NotImplementedError, match="allreduce_max and allgather"):
        opt.ei_point()
    assert opt._backend.calls == []


# ---- 4. world 2 over gloo ----------------------------------------------------------------------

def _worker(rank, world, port, q):
    try:
        sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
        import torch.distributed as td
        td.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                              rank=rank, world_size=world)
        from safeopt_amd.dist import LocalComm
        comm = TorchComm()
        opt, one = _opt(comm), _opt(LocalComm())
        lo, hi = opt._shard
        out = {"sharded": hi - lo < one.inputs.shape[0],
               "safe_here": bool(opt._backend.S.any()), "cases": []}
        for kw in CASES:
            a = opt.ei_point(return_values=True, **kw)
            b = one.ei_point(return_values=True, **kw)
            out["cases"].append([np.array_equal(u, w) for u, w in zip(a, b)])
        out["picks"] = [opt.ei_point(**kw) for kw in CASES]
        # ---- nothing is safe: raised behind the collective, on both ranks
        opt.S[:] = False
        try:
            opt.ei_point()
            out["unsafe"] = "no error"
        except RuntimeError as e:
            out["unsafe"] = "RuntimeError" if "no safe points" in str(e) else str(e)
        comm.barrier()
        try:
            opt.ei_point(incumbent=1.0, return_values=True)
            out["unsafe_value"] = "no error"
        except RuntimeError as e:
            out["unsafe_value"] = "RuntimeError" if "no safe points" in str(e) else str(e)
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
        assert out["sharded"]
        for kw, same in zip(CASES, out["cases"]):
            assert same == [True, True, True, True], (rank, kw, same)  # x, alpha, values, tau
    a, b = two_ranks
    assert a["safe_here"] and not b["safe_here"]          # a shard without a safe row
    for (xa, va), (xb, vb) in zip(a["picks"], b["picks"]):
        assert_array_equal(xa, xb)
        assert va == vb


@pytest.mark.timeout(300)
def test_all_unsafe_raises_on_both_ranks(two_ranks):
    assert [out["unsafe"] for out in two_ranks] == ["RuntimeError", "RuntimeError"]
    assert [out["unsafe_value"] for out in two_ranks] == ["RuntimeError", "RuntimeError"]
