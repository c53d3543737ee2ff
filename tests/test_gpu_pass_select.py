"""The candidate selection of the big passes on the device against a sorted walk in NumPy
(tests/_pass_ref.py): ``pass_hist`` bin by bin, ``pass_list`` row by row, ``lipschitz_pass`` walked
as ``SafeOpt._visit_in_big_passes`` walks it, ``SafeOpt`` end to end on one rank and on a pretended
world of 2, and ``expander_pass`` once on a case of tests/_expander_ref.py.

Everything here is integers and bit-exact comparisons of doubles: no tolerance.  The states are
uploaded intervals (``upload_Q``) whose safe rows are ``[0, w]``, so the key of a row is ``w`` bit
for bit; the candidate mask and the widths the reference works on are the device's own
(``download(CAND)`` / ``download(WIDTH)``), checked against what they must be.  The hit predicate is
the cdist formula of ``_oracle_backend.lipschitz_check`` with no comparison within 1e-9 of equality
(asserted on the reference, ``_pass_ref.lipschitz_hits``).

Sizes: 255 / 256 / 257 rows (one chunk of 256, its edges), 4097 (17 chunks, two workgroups' worth
of histogram), 262144 + 257 (more than 1024 chunks: the carry loop of ``k_pass_scan``), 2048 * 256 +
300 (more than 2048 chunks: the grid-stride loop of the count / list / histogram kernels), and a
shard at global offset 1000003 (cut index and mode-1 keys are global).
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _pass_ref as pr
from _gpu_common import _PretendWorldPadded

pytestmark = pytest.mark.gpu

INF, I64_MAX = np.inf, pr.I64_MAX
PASS_SIZES = [(16,), (64,), (8, 16), None]
RANGES = [(0.0, 1.1), (0.0, 0.7), (0.0, 0.3), (0.0, 1.7)]


@pytest.fixture(scope="module")
def mods(hip_device):
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip
    return safeopt_amd, gpy, _hip


class State(object):
    pass


def upload(_hip, pts, Q, fmin, goff=0, full=False):
    """Intervals on the device, maximisers, candidate mask: the state behind a selection."""
    st = State()
    st.pts, st.Q, st.goff = np.ascontiguousarray(pts), np.ascontiguousarray(Q), int(goff)
    st.fmin = np.atleast_1d(np.asarray(fmin, dtype=float))
    st.G = st.fmin.size
    st.grid = _hip.DeviceGrid(_hip.Context.default(), st.pts, st.G, st.goff)
    max_l, any_safe = st.grid.upload_Q(st.Q, st.fmin)
    st.S = np.all(st.Q[:, ::2] > st.fmin, axis=1)
    assert any_safe and max_l == st.Q[st.S, 0].max()
    assert_array_equal(st.grid.download(_hip.S), st.S)
    width = st.grid.maximizers(max_l)
    st.M = st.S & (st.Q[:, 1] >= max_l)
    assert width == (st.Q[st.M, 1] - st.Q[st.M, 0]).max()
    n_cand, n_unsafe = st.grid.candidates(width, np.ones(st.G), np.zeros(st.G), full)
    st.cand, st.w = st.grid.download(_hip.CAND), st.grid.download(_hip.WIDTH)
    wd = (st.Q[:, 1::2] - st.Q[:, ::2]).max(axis=1)
    assert_array_equal(st.cand, st.S if full else st.S & ~st.M & (wd > width))
    assert_array_equal(st.w[st.S], wd[st.S])                        # the key, bit for bit
    assert (n_cand, n_unsafe) == (int(st.cand.sum()), int((~st.S).sum()))
    return st


def line(N, d):
    """N rows with a power-of-two spacing: a line, or the first N rows of a square-ish grid."""
    if d == 1:
        return 2.0 ** -5, (np.arange(N) * 2.0 ** -5)[:, None]
    cols = int(np.ceil(np.sqrt(N)))
    ii, jj = np.divmod(np.arange(N), cols)
    return 2.0 ** -6, np.column_stack([ii * 2.0 ** -6, jj * 2.0 ** -6])


def key_pool(rng, size):
    """Widths for the selection kernels: random, two decimals, a tie run at 0.25 and the edge keys
    of both directions for the ranges of RANGES."""
    parts = [rng.uniform(1e-3, 1.2, size), np.round(rng.uniform(0.01, 1.2, size), 2),
             np.full(size // 4 + 8, 0.25)]
    for lo, hi in RANGES:
        for direction in ("counted", "listed"):
            ks = pr.edge_keys(lo, hi, direction)[1]
            if ks.size:
                parts.append(rng.choice(ks[ks > 2.0 ** -10], size // 2))
    return rng.choice(np.concatenate(parts), size)


@pytest.fixture(scope="module")
def key_states(mods):
    cache = {}

    def get(N, goff, G=1):
        if (N, goff, G) not in cache:
            _, _, _hip = mods
            rng = np.random.default_rng(N + 7 * G + goff % 1000)
            _h, pts = line(N, 1 if N < 4000 else 2)
            unsafe = np.arange(N) % 61 == 30
            Q = np.zeros((N, 2 * G))
            Q[:, 1] = key_pool(rng, N)
            Q[rng.choice(N, max(24, N // 16), replace=False), 1] = 0.25
            for i in range(1, G):                     # (narrower: GP 0 carries the key)
                Q[:, 2 * i + 1] = rng.uniform(0, 2.0 ** -11, N)
            Q[unsafe, ::2], Q[unsafe, 1::2] = -15.0, -14.0
            Q[0, :2] = [3.0, 3.0 + 2.0 ** -20]
            fmin = np.full(G, pr.FMIN)
            fmin[1:2] = -INF
            cache[(N, goff, G)] = st = upload(_hip, pts, Q, fmin, goff)
            assert st.cand.sum() == N - unsafe.sum() - 1 and (st.w[st.cand] == 0.25).sum() >= 8
        return cache[(N, goff, G)]
    return get


SHAPES = [(255, 0), (256, 0), (257, 0), (4097, 0), (4097, 1000003)]


def cuts_of(st, mode):
    """(cut_w, cut_idx, key_lo, key_hi): everything, inside a tie run, below everything."""
    N, goff = st.pts.shape[0], st.goff
    if mode == 1:
        lo, hi = -(float(goff + N) + 1.0), 1.0
        mid = -float(goff + N // 2)
        return [(INF, -1, lo, hi), (mid, -1, lo, hi), (mid, I64_MAX, lo, hi),
                (-float(goff + N + 5), -1, lo, hi), (-float(goff + 7), -1, lo, -float(goff))]
    ties = np.flatnonzero(st.cand & (st.w == 0.25)) + goff
    out = [(INF, I64_MAX, lo, hi) for lo, hi in RANGES]
    out += [(0.25, int(ties[ties.size // 2]), 0.0, 0.25), (0.25, int(ties[ties.size // 2]), 0.0, 1.1),
            (0.7, -1, 0.0, 0.7), (2.0 ** -11, -1, 0.0, 1.1)]
    return out


@pytest.mark.parametrize("N,goff", SHAPES)
def test_pass_hist_bin_by_bin(mods, key_states, N, goff):
    st = key_states(N, goff)
    for mode in (0, 1):
        sums = []
        for cut_w, cut_idx, lo, hi in cuts_of(st, mode):
            h = st.grid.pass_hist(mode, cut_w, cut_idx, lo, hi)
            rows, keys = pr.behind(st.cand, st.w, goff, mode, cut_w, cut_idx)
            assert int(h.sum()) == rows.size, (mode, cut_w, cut_idx)
            assert_array_equal(h, pr.hist(keys, lo, hi))
            sums.append(rows.size)
        assert sums[0] == st.cand.sum() and sums[-1 if mode == 0 else -2] == 0
        assert 0 < sums[-4 if mode == 0 else 1] < sums[0]             # (a cut inside)
    # the edge keys are there: bins whose count differs from the count of keys >= their edge
    rows, keys = pr.behind(st.cand, st.w, goff, 0, INF, I64_MAX)
    for (lo, hi), direction in (((0.0, 1.1), "counted"), ((0.0, 0.7), "listed")):
        if N >= 255:
            assert np.isin(keys, pr.edge_keys(lo, hi, direction)[1]).sum() >= 8


def thresholds_of(st, mode):
    N, goff = st.pts.shape[0], st.goff
    if mode == 1:
        return [-INF, -float(goff + N // 3), -float(goff + N // 3) + 0.5, -float(goff), 1.0]
    keys = st.w[st.cand]
    out = [-INF, 0.25, 2.0]
    for (lo, hi), direction in (((0.0, 1.1), "counted"), ((0.0, 0.7), "listed"), ((0.0, 0.3), "counted")):
        bs, ks = pr.edge_keys(lo, hi, direction)
        have = bs[np.isin(ks, keys)]
        assert have.size
        out += [float(pr.edge(b, lo, hi)) for b in have[[0, have.size // 2, -1]]]
    return out


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("N,goff", SHAPES)
def test_pass_list_row_by_row(mods, key_states, N, goff, G):
    st = key_states(N, goff, G)
    counts = []
    for mode in (0, 1):
        cuts = cuts_of(st, mode)
        for cut_w, cut_idx, _lo, _hi in (cuts[0], cuts[-4] if mode == 0 else cuts[2]):
            r0, k0 = pr.behind(st.cand, st.w, goff, mode, cut_w, cut_idx)
            for thr in thresholds_of(st, mode):
                rows, keys, x, resid = st.grid.pass_list(mode | 2, cut_w, cut_idx, thr, N)
                er, ek = pr.listed(r0, k0, thr)
                assert rows.size == er.size, (mode, cut_w, cut_idx, thr)
                assert_array_equal(rows, er)                       # ascending rows
                assert_array_equal(keys, ek)                       # widths / minus the row, bit for bit
                assert_array_equal(x, st.pts[er - goff])
                assert_array_equal(resid, st.Q[er - goff, 1::2])
                counts.append(er.size)
    assert 0 in counts and st.cand.sum() in counts


def test_pass_list_residual_after_a_confidence_pass(mods):
    """Without ``| 2`` the list carries ``u - mean``: compared once ``confidence`` has written
    ``mean`` (bit for bit: one subtraction of two resident doubles)."""
    _, gpy, _hip = mods
    rng = np.random.default_rng(3)
    _h, pts = line(4097, 2)
    X = rng.uniform(0, 1, (5, 2))
    gps = [gpy.models.GPRegression(X, np.sin(3 * X[:, :1]) + 0.1 * i, gpy.kern.RBF(2, variance=1.3, lengthscale=0.4),
                                   noise_var=0.01) for i in range(2)]
    devs = [g._fitted() for g in gps]
    grid = _hip.DeviceGrid(devs[0].ctx, pts, 2)
    fmin = np.array([-0.5, -INF])
    max_l, any_safe = grid.confidence(devs, 2.0, fmin)
    assert any_safe
    width = grid.maximizers(max_l)
    grid.candidates(width, np.ones(2), np.zeros(2), True)       # (every safe row)
    Q, mean = grid.download(_hip.Q), grid.download(_hip.MEAN)
    cand, w = grid.download(_hip.CAND), grid.download(_hip.WIDTH)
    assert_array_equal(cand, grid.download(_hip.S))
    assert 100 < cand.sum() < 4097 and np.any(mean != 0.0)
    thr = float(np.median(w[cand]))
    r0, k0 = pr.behind(cand, w, 0, 0, INF, I64_MAX)
    er, ek = pr.listed(r0, k0, thr)
    for flag, want in ((0, Q[er, 1::2] - mean[:, er].T), (2, Q[er, 1::2])):
        rows, keys, x, resid = grid.pass_list(flag, INF, I64_MAX, thr, 4097)
        assert_array_equal(rows, er)
        assert_array_equal(keys, ek)
        assert_array_equal(x, pts[er])
        assert_array_equal(resid, want)


@pytest.mark.parametrize("N", [262144 + 257, 2048 * 256 + 300])
def test_scan_carry_and_grid_stride(mods, N):
    """More than 1024 chunks (the carry of ``k_pass_scan``) and more than 2048 (the stride of
    the histogram / count / list kernels), with known contents: chunks without a candidate,
    dense chunks, candidates in the last rows; one ``lipschitz_pass`` whose first hit is there."""
    _, _, _hip = mods
    rng = np.random.default_rng(N)
    h, pts = line(N, 1)
    unsafe = np.arange(N) % 1009 == 500
    unsafe[[N - 150, 262144 + 100]] = True
    w = np.where(rng.random(N) < 0.3, rng.uniform(0.01, 1.05, N), 0.0)
    w[3000:9000] = 0.0                                         # chunks without a candidate
    w[N - 300:] = rng.uniform(0.01, 1.05, 300)                 # the ragged tail, dense
    w[[N - 151, N - 149]] = [1.0875, 1.09375]                  # touch an unsafe row, near the top
    w[[262144 + 99, 262144 + 101]] = [1.0625, 1.078125]
    nb = np.flatnonzero(np.arange(N) % 1009 == 500)
    w[nb - 1], w[nb + 1] = 0.0, 0.0                            # (the only hits are those four)
    Q = np.zeros((N, 2))
    Q[:, 1] = w
    Q[unsafe] = [-15.0, -14.0]
    Q[0] = [3.0, 3.0 + 2.0 ** -20]
    st = upload(_hip, pts, Q, pr.FMIN)
    assert 0.2 * N < st.cand.sum() < 0.4 * N
    lo, hi = 0.0, 1.1
    r0, k0 = pr.behind(st.cand, st.w, 0, 0, hi, I64_MAX)
    assert r0.size == st.cand.sum()
    hh = st.grid.pass_hist(0, hi, I64_MAX, lo, hi)
    assert_array_equal(hh, pr.hist(k0, lo, hi))
    for thr in (float(pr.edge(3800, lo, hi)), -INF):
        rows, keys, x, resid = st.grid.pass_list(2, hi, I64_MAX, thr, N)
        er, ek = pr.listed(r0, k0, thr)
        assert_array_equal(rows, er)
        assert_array_equal(keys, ek)
        assert_array_equal(x[:, 0], pts[er, 0])
        assert_array_equal(resid[:, 0], Q[er, 1])
        assert er.max() >= N - 300 and (er < 262144).any()
    L = -pr.FMIN / (1.75 * h)
    want = 1000
    b, thr, est = pr.pick(hh, want, lo, hi)
    er, ek = pr.listed(r0, k0, thr)
    hits = pr.lipschitz_hits(pts, st.S, er, ek, pr.FMIN, L)
    assert want <= er.size == est <= want + 200 and hits.sum() == 4
    t, nh, key, row, left, _amax = st.grid.lipschitz_pass([pr.FMIN], [L], 0, hi, I64_MAX, lo, hi, want)
    assert (t, nh, left) == (er.size, 4, thr)
    assert (key, row) == pr.first_hit(er, ek, hits) == (1.09375, N - 149)
    assert not st.grid.download(_hip.G).any()


# ---- lipschitz_pass walked as the driver walks it ------------------------------------------
def three_gps(sc, seed=0):
    """The scenario with two more GPs: one without a constraint (wide intervals that do not
    count), one whose reach is 1.25 .. 1.39 spacings (the 4-neighbourhood in 2-D)."""
    pts, Q0 = sc.shard()
    rng = np.random.default_rng(seed)
    n = sc.n
    Q = np.zeros((n, 6))
    Q[:, :2] = Q0
    Q[:, 3] = rng.uniform(0.0, 1.0, n) * Q0[:, 1]              # (never the widest: the key stays GP 0's)
    Q[:, 5] = rng.uniform(0.5, 1.0, n) * Q0[:, 1]
    unsafe = Q0[:, 0] <= sc.fmin
    Q[unsafe, ::2], Q[unsafe, 1::2] = -15.0, -14.0
    Q[0, 2:] = [0.0, 2.0 ** -21, 0.0, 2.0 ** -21]
    h = 2.0 ** -5 if sc.dim == 1 else 2.0 ** -6
    return pts, Q, np.array([sc.fmin, -INF, sc.fmin]), np.array([sc.lipschitz, 1.0, -sc.fmin / (1.25 * h)])


def walk(st, hit, fmin, L, mode, cut_w, cut_idx, lo, hi, want):
    """The loop of ``_visit_in_big_passes`` over ``lipschitz_pass``, every pass against the
    reference: what it tested, how many hits, the first one, the key it leaves.  Returns the sum
    of ``tested``, the first reported ``(key, row)``, the tested counts."""
    total, first, tested = 0, None, []
    while True:
        t, nh, key, row, left, _amax = st.grid.lipschitz_pass(fmin, L, mode, cut_w, cut_idx, lo, hi, want)
        r, k = pr.behind(st.cand, st.w, st.goff, mode, cut_w, cut_idx)
        _b, thr, _est = pr.pick(pr.hist(k, lo, hi), want, lo, hi)
        lr, lk = pr.listed(r, k, thr)
        lh = hit[lr - st.goff]
        assert (t, nh) == (lr.size, int(lh.sum())), (len(tested), cut_w, cut_idx, thr)
        assert left == thr, (len(tested), t, left, thr)
        if mode == 0 and nh:
            assert (key, row) == pr.first_hit(lr, lk, lh)
            first = first or (key, row)
        assert t or not tested or tested[-1], "two consecutive passes tested nothing"
        tested.append(t)
        total += t
        if left == -INF:
            return total, first, tested
        cut_w, cut_idx = left, -1
        if mode == 0 or t == 0:
            hi = left


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("name", pr.SCENARIOS)
def test_lipschitz_pass_walk(mods, name, G):
    _, _, _hip = mods
    sc = pr.scenario(name, 2 if name in "aceg" else 1, lead=17, want=64)
    if G == 1:
        (pts, Q), fmin, L = sc.shard(), np.array([sc.fmin]), np.array([sc.lipschitz])
    else:
        pts, Q, fmin, L = three_gps(sc)
    n = sc.n
    for mode in (0, 1):
        st = upload(_hip, pts, Q, fmin, full=mode == 1)
        hit = np.zeros(n, dtype=bool)
        c = np.flatnonzero(st.cand)
        hit[c] = pr.lipschitz_hits(pts, st.S, c, st.Q[c, 1::2], fmin, L)
        assert hit.any() and not hit[c].all()
        for want in (1, 16, 64, 1000):
            if mode == 1:
                st.grid.upload_mask(_hip.G, np.zeros(n, dtype=bool))
                total, first, tested = walk(st, hit, fmin, L, 1, INF, -1, -(float(n) + 1.0), 1.0, want)
                assert total == st.cand.sum()
                assert_array_equal(st.grid.download(_hip.G), hit)        # row for row
                continue
            # (from the cut at which the driver begins; once from the top as well)
            for cut_w, cut_idx in (sc.cut, (float(st.w[st.cand].max()), I64_MAX))[:2 if want == 64 else 1]:
                r0, k0 = pr.behind(st.cand, st.w, 0, 0, cut_w, cut_idx)
                total, first, tested = walk(st, hit, fmin, L, 0, cut_w, cut_idx, 0.0, cut_w, want)
                assert total == r0.size
                vr, vk = pr.visiting_order(r0, k0)
                assert hit[vr].any()
                pos = int(np.argmax(hit[vr]))                            # largest key, then largest row
                assert first == (float(vk[pos]), int(vr[pos]))
                if G == 1 and (cut_w, cut_idx) == sc.cut:
                    assert first == sc.first
                    if name in "cf" and want in (16, 64):
                        print("scenario (%s) lipschitz_pass want %d: tested per pass %s" % (name, want, tested))
                    if name == "d" and want <= 64:
                        assert tested[0] == 0 and tested[1] >= 4 * want   # counted, then listed
            assert not st.grid.download(_hip.G).any()                    # mode 0 marks nothing


# ---- SafeOpt end to end -------------------------------------------------------------------
def _one_rank_comm(_hip, dist):
    ctx = _hip.Context.default()
    if not getattr(ctx, "_one_rank_comm", False):
        ctx.comm_init(_hip.Context.comm_unique_id(), 0, 1)
        ctx._one_rank_comm = True
    return _PretendWorldPadded(dist.RcclComm(ctx), 2)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("name", pr.SCENARIOS)
def test_safeopt_end_to_end(mods, name, world):
    safeopt_amd, gpy, _hip = mods
    from safeopt_amd import dist
    for dim in (1, 2):
        for sizes in PASS_SIZES:
            sc = pr.scenario(name, dim, lead=17 if world == 2 else 1, want=64 if sizes is None else sizes[0])
            S, M, G, q = pr.reference_sets(sc)
            gp = gpy.models.GPRegression(np.zeros((1, dim)), np.ones((1, 1)), gpy.kern.RBF(dim),
                                         noise_var=0.01)
            if world == 2:
                opt = safeopt_amd.SafeOpt(gp, sc.points, sc.fmin, lipschitz=sc.lipschitz,
                                          threshold=sc.threshold, comm=_one_rank_comm(_hip, dist))
                opt.Q = sc.Q
            else:
                opt = safeopt_amd.SafeOpt(gp, sc.points[:sc.n], sc.fmin, lipschitz=sc.lipschitz,
                                          threshold=sc.threshold)
                opt.Q = sc.Q[:sc.n]
            assert np.all(opt.scaling == 1.0)
            if sizes is not None:
                opt.pass_sizes = sizes
            be, tested = opt._backend, []
            if world == 2:
                assert opt._shard == (0, sc.n)
                inner = be.pass_list
                be.pass_list = lambda *a: (lambda out: tested.append(int(out[0].size)) or out)(inner(*a))
            else:
                inner = be.lipschitz_pass
                be.lipschitz_pass = lambda *a: (lambda out: tested.append(out[0]) or out)(inner(*a))
            opt.compute_sets()
            assert tested, "the loop never reached a big pass"
            for what, ref in ((_hip.S, S), (_hip.M, M)):
                assert_array_equal(be.download(what)[:sc.n], ref)
            assert_array_equal(np.flatnonzero(be.download(_hip.G)[:sc.n]), np.flatnonzero(G))
            assert_array_equal(opt.get_new_query_point(), sc.points[q])
            if name in "cf":
                print("scenario (%s) %d-D, %d rank(s), pass_sizes %s: tested per pass %s" % (
                    name, dim, world, sizes, tested))


# ---- the GP form: the same selection, margins of tests/_expander_ref.py ---------------------
def _expander_case(name):
    from test_gpu_expander_flags import _device
    return _device(name)


def test_expander_pass_reports_the_first_expander(mods):
    """``m32_d2_n16_grid``, every safe row a candidate, mode 0, 16 per pass, walked from the top
    of the visiting order and from cuts further down: the first expander reported over a walk is
    the widest row (then the largest) behind the cut whose reference margin is a decided hit -- or
    a row inside the band ahead of it, which may go either way."""
    import _expander_ref as er
    _, _, _hip = mods
    dv = _expander_case("m32_d2_n16_grid")
    c, grid = dv.c, dv.grid
    grid.candidates(0.0, np.ones(c.G), np.zeros(c.G), True)
    cand, w = grid.download(_hip.CAND), grid.download(_hip.WIDTH)
    assert_array_equal(np.flatnonzero(cand), c.safe_rows)
    dec, hit = er.decided(c, dv.best_safe)
    act = c.active[None, :]
    sure1 = np.all(hit | ~act, axis=1)                 # (per safe row)
    band = np.any(~dec & act, axis=1) & ~np.any(dec & ~hit, axis=1)
    r0, k0 = pr.behind(cand, w, 0, 0, INF, I64_MAX)
    vr, vk = pr.visiting_order(r0, k0)
    starts = [0] + [j for j in (100, 300, 500, 690, 800) if j < vr.size]
    for j in starts:
        # strictly behind candidate j - 1 of the visiting order
        cut_w, cut_idx = (float(vk[0]), I64_MAX) if j == 0 else (float(vk[j - 1]), int(vr[j - 1]))
        at = np.searchsorted(c.safe_rows, vr[j:])
        assert sure1[at].any()
        pos = int(np.argmax(sure1[at]))
        allowed = [int(vr[j + pos])] + [int(r) for r in vr[j:j + pos][band[at[:pos]]]]
        hi, total, passes = cut_w, 0, 0
        while True:
            t, nh, key, row, left, _amax = grid.expander_pass(dv.devs, er.BETA, c.fmin, 0, cut_w,
                                                              cut_idx, 0.0, hi, 16)
            r, k = pr.behind(cand, w, 0, 0, cut_w, cut_idx)
            _b, thr, _est = pr.pick(pr.hist(k, 0.0, hi), 16, 0.0, hi)
            assert (t, left) == (pr.listed(r, k, thr)[0].size, thr)
            total, passes = total + t, passes + 1
            assert passes < 100
            if nh or left == -INF:
                break
            cut_w, cut_idx, hi = left, -1, left
        assert nh and row in allowed and key == w[row], (j, key, row, allowed)
        assert total >= pos + 1
        assert not grid.download(_hip.G).any()
        print("expander_pass from candidate %d: first expander row %d (width %.17g) after %d "
              "candidates in %d passes; %d rows allowed" % (j, row, key, total, passes, len(allowed)))


def test_no_constraint_at_all(mods):
    """Every ``fmin = -inf``: the reference's loop over the GPs only continues and ``G`` stays
    false -- ``lipschitz_pass`` and ``expander_pass``, called directly, report 0 hits and mark
    nothing, in both modes; so does ``pass_lipschitz_test``."""
    import _expander_ref as er
    _, _, _hip = mods
    sc = pr.scenario("a", 2, lead=17, want=64)
    pts, Q = sc.shard()
    st = upload(_hip, pts, Q, sc.fmin)
    n, none = sc.n, np.array([-INF])
    assert (~st.S).any()
    for mode, cut, lo, hi in ((0, (1.0, I64_MAX), 0.0, 1.0), (1, (INF, -1), -(float(n) + 1.0), 1.0)):
        t, nh, key, row, left, amax = st.grid.lipschitz_pass(none, [sc.lipschitz], mode, cut[0], cut[1],
                                                            lo, hi, 4096)
        assert t == st.cand.sum() and nh == 0 and left == -INF
        assert not st.grid.download(_hip.G).any()
    c = np.flatnonzero(st.cand)[:100]
    assert not st.grid.pass_lipschitz_test(none, [sc.lipschitz], pts[c], Q[c, 1:]).any()
    # ... with the constraint the same calls do find hits (the case is not void)
    t, nh, key, row, left, amax = st.grid.lipschitz_pass([sc.fmin], [sc.lipschitz], 1, INF, -1,
                                                        -(float(n) + 1.0), 1.0, 4096)
    assert nh == 32 and st.grid.download(_hip.G).sum() == 32
    dv = _expander_case("m32_d2_n16_grid")
    cc, grid = dv.c, dv.grid
    grid.candidates(0.0, np.ones(cc.G), np.zeros(cc.G), True)
    N = cc.pts.shape[0]
    none = np.full(cc.G, -INF)
    wmax = float(grid.download(_hip.WIDTH)[cc.S].max())
    for mode, cut, lo, hi in ((0, (wmax, I64_MAX), 0.0, wmax), (1, (INF, -1), -(float(N) + 1.0), 1.0)):
        t, nh, key, row, left, amax = grid.expander_pass(dv.devs, er.BETA, none, mode, cut[0], cut[1],
                                                        lo, hi, 4096)
        assert t == cc.safe_rows.size and nh == 0 and left == -INF
        assert not grid.download(_hip.G).any()
