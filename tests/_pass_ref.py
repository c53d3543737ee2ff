"""Reference for the candidate selection of the big passes (csrc/sets.hip: k_pass_hist, k_pass_pick,
k_pass_count / scan / list; gp_opt.py: _visit_in_big_passes): NumPy only, integers and bit-exact
comparisons of doubles, no tolerance.

TEST INFRASTRUCTURE.  A big pass selects the candidates strictly behind a cut ``(cut_w, cut_idx)``
in visiting order -- key descending, then row descending; the key is the width, or minus the global
row in mode 1 -- whose key is at least a threshold picked from a 4096-bin histogram.  What is
restated here: ``behind`` (pass_key), ``bin_of`` / ``edge`` (the two sides of the histogram that
can disagree by an ulp: the histogram multiplies, the list compares with an edge), ``pick``
(k_pass_pick), ``first_hit`` (k_pass_result) and the Lipschitz predicate.

Scenarios ``(a)`` .. ``(g)`` are states whose hit set does not depend on the widths: safe rows are
``[0, w]``, unsafe rows ``[-15, -14]``, ``fmin = -10`` and the Lipschitz constant puts the reach
``(u - fmin) / L`` of every ``u`` in ``[0, 1.1]`` between 1.75 and 1.95 grid spacings (the spacing is
a power of two, so distances are exact): a candidate is an expander exactly when it touches an
unsafe row (8-neighbourhood in 2-D), with margins of order one.  The widths are then assigned by
hand, and every builder asserts its own premise.
"""
import numpy as np

NBINS = 4096
I64_MAX = np.iinfo(np.int64).max
FMIN = -10.0
W_MAX = 1.1


# ---- the selection --------------------------------------------------------------------
def behind(cand, w, goff, mode, cut_w, cut_idx):
    """Global rows and keys of the candidates strictly behind the cut (row order)."""
    idx = np.flatnonzero(np.asarray(cand, dtype=bool)).astype(np.int64) + int(goff)
    key = -idx.astype(np.float64) if (mode & 1) else np.asarray(w, dtype=np.float64)[idx - int(goff)]
    keep = (key < cut_w) | ((key == cut_w) & (idx < cut_idx))
    return idx[keep], key[keep]


def visiting_order(rows, keys):
    """Key descending, then row descending."""
    order = np.lexsort((rows, keys))[::-1]
    return rows[order], keys[order]


def bin_of(key, lo, hi):
    """The bin k_pass_hist counts a key in: ``int((key - lo) * (4096 / (hi - lo)))``, clamped."""
    b = ((np.asarray(key, dtype=np.float64) - lo) * (float(NBINS) / (hi - lo)))
    return np.clip(b, -1.0, float(NBINS)).astype(np.int64).clip(0, NBINS - 1)


def edge(b, lo, hi):
    """The lower edge of bin b as k_pass_pick computes the threshold."""
    return lo + (hi - lo) * (np.asarray(b, dtype=np.float64) / float(NBINS))


def hist(keys, lo, hi):
    return np.bincount(bin_of(keys, lo, hi), minlength=NBINS).astype(np.uint32)


def pick(h, want, lo, hi):
    """k_pass_pick: ``(bin, threshold, promised count)``; the highest bin at which the count from
    the top reaches ``want`` (bin 0 / -inf: everything left)."""
    from_top = np.cumsum(np.asarray(h, dtype=np.int64)[::-1])
    if from_top[-1] < want:
        return 0, -np.inf, int(from_top[-1])
    k = int(np.argmax(from_top >= want))
    b = NBINS - 1 - k
    return b, (-np.inf if b == 0 else float(edge(b, lo, hi))), int(from_top[k])


def listed(rows, keys, thr):
    """What a pass lists of ``behind(...)``: key >= thr, ascending rows."""
    keep = keys >= thr
    order = np.argsort(rows[keep], kind="stable")
    return rows[keep][order], keys[keep][order]


def edge_keys(lo, hi, direction):
    """Every ``(b, key)`` at which the histogram and the list disagree: ``"counted"``: the
    predecessor of edge b that bins into b (counted in the picked bin, not listed);
    ``"listed"``: edge b itself binning into b - 1 (listed, not counted)."""
    b = np.arange(1, NBINS)
    e = edge(b, lo, hi)
    if direction == "counted":
        k = np.nextafter(e, -np.inf)
        ok = bin_of(k, lo, hi) == b
    else:
        assert direction == "listed"
        k = e
        ok = bin_of(k, lo, hi) == b - 1
    return b[ok], k[ok]


def find_edge_key(lo, hi, direction):
    bs, ks = edge_keys(lo, hi, direction)
    assert bs.size, "no %s edge key for [%r, %r]" % (direction, lo, hi)
    return int(bs[0]), float(ks[0])


# ---- the test of the listed candidates ------------------------------------------------
def lipschitz_margins(pts, S, rows, u, fmin, lipschitz):
    """``max over the unsafe rows of u_i - L_i d - fmin_i`` (m, G) for the candidates at local
    ``rows`` with upper bounds ``u`` (m, G): the cdist formula of
    ``_oracle_backend.lipschitz_check``; +inf in the columns without a constraint, -inf
    everywhere without an unsafe row."""
    from scipy.spatial.distance import cdist
    fmin, lipschitz = np.atleast_1d(fmin).astype(float), np.atleast_1d(lipschitz).astype(float)
    u = np.asarray(u, dtype=float).reshape(len(rows), fmin.size)
    out = np.full(u.shape, -np.inf)
    unsafe = ~np.asarray(S, dtype=bool)
    for i in range(u.shape[1]):
        if fmin[i] == -np.inf:
            out[:, i] = np.inf
            continue
        if not unsafe.any():
            continue
        for a in range(0, len(rows), 512):
            d = cdist(pts[rows[a:a + 512]], pts[unsafe])
            out[a:a + 512, i] = np.max(u[a:a + 512, [i]] - lipschitz[i] * d - fmin[i], axis=1)
    return out


def lipschitz_hits(pts, S, rows, u, fmin, lipschitz, clear=1e-9):
    """Hit per candidate (every GP with a constraint has a row; none at all: no hit, the
    reference leaves G false).  Asserts that no comparison is within ``clear`` of equality."""
    fmin = np.atleast_1d(fmin).astype(float)
    if not np.any(fmin != -np.inf):
        return np.zeros(len(rows), dtype=bool)
    m = lipschitz_margins(pts, S, rows, u, fmin, lipschitz)
    assert not np.any(np.abs(m) <= clear), "a comparison within %g of equality" % clear
    return np.all(m >= 0, axis=1)


def first_hit(rows, keys, hits):
    """k_pass_result, mode 0: the hit with the largest (key, row), or None."""
    if not np.any(hits):
        return None
    r, k = visiting_order(rows[hits], keys[hits])
    return float(k[0]), int(r[0])


# ---- scenarios ------------------------------------------------------------------------
SCENARIOS = ("a", "b", "c", "d", "e", "f", "g")
HI_COUNTED, HI_LISTED = 1.1, 0.7     # (1188 and 1027 of the 4095 edges; profiles/pass_select)
N_SHARD = 1200


class Scenario(object):
    """``points``, ``Q``: the grid of a world of 2 (rank 0 owns the first ``n`` rows, the other
    half is unsafe); ``fmin``, ``lipschitz``, ``threshold``; ``lead``: how many candidates the
    driver visits before its first big pass; ``want``: the pass size the premise was built for."""

    def parts(self):
        return self.points, self.Q, self.fmin, self.lipschitz, self.threshold

    def shard(self):
        return self.points[:self.n], self.Q[:self.n]


def _layout(dim):
    """Grid of 2 n rows, the unsafe block inside rank 0's half and the maximiser row 0."""
    n = N_SHARD
    if dim == 1:
        h = 2.0 ** -5
        pts = (np.arange(2 * n) * h)[:, None]
        unsafe = np.zeros(2 * n, dtype=bool)
        unsafe[700:760] = True
    else:
        h, cols = 2.0 ** -6, 50
        ii, jj = np.divmod(np.arange(2 * n), cols)
        pts = np.column_stack([ii * h, jj * h])
        unsafe = (ii >= 12) & (ii < 16) & (jj >= 20) & (jj < 30)
    unsafe[n:] = True
    return n, h, pts, unsafe


def scenario(name, dim=1, lead=17, want=64, seed=0):
    n, h, pts, unsafe = _layout(dim)
    rng = np.random.default_rng(1000 * dim + seed + ord(name))
    sc = Scenario()
    sc.name, sc.dim, sc.n, sc.lead, sc.want = name, dim, n, lead, want
    sc.points, sc.fmin, sc.threshold = pts, FMIN, 0.0
    sc.lipschitz = -FMIN / (1.75 * h)
    safe = np.flatnonzero(~unsafe[:n])
    safe = safe[safe != 0]                       # (row 0: the maximiser)
    # the rows that touch the unsafe block: the hits, whatever their width
    S = ~unsafe[:n]
    near = safe[lipschitz_hits(pts[:n], S, safe, np.zeros(safe.size), FMIN, sc.lipschitz)]
    near_hi = safe[lipschitz_hits(pts[:n], S, safe, np.full(safe.size, W_MAX), FMIN, sc.lipschitz)]
    assert np.array_equal(near, near_hi) and near.size == (2 if dim == 1 else 32)
    far = np.setdiff1d(safe, near)
    w = np.zeros(n)
    sc.hi = None
    if name == "a":                                   # random widths, the hits deep in the order
        w[far] = rng.uniform(0.05, 1.0, far.size)
        w[near] = rng.uniform(0.30, 0.45, near.size)
    elif name == "b":                                 # two decimals: many small tie runs
        w[far] = np.round(rng.uniform(0.05, 1.0, far.size), 2)
        w[near] = np.round(rng.uniform(0.30, 0.45, near.size), 2)
        _v, c = np.unique(w[safe], return_counts=True)
        assert c.max() >= 8 and (c >= 2).sum() >= 50
    elif name == "c":                                 # one value shared by >= 4 want candidates
        w[far] = rng.uniform(0.5, 1.0, far.size)
        mass = np.concatenate([near, rng.choice(far, 4 * want + 40, replace=False)])
        w[mass] = 0.3125
        assert (w[safe] == 0.3125).sum() >= 4 * want and np.all(w[near] == 0.3125)
    elif name in ("d", "e"):                          # a mass of edge keys under `lead` wide rows
        sc.hi = HI_COUNTED if name == "d" else HI_LISTED
        b, key = find_edge_key(0.0, sc.hi, "counted" if name == "d" else "listed")
        guard = far[:lead]                            # (the lowest rows: far from the block)
        w[safe] = key
        w[guard] = sc.hi
        low = np.setdiff1d(far, guard)[-100:]         # something below the bin as well
        w[low] = rng.uniform(0.2, 0.9, low.size) * edge(b - 1, 0.0, sc.hi)
        sc.edge_bin, sc.edge_key = b, key
    elif name == "f":                                 # everything within 1e-12: one bin
        w[safe] = 0.5 + rng.integers(0, 4096, safe.size) * 2.0 ** -53
        w[near] = 0.5 + rng.integers(0, 64, near.size) * 2.0 ** -53
        assert np.ptp(w[safe]) < 1e-12 and np.unique(w[safe]).size > 500
    elif name == "g":                                 # the cut falls inside a tie run
        w[far] = rng.uniform(0.05, 0.9, far.size)
        run = np.concatenate([near[:1], far[far > near.max()][:lead + 22]])
        w[run] = 1.0
        w[near[1:]] = 0.01
        sc.run = np.sort(run)
    else:
        raise KeyError(name)
    Q = np.empty((2 * n, 2))
    Q[:, 0], Q[:, 1] = 0.0, 0.0
    Q[:n, 1] = w
    Q[unsafe] = [-15.0, -14.0]
    Q[0] = [3.0, 3.0 + 2.0 ** -20]
    sc.Q = Q
    assert np.array_equal(Q[safe, 1] - Q[safe, 0], w[safe])       # the key is the width bit for bit
    _check_premise(sc, safe, near)
    return sc


def reference_sets(sc):
    """``S, M, G`` and the query row of the oracle on rank 0's shard."""
    from oracle import safeopt_numpy as son
    pts, Q = sc.shard()
    S, M, G = son.compute_sets([None], pts, Q, [sc.fmin], np.ones(1), sc.threshold, 2.0,
                               lipschitz=np.array([sc.lipschitz]))
    return S, M, G, son.query_index(Q, S, M, G, np.ones(1))


def _check_premise(sc, safe, near):
    """The properties that keep a scenario from going vacuous, on the reference alone."""
    pts, Q = sc.shard()
    n, w = sc.n, Q[:sc.n, 1] - Q[:sc.n, 0]
    S, M, G, _q = reference_sets(sc)
    assert np.array_equal(np.flatnonzero(M), [0]) and np.array_equal(np.flatnonzero(S & ~M), safe)
    cand = S & ~M & (w > Q[0, 1] - Q[0, 0])
    assert np.array_equal(np.flatnonzero(cand), safe)             # every other safe row
    rows, keys = visiting_order(*behind(cand, w, 0, 0, np.inf, I64_MAX))
    hits = np.isin(rows, near)
    assert np.array_equal(hits, lipschitz_hits(pts, S, rows, keys, sc.fmin, sc.lipschitz))
    # the oracle's G: one row, not among the `lead` candidates the driver visits first, and tied
    # with the first hit of the visiting order (an exact tie is numpy's to settle)
    assert G.sum() == 1 and not G[rows[:sc.lead]].any()
    pos = int(np.argmax(hits))
    assert pos >= sc.lead and w[G][0] == keys[pos]
    sc.cut = (float(keys[sc.lead - 1]), int(rows[sc.lead - 1]))   # where the big passes begin
    sc.first = (float(keys[pos]), int(rows[pos]))                 # (key, row) the device reports
    r2, k2 = behind(cand, w, 0, 0, *sc.cut)
    assert r2.size == rows.size - sc.lead
    hi, want = sc.cut[0], sc.want
    hh = hist(k2, 0.0, hi)
    b, thr, est = pick(hh, want, 0.0, hi)
    got = listed(r2, k2, thr)[0].size
    if sc.name == "c":
        assert (k2 == 0.3125).sum() >= 4 * want and np.all(k2[np.isin(r2, near)] == 0.3125)
    elif sc.name == "d":
        # counted in the picked bin, nothing in or above it is listed
        assert hi == sc.hi and b == sc.edge_bin and est == hh[b] >= want and got == 0
        assert (k2 == sc.edge_key).sum() == est and hh[b + 1:].sum() == 0
    elif sc.name == "e":
        # listed by the threshold of its own bin's edge, counted one bin below
        assert hi == sc.hi and b == sc.edge_bin - 1 and hh[b] >= want and hh[b + 1:].sum() == 0
        assert (k2 == sc.edge_key).sum() == hh[b] == got
        assert listed(r2, k2, float(edge(sc.edge_bin, 0.0, hi)))[0].size == got
    elif sc.name == "f":
        assert np.ptp(k2) < 1e-12 and hh[NBINS - 1] == k2.size and got == k2.size
    elif sc.name == "g":
        # the cut is a member of the run, members lie on both sides of it
        assert hi == 1.0 and sc.cut[1] in sc.run and (k2 == 1.0).sum() >= 20
        assert (sc.run > sc.cut[1]).sum() == sc.lead - 1 and sc.first[0] == 1.0
