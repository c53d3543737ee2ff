"""The host drivers of the big passes (``SafeOpt._visit_in_big_passes`` over ``_pass_n_ranks``)
through the scenarios of tests/_pass_ref.py, without a GPU: the NumPy stand-in backend restates the
device's binning, rank 0 of a pretended world of 2 owns the first half of the grid.

What must hold, whatever the pass sizes: ``S / M / G`` and the query point are the oracle's on that
half; the passes list every candidate behind the cut at which they begin exactly once, down to the
threshold of the pass that holds the first expander; no pass lists a row at or ahead of its cut;
the first expander is found by the LAST pass, and no two consecutive passes list nothing (a pass that
lists nothing over a non-empty histogram is not the end of the loop: scenario (d), where the parent
of this test's commit returned an empty ``G``).
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

import _pass_ref as pr
import safeopt_amd
from safeopt_amd import dist
from oracle import gp_numpy as gpn
from _oracle_backend import use_oracle_backend

PASS_SIZES = [(16,), (64,), (8, 16), None]


class _TwoRanksPadded(dist.LocalComm):
    """Rank 0 of a world of 2 whose other rank sends zeros: no rows, no candidates."""
    rank, world = 0, 2

    def allgather(self, a):
        a = np.asarray(a)[None, ...]
        return np.concatenate([a, np.zeros_like(a)])


class Recorder(object):
    """Wraps ``pass_hist`` / ``pass_list`` of a backend: the cut, range and threshold of every
    pass and the rows and keys it listed; two consecutive empty passes end the test."""

    def __init__(self, be):
        self.passes, self._hist, self._list = [], be.pass_hist, be.pass_list
        be.pass_hist, be.pass_list = self.hist, self.list

    def hist(self, mode, cut_w, cut_idx, lo, hi, *a):
        self.cur = dict(mode=mode, cut=(cut_w, cut_idx), lo=lo, hi=hi)
        return self._hist(mode, cut_w, cut_idx, lo, hi, *a)

    def list(self, mode, cut_w, cut_idx, thr, cap):
        assert (cut_w, cut_idx) == self.cur["cut"] and (mode & 1) == self.cur["mode"]
        out = self._list(mode, cut_w, cut_idx, thr, cap)
        self.passes.append(dict(self.cur, thr=thr, rows=np.array(out[0]), keys=np.array(out[1])))
        assert len(self.passes) < 2 or self.passes[-1]["rows"].size or self.passes[-2]["rows"].size, \
            "two consecutive passes listed nothing (pass %d)" % len(self.passes)
        return out


def check_walk(sc, passes, cand, w, goff=0):
    """The recorded passes against the reference walk from the cut of the first one."""
    assert passes, "the loop never reached a big pass"
    cut0 = passes[0]["cut"]
    assert cut0 == sc.cut
    rows0, keys0 = pr.behind(cand, w, goff, 0, *cut0)
    pts, Q = sc.shard()
    S = Q[:, 0] > sc.fmin
    seen = []
    for k, p in enumerate(passes):
        # exactly { behind this pass's cut, key >= its threshold }, ascending rows, widths bit for bit
        r, kk = pr.listed(*pr.behind(cand, w, goff, p["mode"], *p["cut"]), p["thr"])
        assert_array_equal(p["rows"], r)
        assert_array_equal(p["keys"], kk)
        hits = pr.lipschitz_hits(pts, S, p["rows"] - goff, Q[p["rows"] - goff, 1], sc.fmin,
                                 sc.lipschitz)
        assert hits.any() == (k == len(passes) - 1), "pass %d of %d" % (k, len(passes))
        seen.append(p["rows"])
    seen = np.concatenate(seen)
    assert np.unique(seen).size == seen.size                       # each exactly once
    want = rows0[keys0 >= passes[-1]["thr"]]
    assert_array_equal(np.sort(seen), np.sort(want))               # and nothing skipped
    assert sc.first[1] in seen
    return [int(p["rows"].size) for p in passes]


def drive(sc, pass_sizes, comm):
    gp = gpn.GPRegression(np.zeros((1, sc.dim)), np.ones((1, 1)), gpn.RBF(sc.dim), noise_var=0.01)
    opt = safeopt_amd.SafeOpt(gp, sc.points, sc.fmin, lipschitz=sc.lipschitz,
                              threshold=sc.threshold, comm=comm)
    if pass_sizes is not None:
        opt.pass_sizes = pass_sizes
    assert opt._shard == (0, sc.n) and np.all(opt.scaling == 1.0)
    opt.Q = sc.Q
    rec = Recorder(opt._backend)
    opt.compute_sets()
    return opt, rec


@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("name", pr.SCENARIOS)
def test_n_rank_driver_walks_every_candidate(name, dim):
    use_oracle_backend()
    for sizes in PASS_SIZES:
        sc = pr.scenario(name, dim, lead=17, want=64 if sizes is None else sizes[0])
        S, M, G, q = pr.reference_sets(sc)
        opt, rec = drive(sc, sizes, _TwoRanksPadded())
        be = opt._backend
        assert_array_equal(be.S, S)
        assert_array_equal(be.M, M)
        assert_array_equal(np.flatnonzero(be.G), np.flatnonzero(G))
        assert_array_equal(opt.get_new_query_point(), sc.points[q])
        tested = check_walk(sc, rec.passes, be.cand, be.w)
        if name in ("c", "f"):
            print("scenario (%s) %d-D, pass_sizes %s: tested per pass %s" % (name, dim, sizes, tested))
        if name == "d" and sizes is not None:
            # the pass that counted the mass and listed nothing, then the one that lists it
            assert tested[0] == 0 and tested[1] >= 4 * sizes[0]


def test_edge_keys_exist_in_both_directions():
    """``find_edge_key`` on the ranges the scenarios use, and the edges that disagree per range."""
    for hi in (pr.HI_COUNTED, pr.HI_LISTED, 0.3, 1.7):
        n = {d: pr.edge_keys(0.0, hi, d)[0].size for d in ("counted", "listed")}
        print("hi = %g: %d edges counted-not-listed, %d listed-not-counted" % (
            hi, n["counted"], n["listed"]))
    b, k = pr.find_edge_key(0.0, pr.HI_COUNTED, "counted")
    assert pr.bin_of(k, 0.0, pr.HI_COUNTED) == b and k < pr.edge(b, 0.0, pr.HI_COUNTED)
    assert (b, k.hex()) == (7, "0x1.ecccccccccccdp-10")
    b, k = pr.find_edge_key(0.0, pr.HI_LISTED, "listed")
    assert pr.bin_of(k, 0.0, pr.HI_LISTED) == b - 1 and k == pr.edge(b, 0.0, pr.HI_LISTED)
    assert pr.edge_keys(0.0, pr.HI_COUNTED, "counted")[0].size == 1188
    assert pr.edge_keys(0.0, pr.HI_LISTED, "listed")[0].size == 1027


def test_pick_restates_the_driver():
    """``_pass_ref.pick`` against the arithmetic of ``_pass_n_ranks`` on random histograms."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        h = rng.integers(0, 4, pr.NBINS) * (rng.random(pr.NBINS) < rng.choice([0.002, 0.05, 1.0]))
        want = int(rng.choice([1, 8, 64, 1000, 10 ** 6]))
        from_top = np.cumsum(h[::-1])
        b = pr.NBINS - 1 - int(np.argmax(from_top >= want)) if from_top[-1] >= want else 0
        thr = -np.inf if b == 0 else 0.0 + (1.1 - 0.0) * (float(b) / pr.NBINS)
        assert pr.pick(h, want, 0.0, 1.1)[:2] == (b, thr)
