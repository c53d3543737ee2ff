"""SafeOptSwarm's safe-set growth (``sgp_swarm_grow``, gp_opt.py:1089-1111) at the sizes of
config 5: 1e5 candidates against a safe set of 5e4 points, on the chip-wide kernels of
csrc/swarm.hip (the clear-of-S grid, then the candidates in blocks of kGrowBlock).

* an exact construction -- candidates on a lattice whose neighbours correlate at <= 0.6,
  near-duplicates of earlier candidates and of S points interleaved in a shuffled order --
  whose expected mask follows in O(n) from the lattice cells;
* random candidates against a NumPy reference of the sequential loop, in row blocks;
* the shapes of the small growth test and shapes that cross the block boundaries.
"""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from _gpu_common import mods, _grow_reference  # noqa: F401

pytestmark = pytest.mark.gpu

LS = np.array([0.9, 1.1, 1.0, 1.3])


def _kern(ns, kind):
    if kind == "prod":
        return (ns.RBF(2, variance=1.5, lengthscale=list(LS[:2]), ARD=True, active_dims=[0, 1]) *
                ns.Matern52(2, variance=1.2, lengthscale=list(LS[2:]), ARD=True,
                            active_dims=[2, 3], name="other"))
    return getattr(ns, kind)(4, variance=2.0, lengthscale=list(LS), ARD=True)


def _gp(gpy, kind, rng):
    X0 = rng.normal(size=(5, 4))
    return gpy.models.GPRegression(X0, rng.normal(size=(5, 1)), _kern(gpy.kern, kind),
                                   noise_var=0.01)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["RBF", "Matern52", "prod"])
def test_grow_lattice_exact_100k(mods, kind):
    """n = 100 000 candidates, m = 50 000 safe points, d = 4: the first visitor of a free
    lattice cell is accepted; a cell that S holds, or that an earlier candidate took,
    rejects.  Lattice neighbours correlate at <= 0.6 (spacing 1.2 lengthscales), members of
    one cell at > 0.99 (offsets <= 0.005 lengthscales per axis): no knife edges."""
    _, gpy, gpn, _ = mods
    from safeopt_amd import _hip
    rng = np.random.default_rng(2024)
    side, n, m = 15, 100_000, 50_000
    ncell = side ** 4
    h = 1.2 * LS                                  # lattice spacing per axis

    def points(cells):
        ijk = np.stack(np.unravel_index(cells, (side,) * 4), axis=1).astype(float)
        jit = rng.uniform(-0.005, 0.005, size=ijk.shape) * LS
        return (ijk - (side - 1) / 2) * h + jit
    # S: 50 000 points in 18 000 cells (repeats are near-duplicates of S points)
    s_cells = rng.choice(ncell, size=18_000, replace=False)
    s_of = s_cells[rng.integers(0, s_cells.size, size=m)]
    S = points(s_of)
    # candidates: cells drawn with repeats, a quarter of them in S's cells
    c_cells = np.where(rng.random(n) < 0.25, s_cells[rng.integers(0, s_cells.size, size=n)],
                       rng.integers(0, ncell, size=n))
    rng.shuffle(c_cells)
    B = points(c_cells)
    in_s = np.zeros(ncell, dtype=bool)
    in_s[s_of] = True                             # (the cells that hold a point of S)
    taken = np.zeros(ncell, dtype=bool)
    want = np.zeros(n, dtype=bool)
    for j, c in enumerate(c_cells):
        if not in_s[c] and not taken[c]:
            want[j] = True
            taken[c] = True
    ko = _kern(gpn, kind)
    scale2 = float(ko.Kdiag(np.zeros((1, 4)))[0])
    # the construction's premises, on the oracle kernel
    e = np.eye(4) * h
    assert np.max(ko.K(np.zeros((1, 4)), e) / scale2) <= 0.6
    pair = points(np.array([0, 0]))
    assert float(ko.K(pair[:1], pair[1:])[0, 0]) / scale2 > 0.99
    gp = _gp(gpy, kind, rng)
    dev = gp._fitted()
    got = _hip.swarm_grow(dev.ctx, dev, S, B, scale2, 0.95)
    assert_array_equal(got, want)
    assert 1000 < want.sum() < n - 1000


def _reference_blocks(ko, S, B, scale2, thr=0.95, rows=500):
    """The sequential loop of gp_opt.py:1089-1111 in row blocks, and the smallest distance
    of any compared covariance from the threshold."""
    n = B.shape[0]
    acc = np.zeros(n, dtype=bool)
    idx = []                                      # accepted so far
    edge = np.inf
    for r0 in range(0, n, rows):
        blk = B[r0:r0 + rows]
        ok = np.ones(blk.shape[0], dtype=bool)
        if S.shape[0]:
            for s0 in range(0, S.shape[0], 10_000):
                c = ko.K(blk, S[s0:s0 + 10_000]) / scale2
                edge = min(edge, np.min(np.abs(c - thr)))
                ok &= np.all(c <= thr, axis=1)
        if idx:
            c = ko.K(blk, B[np.array(idx)]) / scale2
            edge = min(edge, np.min(np.abs(c - thr)))
            ok &= np.all(c <= thr, axis=1)
        inner = ko.K(blk, blk) / scale2
        for i in range(blk.shape[0]):
            if not ok[i]:
                continue
            prev = [k for k in range(i) if acc[r0 + k]]
            if prev:
                c = inner[i, prev]
                edge = min(edge, np.min(np.abs(c - thr)))
                if not np.all(c <= thr):
                    continue
            acc[r0 + i] = True
            idx.append(r0 + i)
    return acc, edge


@pytest.mark.timeout(900)
@pytest.mark.parametrize("m", [0, 50_000])
def test_grow_random_20k_matches_reference(mods, m):
    """n = 20 000 random candidates (d = 4, RBF) against m random safe points."""
    _, gpy, gpn, _ = mods
    from safeopt_amd import _hip
    rng = np.random.default_rng(77 + m)
    S = rng.uniform(-4, 4, size=(m, 4))
    B = rng.uniform(-5, 5, size=(20_000, 4))
    ko = _kern(gpn, "RBF")
    scale2 = float(ko.Kdiag(np.zeros((1, 4)))[0])
    want, edge = _reference_blocks(ko, S, B, scale2)
    assert edge > 1e-9                            # no knife-edge decisions
    dev = _gp(gpy, "RBF", rng)._fitted()
    got = _hip.swarm_grow(dev.ctx, dev, S, B, scale2, 0.95)
    assert_array_equal(got, want)
    assert 0 < want.sum() < B.shape[0]


@pytest.mark.parametrize("kind,d,m,n", [("RBF", 2, 300, 40), ("Matern52", 3, 9000, 64),
                                         ("Matern32", 1, 5, 30), ("RBF", 4, 0, 25),
                                         ("prod", 3, 700, 50),
                                         # across the blocks of kGrowBlock = 512 candidates
                                         ("RBF", 2, 300, 513), ("Matern52", 3, 2000, 1500),
                                         ("RBF", 4, 0, 1100)])
def test_grow_small_shapes(mods, kind, d, m, n):
    """The shapes of the small growth test, and a few past one block of candidates."""
    _, gpy, gpn, _ = mods
    from safeopt_amd import _hip
    rng = np.random.default_rng(3 * m + n)

    def kern(ns):
        if kind == "prod":
            return (ns.RBF(2, variance=1.5, lengthscale=[0.7, 1.1], ARD=True, active_dims=[0, 1]) *
                    ns.Matern52(1, variance=1.2, lengthscale=0.9, active_dims=[2], name="context"))
        return getattr(ns, kind)(d, variance=2.0, lengthscale=list(0.5 + 0.2 * np.arange(d)),
                                 ARD=True)
    X0 = rng.normal(size=(5, d))
    gp = gpy.models.GPRegression(X0, rng.normal(size=(5, 1)), kern(gpy.kern), noise_var=0.01)
    ko = kern(gpn)
    box = 3.0 * max(1.0, (n / 40) ** (1.0 / d))
    S = rng.uniform(-box + 1, box - 1, size=(m, d))
    B = rng.uniform(-box, box, size=(n, d))
    if m:
        B[::5] = S[rng.integers(0, m, size=B[::5].shape[0])] + 0.02 * rng.normal(size=B[::5].shape)
    B[1::7] = B[:1] + 0.03 * rng.normal(size=B[1::7].shape)
    scale2 = float(ko.Kdiag(np.zeros((1, d)))[0])
    ref, cov = _grow_reference(ko.K(B, np.vstack((S, B))), m, scale2)
    off = cov[~np.eye(n, m + n, k=m, dtype=bool)]
    assert np.min(np.abs(off - 0.95)) > 1e-9          # no knife-edge decisions
    dev = gp._fitted()
    got = _hip.swarm_grow(dev.ctx, dev, S, B, scale2, 0.95)
    assert_array_equal(got, ref)
    assert 0 < ref.sum() < n
