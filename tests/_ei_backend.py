"""NumPy stand-in for the ``ei`` half of ``SafeOpt``'s grid backend, on top of
``tests/_oracle_backend.OracleGridBackend`` (which stays as it is): lets the CPU suite drive the
host logic of ``SafeOpt.ei_point`` -- incumbent, masks, the merge over ranks, errors -- without
a GPU.  Posterior from the oracle GP ONE ROW PER CALL (BLAS blocks by the number of rows: a
row of a shard then has the bits of the same row of the whole grid), alpha from
tests/_ei_ref.py.
"""
import numpy as np

import _ei_ref as ref
from _oracle_backend import OracleGridBackend

ALL, S_ROWS, MG_ROWS = 0, 1, 2


class EiOracleBackend(OracleGridBackend):
    def __init__(self, gps, inputs_shard, global_offset):
        OracleGridBackend.__init__(self, gps, inputs_shard, global_offset)
        self.calls = []

    def _posterior(self):
        for i, gp in enumerate(self.gps):
            for r in range(self.x.shape[0]):
                m, v = gp.predict_noiseless(self.x[r:r + 1])
                self.mean[r, i], self.var[r, i] = m[0, 0], v[0, 0]

    def ei(self, kind, rows, tau, xi, fmin, alpha=False, comm=False):
        assert not comm, "the stand-in has no in-stream communicator"
        self._posterior()
        self.calls.append((kind, rows, tau, xi, None if fmin is None else tuple(fmin)))
        N = self.x.shape[0]
        if isinstance(tau, str):
            over = np.ones(N, dtype=bool) if rows == ALL else self.S
            tau = self.mean[over, 0].max() if over.any() else -np.inf
        if tau == -np.inf:
            return (np.full(N, -np.inf) if alpha else None), -np.inf, -1, tau
        al = ref.alpha(self.mean.T, self.var.T, tau, xi, kind, fmin)
        mask = {ALL: np.ones(N, dtype=bool), S_ROWS: self.S, MG_ROWS: self.M | self.G}[rows]
        v, i = -np.inf, -1
        if mask.any():
            j = int(np.flatnonzero(mask)[np.argmax(al[mask])])       # first among equals
            v, i = float(al[j]), j + self.lo
        return (al if alpha else None), v, i, float(tau)


def use_ei_backend():
    """Install the stand-in (tests/conftest.py resets the hook after every test)."""
    import safeopt_amd.gp_opt as go
    go._BACKEND_FACTORY = EiOracleBackend
