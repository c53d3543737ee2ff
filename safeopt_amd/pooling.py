"""Which row of which GP holds which measurement of the log, when repeated inputs are pooled.

With ``pool_repeats=True`` an optimiser keeps its measurement log as it is -- every measurement,
in order -- while every GP is a POOLED IMAGE of its column of the log: the measurements a GP
observed at one input (context columns included, compared as float64 values) share one row of
that GP, which carries their precision-weighted mean and the noise scale of that mean
(``GPRegression.pool_data``).  ``PoolBook`` is the map between the two: log index -> row per GP,
and input row -> GP row through a dict of the row's bytes (no scan).  Pure Python, no device.

    book = PoolBook(x0, seen0)            # the initial data: one GP row per log row, as they are
    book.add(x, seen)                     # -> per GP ('pool', row) | ('append', row) | None
    book.remove(index)                    # -> per GP ('unpool', row) | ('remove', row) | None

``add`` and ``remove`` change the book and say what the GPs have to do to follow.
"""
import numpy as np


def row_key(x):
    """The bytes of an input row as float64 values; -0.0 and 0.0 compare equal, so they share
    one key."""
    return (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) + 0.0).tobytes()


class PoolBook(object):
    """The map from the measurement log to the rows of ``n_gps`` pooled GPs."""

    def __init__(self, x0, seen0):
        """``x0`` (t0, d): the initial log; ``seen0`` (t0, n_gps) bool: which GP holds which of
        its rows.  The initial data are taken as they are: one GP row per observed log row,
        equal inputs among them included."""
        x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
        seen0 = np.atleast_2d(np.asarray(seen0, dtype=bool))
        self.n_gps = seen0.shape[1]
        self.where = []                                   # [log index][gp] -> row or None
        self.count = [[] for _ in range(self.n_gps)]      # [gp][row] -> measurements in the row
        self.keys = [[] for _ in range(self.n_gps)]       # [gp][row] -> key of the row's input
        self.index = [{} for _ in range(self.n_gps)]      # [gp]{key} -> row that takes repeats
        for x, seen in zip(x0, seen0):
            key = row_key(x)
            self.where.append([self._new_row(g, key) if seen[g] else None
                               for g in range(self.n_gps)])

    t = property(lambda self: len(self.where))

    def rows(self, g):
        """Number of rows of GP ``g``."""
        return len(self.count[g])

    def _new_row(self, g, key):
        row = len(self.count[g])
        self.count[g].append(1)
        self.keys[g].append(key)
        self.index[g].setdefault(key, row)                # (the first of equal rows takes repeats)
        return row

    def match(self, x, g):
        """The row of GP ``g`` whose input equals ``x``, or None."""
        return self.index[g].get(row_key(x))

    def add(self, x, seen):
        """Log one more measurement at ``x``, observed by the GPs flagged in ``seen``.  Per GP:
        ``('pool', row)`` -- the row holds that input already --, ``('append', row)`` -- a new
        row, the GP's last --, or None."""
        key = row_key(x)
        acts, where = [], []
        for g in range(self.n_gps):
            if not seen[g]:
                acts.append(None)
                where.append(None)
                continue
            row = self.index[g].get(key)
            if row is None:
                row = self._new_row(g, key)
                acts.append(('append', row))
            else:
                self.count[g][row] += 1
                acts.append(('pool', row))
            where.append(row)
        self.where.append(where)
        return acts

    def locate(self, index):
        """Per GP the row that holds measurement ``index`` of the log, or None."""
        return list(self.where[index])

    def members(self, g, row):
        """The log indices of the measurements in row ``row`` of GP ``g``, ascending."""
        return [j for j, w in enumerate(self.where) if w[g] == row]

    def remove(self, index):
        """Forget measurement ``index`` of the log (the later ones move one down).  Per GP:
        ``('unpool', row)`` -- the row keeps other measurements --, ``('remove', row)`` -- the
        row leaves the GP, the rows behind it move one up --, or None."""
        if not 0 <= index < len(self.where):
            raise IndexError("measurement %r of %d" % (index, len(self.where)))
        acts = []
        for g, row in enumerate(self.where[index]):
            if row is None:
                acts.append(None)
            elif self.count[g][row] > 1:
                self.count[g][row] -= 1
                acts.append(('unpool', row))
            else:
                acts.append(('remove', row))
                self._drop_row(g, row)
        del self.where[index]
        return acts

    def _drop_row(self, g, row):
        key = self.keys[g][row]
        del self.count[g][row]
        del self.keys[g][row]
        for w in self.where:
            if w[g] is not None and w[g] > row:
                w[g] -= 1
        idx = self.index[g]
        if idx.get(key) == row:
            del idx[key]
        for k, r in idx.items():
            if r > row:
                idx[k] = r - 1
        if key not in idx and key in self.keys[g]:        # another of equal initial rows
            idx[key] = self.keys[g].index(key)

    def image(self, g, x, y, rho=None):
        """The pooled data of GP ``g`` from the log ``x`` (t, d), ``y`` (t, n_gps) and the
        noise scales ``rho`` (t, n_gps; None: ones): ``(X, ybar, r, k)`` per row of the GP --
        ``r = 1 / sum_j 1/rho_j``, ``ybar = r sum_j y_j / rho_j``, ``k`` measurements."""
        n = self.rows(g)
        X = np.zeros((n, np.shape(x)[1]))
        s1, sy, k = np.zeros(n), np.zeros(n), np.zeros(n, dtype=int)
        for j, w in enumerate(self.where):
            row = w[g]
            if row is None:
                continue
            p = 1.0 if rho is None else rho[j][g]
            X[row] = x[j]
            s1[row] += 1.0 / p
            sy[row] += y[j][g] / p
            k[row] += 1
        return X, sy / s1, 1.0 / s1, k
