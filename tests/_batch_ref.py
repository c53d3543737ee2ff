"""NumPy restatement of ``SafeOpt.optimize_batch`` (GP-BUCB on SafeOpt's rule).

TEST INFRASTRUCTURE.  The same quantity computed the slow way: instead of chained rank-1
downdates of a variance buffer, the oracle GPs (``oracle/gp_numpy.py``) are REFITTED on the
training inputs plus the hallucinated ones and predict the variance over the whole grid.  ``Y``
is extended by zeros: the posterior variance does not depend on it.  The means, ``S``, ``M`` and
``G`` are those of the real data and are arguments.
"""
import numpy as np

from oracle import gp_numpy as gpn

MG_WIDTH, UCB = 0, 1


def refit_variances(gps, grid, picked_x):
    """``(G, N)``: the variance over ``grid`` of every GP refitted on ``X`` and ``picked_x``."""
    picked_x = np.asarray(picked_x, dtype=float).reshape(-1, grid.shape[1])
    out = np.empty((len(gps), grid.shape[0]))
    for i, gp in enumerate(gps):
        X = np.vstack([gp.X, picked_x])
        Y = np.vstack([gp.Y, np.zeros((picked_x.shape[0], 1))])
        twin = gpn.GPRegression(X, Y, gp.kern, noise_var=gp.noise_var)
        out[i] = twin.predict_noiseless(grid)[1].ravel()
    return out


def intervals(mean, var_h, beta):
    """Hallucinated ``(l, u)``, each ``(G, N)``, from the real means ``(G, N)``."""
    sd = np.sqrt(var_h)
    return mean - beta * sd, mean + beta * sd


def rule_values(mean, var_h, beta, scaling, mode):
    """The value of rule 3 per row: ``max_i (u_i - l_i) / scaling_i``, or ``u_0``."""
    lo, up = intervals(mean, var_h, beta)
    if mode == UCB:
        return up[0].copy()
    return np.max((up - lo) / np.asarray(scaling, dtype=float)[:, None], axis=0)


def pick(values, mask, taken):
    """``(row, margin)``: the arg-max of ``values`` over the rows of ``mask`` that are not in
    ``taken`` -- the lowest row among equal values -- and the margin between the best and the
    second-best eligible value (inf with one eligible row).  ``(-1, inf)``: no row left."""
    ok = np.array(mask, dtype=bool)
    ok[np.asarray(list(taken), dtype=np.int64)] = False
    rows = np.flatnonzero(ok)
    if rows.size == 0:
        return -1, np.inf
    v = values[rows]
    j = int(np.argmax(v))                       # (first among equals)
    rest = np.delete(v, j)
    return int(rows[j]), (float(v[j] - rest.max()) if rest.size else np.inf)


def batch(gps, grid, mean, S, M, G, row0, size, beta, scaling, mode, forced=None):
    """The batch behind ``row0``.  ``forced``: teacher forcing -- the rows somebody else
    picked are hallucinated instead of the restatement's own, so that every pick is judged
    on the same earlier picks.  Returns ``(rows, downdates, var_h, values, margins)``:
    ``var_h`` ``(G, N)`` after the last downdate, and per pick after the first the value
    array it was taken from and its margin."""
    mask = (np.asarray(M) | np.asarray(G)) if mode == MG_WIDTH else np.asarray(S)
    rows, values, margins, downdates = [int(row0)], [], [], 0
    var_h = refit_variances(gps, grid, np.empty((0, grid.shape[1])))
    for b in range(1, size):
        if forced is not None and b > len(forced):
            break
        used = [int(r) for r in (forced[:b] if forced is not None else rows[:b])]
        var_h = refit_variances(gps, grid, grid[used])
        downdates += 1
        val = rule_values(mean, var_h, beta, scaling, mode)
        r, margin = pick(val, mask, used)
        if r < 0:
            break
        rows.append(r)
        values.append(val)
        margins.append(margin)
    return np.asarray(rows, dtype=np.int64), downdates, var_h, values, margins
